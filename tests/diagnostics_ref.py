"""Yardstick of the convergence diagnostics (csrc/diag.hip): a direct float64 numpy restatement of
the estimator — split-chain R-hat and mean ESS of BDA3 / Stan / ArviZ without rank normalisation —
with the autocovariance by explicit sums (no FFT), plus the AR(1) input sets the tests share.

``series_stats(y)`` returns the six statistics (mean, sd, mcse, ess, rhat, lag) and the decision
margin of Geyer's truncation: the minimum over the loop of |even + odd| at every evaluated pair and
|even| at the end — how far the nearest comparison against zero was from going the other way,
which is the condition for comparing the truncation lag exactly.
"""
from __future__ import annotations

import functools

import numpy as np

STATS = ("mean", "sd", "mcse", "ess", "rhat", "lag")


def series_stats(y, log: bool = False):
    """y: (m, n) chains x draws, m >= 1, n >= 8.  Returns (stats[6], margin)."""
    y = np.asarray(y, dtype=np.float64)
    if log:
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.log(y)
    m, n = y.shape
    nan = np.full(6, np.nan)
    if not np.isfinite(y).all():
        return nan, np.inf
    mean = y.mean()
    sd = y.std(ddof=1)
    h = n // 2
    M = 2 * m
    split = np.concatenate([y[:, :h], y[:, n - h:]], axis=0)  # (M, h); the order of split chains is immaterial
    mu = split.mean(axis=1)
    c = split - mu[:, None]

    @functools.lru_cache(maxsize=None)
    def a(t):  # mean over split chains of the biased autocovariance at lag t
        return float(np.mean(np.sum(c[:, :h - t] * c[:, t:], axis=1) / h))

    W = a(0) * h / (h - 1)
    if W == 0:
        return nan, np.inf
    V = a(0) + np.var(mu, ddof=1)
    rhat = np.sqrt(V / W)

    def rho(t):
        return 1.0 - (W - a(t)) / V

    r = np.zeros(h + 2)
    r[0] = 1.0
    r[1] = rho(1)
    t, even, odd = 1, 1.0, r[1]
    margin = np.inf
    while t < h - 3 and even + odd > 0:
        even, odd = rho(t + 1), rho(t + 2)
        margin = min(margin, abs(even + odd))
        if even + odd >= 0:
            r[t + 1], r[t + 2] = even, odd
        t += 2
    T = t - 2
    margin = min(margin, abs(even))
    if even > 0:
        r[T + 1] = even
    t = 1
    while t <= T - 2:
        if r[t + 1] + r[t + 2] > r[t - 1] + r[t]:
            r[t + 1] = (r[t - 1] + r[t]) / 2
            r[t + 2] = r[t + 1]
        t += 2
    tau = -1.0 + 2.0 * np.sum(r[:T + 1]) + r[T + 1]
    tau = max(tau, 1.0 / np.log10(M * h))
    ess = M * h / tau
    return np.array([mean, sd, sd / np.sqrt(ess), ess, rhat, float(T)]), margin


def stats_many(arr, log_mask: int = 0, period: int = 1):
    """arr: (m, n, n_series), the C ABI's layout.  Returns (stats[n_series][6], margins[n_series])."""
    arr = np.asarray(arr, dtype=np.float64)
    ns = arr.shape[2]
    out = np.empty((ns, 6))
    mg = np.empty(ns)
    for s in range(ns):
        out[s], mg[s] = series_stats(arr[:, :, s], log=bool((log_mask >> (s % period)) & 1))
    return out, mg


def autocorr(y, max_lag: int):
    """Per-chain ACF of az.plot_autocorr: y (m, n) -> (m, max_lag + 1), A_c(t) / A_c(0) on the unsplit
    chain centred at its mean, divisor n."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[1]
    c = y - y.mean(axis=1, keepdims=True)
    A = np.stack([np.sum(c[:, :n - t] * c[:, t:], axis=1) / n for t in range(max_lag + 1)], axis=1)
    return A / A[:, :1]


def ar1(rng_or_seed, m: int, n: int, phi: float):
    """x_0 = e_0, x_i = phi x_{i-1} + sqrt(1 - phi^2) e_i, e = standard_normal((m, n)) in one call."""
    rng = np.random.default_rng(rng_or_seed) if not isinstance(rng_or_seed, np.random.Generator) else rng_or_seed
    e = rng.standard_normal((m, n))
    x = np.empty((m, n))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + s * e[:, i]
    return x


SMALL_SHAPES = ((4, 250), (2, 101), (1, 64), (3, 16))
MIN_SHAPES = ((2, 8), (2, 9), (1, 8), (4, 11))
LONG_SHAPE = (4, 6000)


@functools.lru_cache(maxsize=None)
def small_set():
    """Seed 7; for k in range(512), phi = (k % 8) / 8 * 0.95, the four SMALL_SHAPES in that order (one
    generator call per series).  Returns {shape: (m, n, 512)}."""
    rng = np.random.default_rng(7)
    out = {sh: np.empty(sh + (512,)) for sh in SMALL_SHAPES}
    for k in range(512):
        phi = (k % 8) / 8 * 0.95
        for sh in SMALL_SHAPES:
            out[sh][:, :, k] = ar1(rng, sh[0], sh[1], phi)
    return out


@functools.lru_cache(maxsize=None)
def min_set():
    """Seed 11; 256 series of each of MIN_SHAPES (phi cycling as in the small set), shape by shape."""
    rng = np.random.default_rng(11)
    out = {}
    for sh in MIN_SHAPES:
        a = np.empty(sh + (256,))
        for k in range(256):
            a[:, :, k] = ar1(rng, sh[0], sh[1], (k % 8) / 8 * 0.95)
        out[sh] = a
    return out


@functools.lru_cache(maxsize=None)
def long_set():
    """Seed 13; 8 series of (4, 6000) at phi = 0.99 (192 KB each: the global-memory path)."""
    rng = np.random.default_rng(13)
    a = np.empty(LONG_SHAPE + (8,))
    for k in range(8):
        a[:, :, k] = ar1(rng, LONG_SHAPE[0], LONG_SHAPE[1], 0.99)
    return a


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(stats, margins) of a named input set, computed once per session and shared (read-only)."""
    if name.startswith("small:") or name.startswith("min:"):
        kind, m, n = name.split(":")
        arr = (small_set() if kind == "small" else min_set())[(int(m), int(n))]
        st, mg = stats_many(arr)
    elif name == "long":
        st, mg = stats_many(long_set())
    else:
        raise KeyError(name)
    st.setflags(write=False)
    mg.setflags(write=False)
    return st, mg


@functools.lru_cache(maxsize=None)
def golden_level1(kind: str):
    """Real level-1 draws of tests/golden/analysis_abe400.npz ("bi": (2, 30, 400, 4), "tri":
    (2, 20, 400, 5)) with lambda and mu logged: (draws, width, log mask, stats, margins)."""
    import os
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis_abe400.npz"),
                allow_pickle=False)
    a = np.ascontiguousarray(f[f"{kind}_level1"], dtype=np.float64)
    w = a.shape[3]
    st, mg = stats_many(a.reshape(a.shape[0], a.shape[1], -1), log_mask=0b11, period=w)
    for x in (a, st, mg):
        x.setflags(write=False)
    return a, w, 0b11, st, mg

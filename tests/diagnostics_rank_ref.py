"""Yardstick of the rank-normalised diagnostics (csrc/diag_rank.hip): a float64 numpy / scipy
restatement of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021) as ArviZ implements them, on
top of ``diagnostics_ref.series_stats`` (the split-chain ESS / R-hat / truncation lag and its
decision margin).

Notation: y the (logged) series of m x n values, h = n // 2, M = 2 m; split chains y[c, :h] and
y[c, n - h:] (the middle draw of an odd n is dropped), in the order (chain 0 first half, chain 0
second half, chain 1 first half, ...), S = M h pooled values.

``rank_series_stats(y)`` returns the thirteen statistics of ``STATS`` and the decision margins of
the four ESS evaluations (``MARGINS``: bulk, q05, q95, sd).
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from tests import diagnostics_ref as R

STATS = ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "ess_sd", "mcse_sd",
         "hdi_lo", "hdi_hi", "median", "lag_bulk")
(RHAT, RHAT_BULK, RHAT_FOLDED, ESS_BULK, ESS_TAIL, ESS_Q05, ESS_Q95, ESS_SD, MCSE_SD, HDI_LO, HDI_HI, MEDIAN,
 LAG_BULK) = range(len(STATS))
MARGINS = ("bulk", "q05", "q95", "sd")
_ESS, _RHAT, _LAG = 3, 4, 5  # columns of diagnostics_ref.series_stats


def split_chains(y):
    """(m, n) -> (2 m, h) in split-chain order."""
    y = np.asarray(y, dtype=np.float64)
    m, n = y.shape
    h = n // 2
    return np.stack([y[:, :h], y[:, n - h:]], axis=1).reshape(2 * m, h)


def average_ranks(s):
    """Average 1-based ranks over all pooled values of the split chains s (M, h)."""
    return rankdata(s.ravel(), method="average").reshape(s.shape)


def zscale_arg(r, S):
    return (r - 0.375) / (S + 0.25)


def zscale(s):
    """(ranks, z) of the split chains s (M, h)."""
    r = average_ranks(s)
    return r, ndtri(zscale_arg(r, s.size))


def _split_stats(s):
    """series_stats of already-split chains s (M, h): fed as (m, 2 h) rows, so that the yardstick's
    own split reproduces them."""
    M, h = s.shape
    return R.series_stats(s.reshape(M // 2, 2 * h))


def hdi(values, prob):
    x = np.sort(np.asarray(values, dtype=np.float64).ravel())
    N = x.size
    k = min(int(np.floor(prob * N)), N - 1)
    i = int(np.argmin(x[k:] - x[:N - k]))
    return x[i], x[i + k]


def rank_series_stats(y, log: bool = False, hdi_prob: float = 0.94):
    """y: (m, n), m >= 1, n >= 8.  Returns (stats[13], margins[4])."""
    y = np.asarray(y, dtype=np.float64)
    if log:
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.log(y)
    out = np.full(len(STATS), np.nan)
    mg = np.full(len(MARGINS), np.inf)
    if not np.isfinite(y).all():
        return out, mg
    s = split_chains(y)
    _, z = zscale(s)
    st, mg[0] = _split_stats(z)
    out[RHAT_BULK], out[ESS_BULK], out[LAG_BULK] = st[_RHAT], st[_ESS], st[_LAG]
    _, zf = zscale(np.abs(s - np.median(s)))
    out[RHAT_FOLDED] = _split_stats(zf)[0][_RHAT]
    out[RHAT] = max(out[RHAT_BULK], out[RHAT_FOLDED]) if np.isfinite(out[[RHAT_BULK, RHAT_FOLDED]]).all() else np.nan
    for k, (col, p) in enumerate(((ESS_Q05, 0.05), (ESS_Q95, 0.95))):
        q = np.quantile(y.ravel(), p)
        st, mg[1 + k] = _split_stats((s <= q).astype(np.float64))
        out[col] = st[_ESS]
    out[ESS_TAIL] = min(out[ESS_Q05], out[ESS_Q95]) if np.isfinite(out[[ESS_Q05, ESS_Q95]]).all() else np.nan
    mean = y.mean()
    c2 = (y - mean) ** 2
    st, mg[3] = _split_stats(split_chains(c2))
    out[ESS_SD] = st[_ESS]
    evar = c2.mean()
    if evar != 0 and np.isfinite(out[ESS_SD]):
        varvar = (np.mean(c2 * c2) - evar * evar) / out[ESS_SD]
        out[MCSE_SD] = np.sqrt(varvar / evar / 4.0)
    out[HDI_LO], out[HDI_HI] = hdi(y, hdi_prob)
    out[MEDIAN] = np.median(y)
    return out, mg


def rank_stats_many(arr, log_mask: int = 0, period: int = 1, hdi_prob: float = 0.94):
    """arr: (m, n, n_series), the C ABI's layout.  Returns (stats[n_series][13], margins[n_series][4])."""
    arr = np.asarray(arr, dtype=np.float64)
    ns = arr.shape[2]
    out = np.empty((ns, len(STATS)))
    mg = np.empty((ns, len(MARGINS)))
    for k in range(ns):
        out[k], mg[k] = rank_series_stats(arr[:, :, k], log=bool((log_mask >> (k % period)) & 1), hdi_prob=hdi_prob)
    return out, mg


@functools.lru_cache(maxsize=None)
def threshold_set(n: int):
    """Seed 17; 3 series of 2 x n draws at phi = 0.9 (n = half an LDS threshold, or one more)."""
    rng = np.random.default_rng(17)
    a = np.stack([R.ar1(rng, 2, n, 0.9) for _ in range(3)], axis=2)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(stats, margins) of a named input set at hdi_prob 0.94, computed once per session and shared
    (read-only): "small:m:n", "min:m:n", "long", "threshold:n", "golden:bi", "golden:tri"."""
    if name.startswith("small:") or name.startswith("min:"):
        kind, m, n = name.split(":")
        st, mg = rank_stats_many((R.small_set() if kind == "small" else R.min_set())[(int(m), int(n))])
    elif name == "long":
        st, mg = rank_stats_many(R.long_set())
    elif name.startswith("threshold:"):
        st, mg = rank_stats_many(threshold_set(int(name.split(":")[1])))
    elif name.startswith("golden:"):
        a, w, mask, _, _ = R.golden_level1(name.split(":")[1])
        st, mg = rank_stats_many(a.reshape(a.shape[0], a.shape[1], -1), log_mask=mask, period=w)
    else:
        raise KeyError(name)
    st.setflags(write=False)
    mg.setflags(write=False)
    return st, mg

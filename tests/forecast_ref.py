"""float64 model of csrc/forecast.hip (the closed-form holdout predictive distribution and its
scores), the same definitions in 40-digit mpmath, and the inputs the tests share.

The model follows fc_draw's operations in its order (the shared-exponent downward recurrence, the
mode start, the starting series and the two closed branches), vectorised over
(draw, customer), and adds the draws in draw order as the device does: what differs on the device is
its exp, log, log1p, expm1 and lgamma.  The mpmath functions follow include/clvmcmc.h's definitions
literally, with gammainc(..., regularized=True) for P, and take the float64 inputs as exact numbers.

E_PMF and E_STAT are the model's largest deviation from mpmath ON THE 64 x 100 FIXTURE of
tests/test_forecast_cpu.py (widths 4 and 5, k_max 64, with and without the extreme draws), which
measures and asserts them:
  E_PMF   relative, over the entries >= 1e-290 of the mean pmf: measured 2.91e-14, recorded 3e-14.  It
          is the rounding of the recurrence: 1 / a and ml / lambda are rounded once and multiplied in
          at every step, so the error grows in proportion to the steps, about k_max eps / 2 each;
  E_STAT  over xstar_mean and p_alive relative, over log_score and rps relative to max(|value|, 1)
          (log p is conditioned 1 / |log p| as p -> 1 and rps = sum (F - 1)^2 cancels as F -> 1, so
          neither has a relative bound where it is small): measured 2.27e-15 (rps; 7.3e-16 on the relative pair), recorded 3e-15.
They are the unit of the GPU tolerances, not a bound on the model elsewhere.

The GPU tolerances (pmf_tol, stat_tol below), fixed from documented bounds before any device run:
the device runs the model's operations in the model's order without fused multiply-add, so it shares
the recurrence's rounding, which grows with the steps: E_PMF (k_max / 64).  What it swaps is numpy's
exp, log, log1p, expm1 and lgamma for the device library's, documented at <= 1 ulp for the first
four and <= 4 ulp for lgamma in float64.  They enter a pmf value through the exponent of the start
g_m = exp((m log a - lgamma(m + 1)) - y), m = floor(lambda t): an error of u ulp in a term of size M
moves the result by u M 2^-53 relative.  On the GPU fixture (gpu_case; test_forecast_cpu.py asserts
these figures) the largest exponent arguments of a draw whose g does not underflow are
m log a <= 247, lgamma(m + 1) <= 189, y <= 62, so the device may add
(1 * 247 + 4 * 189 + 1 for exp itself) 2^-53 = 1.12e-13 = 3.7 E_PMF; the draws with log lambda = 70 start
from log w + (k_max - 1) log r, |.| <= 141, and the draws with mu = e^5 give values hundreds of orders
below the other draws' at the same k.  DEVICE_MARGIN = 5 = 1 + 3.7 rounded up:
  pmf_tol(k_max)  = E_PMF (k_max / 64 + DEVICE_MARGIN - 1)   relative, entries >= 1e-290; also the
                    bound on log_score, whose absolute error is the relative error of pmf(x*);
  stat_tol(k_max) = E_STAT (k_max / 64 + DEVICE_MARGIN - 1)  for the other statistics, measured as
                    E_STAT is (their functions take arguments of order 1 to 62: a few ulp)."""
import functools
import math
import os

import numpy as np

from tests.ic_ref import synth_case  # noqa: F401  (the shared inputs)

STATS = ("xstar_mean", "p_alive", "p_zero", "q05", "q50", "q95", "tail_mass", "log_score", "pit_lo", "pit_hi", "rps")
E_PMF = 3e-14
E_STAT = 3e-15
DEVICE_MARGIN = 5.0
GPU_MAX_MLOGA, GPU_MAX_LGAMMA, GPU_MAX_Y = 247.0, 189.0, 62.0   # the margin's inputs (docstring)
PMF_FLOOR = 1e-290
TINY = 2.0 ** -800
P1_EXPONENT = 45.0
SER_CAP = 4096
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")


def holdout_counts(N, seed, k_max=64):
    """x_star of N customers: Poisson(3) counts with customer 0 at 0 and customer 1 at k_max - 1."""
    xs = np.random.default_rng(seed + 77).poisson(3.0, N).astype(np.int32)
    xs = np.minimum(xs, k_max - 1)
    xs[0] = 0
    if N > 1:
        xs[1] = k_max - 1
    return xs


def default_k_max(x_star=None):
    top = 63 if x_star is None or len(x_star) == 0 else max(63, int(np.max(x_star)))
    return 64 * int(math.ceil((top + 1) / 64))


# ---- the float64 model ----------------------------------------------------------------------------
def _exp_scaled(l):
    """exp(l) as (m, e): m 2^e, e = 0 while l >= -700; 0 below -1e8 or NaN."""
    with np.errstate(all="ignore"):
        ok = l > -1e8
        big = ok & (l < -700.0)
        nd = np.where(big, np.rint(l * LOG2E), 0.0)
        m = np.where(ok, np.exp(np.where(ok, l - nd * LN2, 0.0)), 0.0)
    return m, nd.astype(np.int64)


def _ilogb(v):
    return np.frexp(v)[1].astype(np.int64) - 1


_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def draw_pmf(lam, mu, dT, t, K):
    """(pmf [..., K], p_alive, mean) of arrays lam, mu (any shape) and dT broadcast to it, the
    operations in fc_draw's order.  (The device skips the recurrence of a draw whose p_alive is exactly
    0; here its terms are formed and multiplied by that 0: the same values.)"""
    lam, mu = np.asarray(lam, np.float64), np.asarray(mu, np.float64)
    dT = np.broadcast_to(dT, lam.shape)
    shape = lam.shape
    top = K - 1
    with np.errstate(all="ignore"):
        ml = lam + mu
        E = np.exp(-(ml * dT))
        den = mu + lam * E
        pa = (ml * E) / den
        pd = (mu * (-np.expm1(-(ml * dT)))) / den
        mean = (pa * (lam / mu)) * (-np.expm1(-(mu * t)))
        y, a, w, r = ml * t, lam * t, mu / ml, lam / ml
        tiny = ~((a >= TINY) & (r >= TINY))
        rinv, ainv = ml / lam, 1.0 / a
        m = np.fmin(np.floor(a), float(top))
        m = np.where(np.isfinite(m), m, 0.0)
        lg = np.where(m > 0, (m * np.log(a) - _lgamma(m + 1.0)) - y, -y)
        gh, e = _exp_scaled(lg)
        mi = m.astype(np.int64)
        for k in range(int(mi.min()), top):
            on = mi <= k
            gh = np.where(on, gh * (a / float(k + 1)), gh)
            low = on & (gh < 2.0 ** -128) & (gh > 0.0)
            if low.any():
                s = np.where(low, _ilogb(np.where(low, gh, 1.0)), 0)
                gh = np.ldexp(gh, -s)
                e = e + s
        dK = float(K)
        p1 = (y > 1e300) | ((y > dK) & ((y - dK) - dK * np.log(y / dK) > P1_EXPONENT))
        vm, ev = _exp_scaled(np.log(w) + float(top) * (-np.log1p(mu / lam)))
        # closed branch 1: align the two exponents
        g0, v0, up = gh == 0.0, vm == 0.0, ev >= e
        gh1 = np.where(g0 | v0 | ~up, gh, np.ldexp(gh, np.maximum(e - ev, -2000)))
        vh1 = np.where(g0, vm, np.where(v0, 0.0, np.where(up, vm, np.ldexp(vm, np.maximum(ev - e, -2000)))))
        e1 = np.where(g0 | (~v0 & up), ev, e)
        # the series
        term = y / dK
        S = term.copy()
        done = p1 | tiny | ~np.isfinite(y)
        for j in range(1, SER_CAP):
            if done.all():
                break
            kj = dK + float(j)
            term = np.where(done, term, term * (y / kj))
            S = np.where(done, S, S + term)
            done = done | ((kj + 1.0 > y) & (term * y < (2.0 ** -60 * S) * ((kj + 1.0) - y)))
        vh = np.where(p1, vh1, (w * S) * gh)
        gh = np.where(p1, gh1, gh)
        e = np.where(p1, e1, e)
        pmf = np.zeros(shape + (K,))
        for k in range(top, -1, -1):
            mx = np.fmax(gh, vh)
            ren = (mx >= 2.0 ** 128) | ((mx < 2.0 ** -128) & (mx > 0.0))
            if ren.any():
                s = np.where(ren, _ilogb(np.where(ren, mx, 1.0)), 0)
                gh, vh, e = np.ldexp(gh, -s), np.ldexp(vh, -s), e + s
            tk = pa * np.ldexp(gh + vh, np.clip(e, -100000, 100000))
            if k == 0:
                tk = tk + pd
            pmf[..., k] = tk
            vh = (vh + w * gh) * rinv
            gh = gh * (float(k) * ainv)
        # closed branch 2
        p0 = pa * (np.exp(-y) + w * (-np.expm1(-y))) + pd
        pmf[tiny] = 0.0
        pmf[..., 0] = np.where(tiny, p0, pmf[..., 0])
    return pmf, pa, mean


def bad_customers(l1):
    lam, mu = l1[..., 0], l1[..., 1]
    with np.errstate(all="ignore"):
        ok = (lam > 0) & (lam < np.inf) & (mu > 0) & (mu < np.inf) & (lam + mu < np.inf)
    return ~ok.all(axis=0)


def stats_from_pmf(pmf, xstar_mean, p_alive, x_star=None):
    """[N][11] statistics (STATS) of the mean pmf [N][K], in the device's order."""
    N, K = pmf.shape
    out = np.full((N, len(STATS)), np.nan)
    for i in range(N):
        xs = -1 if x_star is None else int(x_star[i])
        F, rps, q = 0.0, 0.0, [K, K, K]
        ls = lo = hi = np.nan
        for k in range(K):
            p = pmf[i, k]
            if k == xs:
                lo = F
                with np.errstate(all="ignore"):
                    ls = float(np.log(p))
            F = F + p
            if k == xs:
                hi = F
            for j, lev in enumerate((0.05, 0.5, 0.95)):
                if q[j] == K and F >= lev:
                    q[j] = k
            dev = F - (1.0 if (xs >= 0 and k >= xs) else 0.0)
            rps = rps + dev * dev
        out[i] = (xstar_mean[i], p_alive[i], pmf[i, 0], q[0], q[1], q[2], max(0.0, 1.0 - F), ls, lo, hi,
                  rps if xs >= 0 else np.nan)
    return out


def model(l1, d, t, K, x_star=None):
    """(stats [N][11], mean pmf [N][K]) of level-1 draws l1 [S][N][width] and the data dict d; a
    customer with a draw outside (0, inf): NaN."""
    S, N = l1.shape[:2]
    pmf, pa, mean = draw_pmf(l1[..., 0], l1[..., 1], d["T_cal"] - d["t_x"], float(t), K)
    acc, s_pa, s_mean = np.zeros((N, K)), np.zeros(N), np.zeros(N)
    for s in range(S):          # the device's order: draw by draw
        acc = acc + pmf[s]
        s_pa = s_pa + pa[s]
        s_mean = s_mean + mean[s]
    acc, s_pa, s_mean = acc / float(S), s_pa / float(S), s_mean / float(S)
    out = stats_from_pmf(acc, s_mean, s_pa, x_star)
    bad = bad_customers(l1)
    out[bad] = np.nan
    acc[bad] = np.nan
    return out, acc


# ---- the same in mpmath ---------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath.mp


def mp_p_alive(lam, mu, dT):
    mp = _mp()
    lam, mu, dT = mp.mpf(float(lam)), mp.mpf(float(mu)), mp.mpf(float(dT))
    ml = lam + mu
    E = mp.exp(-ml * dT)
    return ml * E / (mu + lam * E)


def mp_mean(lam, mu, dT, t):
    mp = _mp()
    return mp_p_alive(lam, mu, dT) * (mp.mpf(float(lam)) / mp.mpf(float(mu))) * (-mp.expm1(-mp.mpf(float(mu)) * t))


def mp_pmf_alive_direct(lam, mu, t, k):
    """pmf_alive(k) from the definition, one gammainc per value."""
    mp = _mp()
    lam, mu, t = mp.mpf(float(lam)), mp.mpf(float(mu)), mp.mpf(float(t))
    ml = lam + mu
    y = ml * t
    return (mp.exp(-y + k * mp.log(lam * t) - mp.loggamma(k + 1))
            + (mu / ml) * (lam / ml) ** k * mp.gammainc(k + 1, 0, y, regularized=True))


def mp_pmf_alive(lam, mu, t, K):
    """[K] pmf_alive(0 ... K - 1): P(K, y) from gammainc, then P(k, y) = P(k + 1, y) + pi_k downward
    in 40 digits (mpf has no underflow); mp_pmf_alive_direct checks it (tests/test_forecast_cpu.py)."""
    mp = _mp()
    lam, mu, t = mp.mpf(float(lam)), mp.mpf(float(mu)), mp.mpf(float(t))
    ml = lam + mu
    y, a, w, r = ml * t, lam * t, mu / ml, lam / ml
    P = mp.gammainc(K, 0, y, regularized=True)               # P(K, y) = sum_{j >= K} pi_j
    pi = mp.exp(-y + (K - 1) * mp.log(y) - mp.loggamma(K))   # pi_{K-1}
    rk = r ** (K - 1)
    out = [None] * K
    for k in range(K - 1, -1, -1):
        out[k] = rk * (pi + w * P)                            # g_k = r^k pi_k
        P = P + pi
        pi = pi * k / y
        rk = rk / r
    return out


@functools.lru_cache(maxsize=None)
def mp_draw(lam, mu, dT, t, K):
    """(pmf(d, i, .) [K] mpf, p_alive, mean) of one draw of one customer (cached: the fixtures with
    and without the extreme draws share the rest)."""
    mp = _mp()
    pa = mp_p_alive(lam, mu, dT)
    pmf = [pa * v for v in mp_pmf_alive(lam, mu, t, K)]
    pmf[0] = pmf[0] + (1 - pa)
    return pmf, pa, pa * (mp.mpf(lam) / mp.mpf(mu)) * (-mp.expm1(-mp.mpf(mu) * mp.mpf(t)))


def mp_customer(l1_i, dT, t, K):
    """(mean pmf [K] mpf, xstar_mean, p_alive) of one customer's draws l1_i [S][width]."""
    mp = _mp()
    S = l1_i.shape[0]
    acc, s_pa, s_mean = [mp.mpf(0)] * K, mp.mpf(0), mp.mpf(0)
    for s in range(S):
        pmf, pa, mean = mp_draw(float(l1_i[s, 0]), float(l1_i[s, 1]), float(dT), float(t), int(K))
        acc = [u + v for u, v in zip(acc, pmf)]
        s_pa += pa
        s_mean += mean
    return [v / S for v in acc], s_mean / S, s_pa / S


def mp_stats(pmf, xs):
    """dict of the mpf statistics of one customer's mean pmf (list of mpf); xs < 0: no x_star."""
    mp = _mp()
    K = len(pmf)
    F, rps, q, lo, hi = mp.mpf(0), mp.mpf(0), [K, K, K], None, None
    for k in range(K):
        if k == xs:
            lo = F
        F = F + pmf[k]
        if k == xs:
            hi = F
        for j, lev in enumerate((0.05, 0.5, 0.95)):
            if q[j] == K and F >= mp.mpf(lev):
                q[j] = k
        rps += (F - (1 if (xs >= 0 and k >= xs) else 0)) ** 2
    return dict(p_zero=pmf[0], q05=q[0], q50=q[1], q95=q[2], tail_mass=max(mp.mpf(0), 1 - F),
                log_score=mp.log(pmf[xs]) if xs >= 0 else None, pit_lo=lo, pit_hi=hi, rps=rps if xs >= 0 else None,
                F=F)


def mp_reference(l1, d, t, K, x_star, customers=None):
    """The mpmath statistics rounded to float64: (stats [n][11], mean pmf [n][K], F [n] = the total
    mass below k_max) of the customers given (default: all)."""
    idx = range(l1.shape[1]) if customers is None else customers
    st, pm, Fs = [], [], []
    for i in idx:
        pmf, mean, pa = mp_customer(l1[:, i], d["T_cal"][i] - d["t_x"][i], t, K)
        xs = -1 if x_star is None else int(x_star[i])
        m = mp_stats(pmf, xs)
        nanf = lambda v: float("nan") if v is None else float(v)
        st.append([float(mean), float(pa), float(m["p_zero"]), m["q05"], m["q50"], m["q95"], float(m["tail_mass"]),
                   nanf(m["log_score"]), nanf(m["pit_lo"]), nanf(m["pit_hi"]), nanf(m["rps"])])
        pm.append([float(v) for v in pmf])
        Fs.append(float(m["F"]))
    return np.array(st), np.array(pm), np.array(Fs)


# ---- the GPU tests' case: S = 100, N = 300 ---------------------------------------------------------
GPU_S, GPU_N, GPU_SEED, GPU_T = 100, 300, 21, 39.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forecast_mp_S100_N300.npz")


def gpu_case(width, extremes):
    """(level1, data, x_star) of the GPU tests; lambda and mu do not depend on the width."""
    l1, d = synth_case(GPU_S, GPU_N, width, GPU_SEED, extremes=extremes)
    return l1, d, holdout_counts(GPU_N, GPU_SEED, 64)


def mp_gpu_reference(extremes):
    """{"pmf": [300][128], "stats64", "stats128": [300][11]} of gpu_case in mpmath, rounded to float64
    (the pmf below k_max = 64 is the first half of the rows).  About two minutes."""
    l1, d, xs = gpu_case(4, extremes)
    pm, st = [], {64: [], 128: []}
    nanf = lambda v: float("nan") if v is None else float(v)
    for i in range(GPU_N):
        mp_draw.cache_clear()
        pmf, mean, pa = mp_customer(l1[:, i], d["T_cal"][i] - d["t_x"][i], GPU_T, 128)
        pm.append([float(v) for v in pmf])
        for K in (64, 128):
            m = mp_stats(pmf[:K], int(xs[i]))
            st[K].append([float(mean), float(pa), float(m["p_zero"]), m["q05"], m["q50"], m["q95"],
                          float(m["tail_mass"]), nanf(m["log_score"]), nanf(m["pit_lo"]), nanf(m["pit_hi"]),
                          nanf(m["rps"])])
    return dict(pmf=np.array(pm), stats64=np.array(st[64]), stats128=np.array(st[128]))


def write_golden(path=GOLDEN):
    """Recompute tests/golden/forecast_mp_S100_N300.npz (from the repository root:
    python -c "from tests import forecast_ref as R; R.write_golden()").  tests/test_forecast_cpu.py
    recomputes a sample of its rows and compares."""
    out = {}
    for ext in (0, 1):
        for k, v in mp_gpu_reference(bool(ext)).items():
            out[f"{k}_x{ext}"] = v
    np.savez_compressed(path, **out)


def pmf_tol(K):
    return E_PMF * (K / 64.0 + DEVICE_MARGIN - 1.0)


def stat_tol(K):
    return E_STAT * (K / 64.0 + DEVICE_MARGIN - 1.0)


def mixed_err(got, want):
    """Largest |got - want| / max(|want|, 1) (NaN must match NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    sel = np.isfinite(want)
    if not sel.any():
        return 0.0
    return float(np.max(np.abs(got[sel] - want[sel]) / np.maximum(np.abs(want[sel]), 1.0)))


def rel_err(got, want, floor=0.0):
    """Largest |got - want| / |want| over the entries with |want| >= floor (NaN must match NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    sel = np.isfinite(want) & (np.abs(want) >= floor) & (want != 0.0)
    if not sel.any():
        return 0.0
    return float(np.max(np.abs(got[sel] - want[sel]) / np.abs(want[sel])))

"""Float64 model of the Philox draws of the posterior analysis and the synthetic generator — TEST
INFRASTRUCTURE ONLY, plain numpy, vectorised.

Written from the documented counter layouts of ``csrc/analysis.hip`` / ``csrc/elog.hip`` and from the
reference's equations as ``oracle/analysis_cpu.py`` restates them (tau_star bi:538-540, the lognormal
spend tri:730-738, the weekly activity window analysis_abe.py:456-460) and as
``bivariate/mcmc.py:95-187`` states them for the generator.  Every variate is a pure function of
(seed, counter), so the model predicts every integer exactly and every float to RTOL.

Counters (Philox4x32-10, key = (seed low word, seed high word)):

    predict   (customer, flat draw, slot, 2)   slot 0 + attempt: the Poisson count;
                                               slot 2^20 + j // 2: spend normals of transactions j, j + 1
    track     (week,     flat draw, slot, 3)   slot 0 + attempt: the Poisson count of the summed rate
    generator (customer, 0,         slot, 4)   slot (k - 1) // 2: covariate k (halves (x, y), (z, w));
                                               8: heterogeneity normals; 9: lifetime (x, y);
                                               16 + g // 2: inter-purchase gap g (two per block)

Every decision (a Poisson acceptance, a floor, an event against a time limit) compares two computed
numbers.  The model returns the smallest relative distance by which any decision on a lane's path
was taken (its "margin"); a lane is *clear* when margin > RTOL, and only clear lanes are compared
(teacher forcing and the cap on the set-aside share are those of tests/philox_sweep_ref.py).
"""
from __future__ import annotations

import math

import numpy as np
from scipy.special import gammaln

from oracle import philox as oph
from tests.philox_sweep_ref import BORDERLINE_CAP, RTOL  # noqa: F401  (the project's own figures)

STREAM_PREDICT, STREAM_TRACK, STREAM_GEN = 2, 3, 4
SLOT_SPEND0 = 1 << 20
GEN_SLOT_NORMAL, GEN_SLOT_LIFETIME, GEN_SLOT_GAP0 = 8, 9, 16
POISSON_MAX_ITER = 1 << 16       # the documented bound of the inversion / rejection loops
TRACK_LANES, TRACK_WEEKS = 64, 112

SEED_LO = 7
SEED_HI = (0x1E3779B9 << 32) | 7  # non-zero high key word; below 2^63, so resolve_seed keeps it as is
SEEDS = (SEED_LO, SEED_HI)


# ---------------------------------------------------------------------------------------------
# keys and blocks
# ---------------------------------------------------------------------------------------------
def key(seed):
    s = int(seed) & ((1 << 64) - 1)
    return np.uint32(s & 0xFFFFFFFF), np.uint32(s >> 32)


def _w32(v):
    return (np.asarray(v).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def block(seed, a, d, slot, stream):
    """Philox block of counter (a, d, slot, stream); a, d, slot broadcast.  Returns (..., 4) uint32."""
    a, d, slot = np.broadcast_arrays(_w32(a), _w32(d), _w32(slot))
    ctr = np.empty(a.shape + (4,), np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = a, d, slot, stream
    k0, k1 = key(seed)
    return oph.philox4x32_10(ctr, k0, k1)


# ---------------------------------------------------------------------------------------------
# Poisson
# ---------------------------------------------------------------------------------------------
def _poisson_inversion(m, seed, a, d, slot0, stream):
    """Sequential-search inversion: the smallest k with u <= F(k), F the Poisson CDF summed upwards."""
    r = block(seed, a, d, slot0, stream)
    u = oph.u53(r[:, 0], r[:, 1])
    p = np.exp(-m)
    F = p.copy()
    k = np.zeros(m.shape, np.int64)
    margin = np.full(m.shape, np.inf)
    act = np.arange(m.size)
    for _ in range(POISSON_MAX_ITER):
        margin[act] = np.minimum(margin[act], np.abs(u[act] - F[act]))   # u against F, scale 1
        act = act[u[act] > F[act]]
        if not act.size:
            break
        k[act] += 1
        p[act] = p[act] * m[act] / k[act]    # pmf recurrence P(k) = P(k - 1) m / k
        F[act] += p[act]
    return k, margin


def _poisson_ptrs(m, seed, a, d, slot0, stream):
    """Hoermann (1993), algorithm PTRS: attempt ``it`` takes U from (x, y) and V from (z, w) of block
    slot0 + it."""
    n = m.size
    slam, loglam = np.sqrt(m), np.log(m)
    b = 0.931 + 2.53 * slam
    al = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    out = np.floor(m).astype(np.int64)
    margin = np.full(n, np.inf)
    act = np.arange(n)
    for it in range(POISSON_MAX_ITER):
        if not act.size:
            break
        r = block(seed, a[act], d[act], np.asarray(slot0, dtype=np.int64) + it, stream)
        U = oph.u53(r[:, 0], r[:, 1]) - 0.5
        V = oph.u53(r[:, 2], r[:, 3])
        us = 0.5 - np.abs(U)
        ma, ba, aa = m[act], b[act], al[act]
        with np.errstate(divide="ignore", invalid="ignore"):
            arg = (2.0 * aa / us + ba) * U + ma + 0.43
            scale = np.abs(2.0 * aa / us * U) + np.abs(ba * U) + ma + 0.43
            kf = np.floor(arg)
            mg = np.minimum(arg - kf, kf + 1.0 - arg) / scale           # floor: distance to an integer
            mg = np.minimum(mg, np.abs(us - 0.07))
            wide = us >= 0.07
            mg = np.where(wide, np.minimum(mg, np.abs(V - vr[act])), mg)
            acc1 = wide & (V <= vr[act])
            # not accepted by the squeeze: the cheap rejections, then the log test
            mg2 = np.minimum(mg, np.abs(us - 0.013))
            mg2 = np.where(us < 0.013, np.minimum(mg2, np.abs(V - us)), mg2)
            rej = (kf < 0) | ((us < 0.013) & (V > us))
            lhs_t = (np.log(V), np.log(invalpha[act]), np.log(aa / (us * us) + ba))
            rhs_t = (ma, kf * loglam[act], gammaln(kf + 1.0))
            lhs = lhs_t[0] + lhs_t[1] - lhs_t[2]
            rhs = -rhs_t[0] + rhs_t[1] - rhs_t[2]
            lscale = sum(np.abs(t) for t in lhs_t + rhs_t)
            mg3 = np.minimum(mg2, np.abs(lhs - rhs) / lscale)
            acc2 = ~acc1 & ~rej & (lhs <= rhs)
        mg = np.where(acc1, mg, np.where(rej, mg2, mg3))
        mg = np.where(np.isfinite(mg), mg, 0.0)
        margin[act] = np.minimum(margin[act], mg)
        done = acc1 | acc2
        out[act[done]] = kf[done].astype(np.int64)
        act = act[~done]
    return out, margin


def poisson(m, seed, a, d, slot0=0, stream=STREAM_PREDICT):
    """Poisson(m) of counter (a, d, slot0 + attempt, stream).  Returns (k int64, margin): 0 for m <= 0
    or NaN; inversion for m < 10; PTRS from 10.  m, a, d broadcast."""
    m, a, d = np.broadcast_arrays(np.asarray(m, dtype=np.float64), np.asarray(a), np.asarray(d))
    shape = m.shape
    m, a, d = m.ravel(), a.ravel(), d.ravel()
    k = np.zeros(m.size, np.int64)
    margin = np.full(m.size, np.inf)
    with np.errstate(invalid="ignore"):
        small = np.flatnonzero((m > 0.0) & (m < 10.0))
        big = np.flatnonzero(m >= 10.0)
    if small.size:
        k[small], margin[small] = _poisson_inversion(m[small], seed, a[small], d[small], slot0, stream)
    if big.size:
        k[big], margin[big] = _poisson_ptrs(m[big], seed, a[big], d[big], slot0, stream)
    return k.reshape(shape), margin.reshape(shape)


# ---------------------------------------------------------------------------------------------
# posterior predictive
# ---------------------------------------------------------------------------------------------
def tau_star(level1, T_cal, T_star):
    """bi:538-540 / tri:717-722: T_star if alive else clip(tau - T_cal, 0, T_star)."""
    tau, alive = level1[..., 2], level1[..., 3] > 0.5
    return np.where(alive, float(T_star), np.clip(tau - np.asarray(T_cal, dtype=np.float64), 0.0, float(T_star)))


def spend_normals(seed, a, d, jb, stream=STREAM_PREDICT, slot0=SLOT_SPEND0):
    """Box-Muller pair of block slot0 + jb: (cos, sin) -> transactions 2 jb, 2 jb + 1."""
    r = block(seed, a, d, np.asarray(jb, dtype=np.int64) + slot0, stream)
    rad = np.sqrt(-2.0 * np.log(oph.u53_open0(r[..., 0], r[..., 1])))
    ang = 2.0 * np.pi * oph.u53(r[..., 2], r[..., 3])
    return rad * np.cos(ang), rad * np.sin(ang)


def predict(level1, T_cal, T_star, seed, simulate_spend=False, sigma_s=0.5, *, swap_counter=False,
            stream=STREAM_PREDICT, spend_slot0=SLOT_SPEND0):
    """x ~ Poisson(lambda tau_star) per (draw, customer) and, with ``simulate_spend``, the total of x
    lognormal(eta, sigma_s) spends summed in transaction order (tri:730-738).  level1: (n_draws, n,
    4 or 5).  ``swap_counter`` / ``stream`` / ``spend_slot0`` are the power checks' wrong layouts."""
    level1 = np.asarray(level1, dtype=np.float64)
    nd, n, _ = level1.shape
    ts = tau_star(level1, T_cal, T_star)
    m = level1[..., 0] * ts
    cust, draw = np.broadcast_arrays(np.arange(n)[None, :], np.arange(nd)[:, None])
    a, d = (draw, cust) if swap_counter else (cust, draw)
    x, margin = poisson(m, seed, a, d, 0, stream)
    out = dict(x=x, margin=margin, tau_star=ts, mean=m)
    if simulate_spend:
        eta = level1[..., 4]
        tot = np.zeros((nd, n))
        for jb in range(int((x.max() + 1) // 2)):
            on = x > 2 * jb
            n0, n1 = spend_normals(seed, a[on], d[on], jb, stream, spend_slot0)
            tot[on] += np.exp(eta[on] + sigma_s * n0)
            second = x[on] > 2 * jb + 1
            idx = tuple(ix[second] for ix in np.nonzero(on))
            tot[idx] += np.exp(eta[idx] + sigma_s * n1[second])
        out["spend"] = tot
    return out


# ---------------------------------------------------------------------------------------------
# weekly tracking
# ---------------------------------------------------------------------------------------------
def track_n_adds(n, n_times):
    """Additions behind one week's fixed-order rate, at most: every customer's +lam and -lam of the
    pass (2 n), then 64 lane additions and one running-sum addition for each of the pass's columns up
    to that week.  Each partial sum is a sum of rates of customers active in one week, so at most the
    peak rate: the rounding error is within n_adds * eps * peak."""
    return 2 * n + (TRACK_LANES + 1) * min(TRACK_WEEKS, n_times)


def track_rates(level1, birth, times, *, birth_inclusive=False):
    """The summed active rate per (draw, week) in the documented fixed order: weeks in passes of 112;
    customer i belongs to lane i mod 64, visited in ascending i; each lane adds +lam at the first week
    of the pass with t > b and -lam at the first with t > b + tau; columns are summed over lanes 0..63,
    then a running sum over the pass's weeks, clamped at 0."""
    level1 = np.asarray(level1, dtype=np.float64)
    nd, n, _ = level1.shape
    lam, tau = level1[..., 0], level1[..., 2]
    birth = np.asarray(birth, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    nt = times.size
    end = birth[None, :] + tau
    rate = np.zeros((nd, nt))
    for w0 in range(0, nt, TRACK_WEEKS):
        tw = times[w0:w0 + TRACK_WEEKS]
        nw = tw.size
        jl = np.broadcast_to(np.searchsorted(tw, birth, side="left" if birth_inclusive else "right"), (nd, n))
        jh = np.maximum(np.searchsorted(tw, end.ravel(), side="right").reshape(nd, n), jl)
        diff = np.zeros((nd, TRACK_LANES, nw + 1))
        for r0 in range(0, n, TRACK_LANES):          # one customer per lane and round: ascending i
            i = np.arange(r0, min(r0 + TRACK_LANES, n))
            on = jl[:, i] < jh[:, i]
            dd, ll = np.nonzero(on)
            diff[dd, ll, jl[dd, i[ll]]] += lam[dd, i[ll]]
            diff[dd, ll, jh[dd, i[ll]]] -= lam[dd, i[ll]]
        col = np.zeros((nd, nw + 1))
        for q in range(TRACK_LANES):
            col += diff[:, q, :]
        run = np.add.accumulate(col[:, :nw], axis=1)
        rate[:, w0:w0 + nw] = np.where(run > 0.0, run, 0.0)
    return rate


def track_exact_rates(level1, birth, times):
    """math.fsum of lambda over the customers with b < t <= b + tau (analysis_abe.py:456-460)."""
    level1 = np.asarray(level1, dtype=np.float64)
    nd = level1.shape[0]
    birth = np.asarray(birth, dtype=np.float64)
    out = np.zeros((nd, len(times)))
    for d in range(nd):
        lam, end = level1[d, :, 0], birth + level1[d, :, 2]
        for j, t in enumerate(times):
            out[d, j] = math.fsum(lam[(t > birth) & (t <= end)])
    return out


def track(level1, birth, times, seed, *, pass_relative_week=False, birth_inclusive=False):
    """One Poisson of the summed rate per (draw, week): counter (week, flat draw, attempt, 3).
    Returns dict(inc (n_draws, n_times) int64, margin, rate, inc_sum, inc_mean)."""
    rate = track_rates(level1, birth, times, birth_inclusive=birth_inclusive)
    nd, nt = rate.shape
    week = np.arange(nt)
    if pass_relative_week:
        week = week % TRACK_WEEKS
    inc, margin = poisson(rate, seed, week[None, :], np.arange(nd)[:, None], 0, STREAM_TRACK)
    inc_sum = np.add.accumulate(inc.astype(np.float64), axis=0)[-1]   # sequential over draws
    return dict(inc=inc, margin=margin, rate=rate, inc_sum=inc_sum, inc_mean=inc_sum / nd)


# ---------------------------------------------------------------------------------------------
# synthetic generator (bi:95-187)
# ---------------------------------------------------------------------------------------------
def gen_covariates(n, K, seed):
    """[1, U(-1, 1) ...] (bi:119-122): covariate k from slot (k - 1) // 2, half (k - 1) % 2."""
    cov = np.ones((n, K))
    cust = np.arange(n)
    for k in range(1, K):
        r = block(seed, cust, 0, (k - 1) // 2, STREAM_GEN)
        h = 2 * ((k - 1) % 2)
        cov[:, k] = -1.0 + 2.0 * oph.u53(r[:, h], r[:, h + 1])
    return cov


def gen_mvn(n, gamma, seed):
    """MVN(0, gamma) per customer: slot 8's Box-Muller pair (cos first, sin second) through the lower
    Cholesky factor of gamma."""
    r = block(seed, np.arange(n), 0, GEN_SLOT_NORMAL, STREAM_GEN)
    rad = np.sqrt(-2.0 * np.log(oph.u53_open0(r[:, 0], r[:, 1])))
    ang = 2.0 * np.pi * oph.u53(r[:, 2], r[:, 3])
    z = np.column_stack([rad * np.cos(ang), rad * np.sin(ang)])
    return z @ np.linalg.cholesky(np.asarray(gamma, dtype=np.float64)).T


def gen_lifetime_exp(n, seed, half=0):
    """Standard exponential of slot 9, (x, y) (``half=1``: (z, w), a power check's wrong layout)."""
    r = block(seed, np.arange(n), 0, GEN_SLOT_LIFETIME, STREAM_GEN)
    return -np.log(oph.u53_open0(r[:, 2 * half], r[:, 2 * half + 1]))


def gen_gap_exps(cust, seed, g0, count, gap_slot0=GEN_SLOT_GAP0):
    """Standard exponentials of gaps g0 .. g0 + count - 1 (g0, count even) of the given customers."""
    slots = gap_slot0 + g0 // 2 + np.arange(count // 2)
    r = block(seed, np.asarray(cust)[:, None], 0, slots[None, :], STREAM_GEN)
    e = np.stack([-np.log(oph.u53_open0(r[..., 0], r[..., 1])), -np.log(oph.u53_open0(r[..., 2], r[..., 3]))], axis=-1)
    return e.reshape(len(cust), count)


def gen_covars_arg(n, K, covars):
    """bi:123-130: a supplied matrix gets the ones column when it lacks it."""
    cov = np.asarray(covars, dtype=np.float64)
    if cov.ndim == 1:
        cov = cov[:, None]
    if not np.allclose(cov[:, 0], 1):
        cov = np.column_stack([np.ones(cov.shape[0]), cov])
    assert cov.shape == (n, K)
    return cov


def gen_params(n, beta, gamma, seed, covars=None, lifetime_half=0):
    """bi:117-137: covariates, theta = exp(X beta + MVN(0, gamma)), tau ~ Exp(mu)."""
    beta = np.asarray(beta, dtype=np.float64)
    K = beta.shape[0]
    cov = gen_covariates(n, K, seed) if covars is None else gen_covars_arg(n, K, covars)
    theta = np.exp(cov @ beta + gen_mvn(n, gamma, seed))
    lam, mu = theta[:, 0], theta[:, 1]
    return dict(cov=cov, lam=lam, mu=mu, tau=gen_lifetime_exp(n, seed, lifetime_half) / mu)


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / (np.abs(a) + np.abs(b))
    return np.where(np.isnan(r), 0.0, r)


def gen_events(lam, tau, T_cal, T_star, seed, *, gap_slot0=GEN_SLOT_GAP0, chunk=64):
    """The event loop of bi:150-162 from given (lam, tau) — teacher forcing — with the CBS rules
    bi:83-87, alive_true bi:169 and the hold-out counts bi:172-181.  Returns dict(x, t_x, alive, x_star
    (n_star, n), n_events, elog_cust, elog_t, margin); margin is the smallest relative distance of any
    compared time from its limit (the t = 0 event is exact on both sides and carries none)."""
    lam, tau = np.asarray(lam, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    n = lam.size
    T_cal = np.broadcast_to(np.asarray(T_cal, dtype=np.float64).ravel(), (n,)) if np.size(T_cal) == 1 \
        else np.asarray(T_cal, dtype=np.float64).ravel()
    T_star = np.asarray(T_star, dtype=np.float64).ravel()
    T_fix, Ts_max = T_cal.max(), T_star.max()
    T_zero = T_fix - T_cal
    min_T = np.minimum(T_cal + Ts_max, tau)
    t_end = T_fix + Ts_max
    x = np.zeros(n, np.int64)
    t_x = np.zeros(n)
    x_star = np.zeros((T_star.size, n), np.int64)
    n_events = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    rows_c, rows_t = [], []
    for i0 in range(0, n, 256):
        cust = np.arange(i0, min(i0 + 256, n))
        t = np.zeros((cust.size, 1))                                   # ts = [0.0]
        while (t[:, -1] < min_T[cust]).any():
            gaps = gen_gap_exps(cust, seed, t.shape[1] - 1, chunk, gap_slot0) / lam[cust, None]
            ext = np.add.accumulate(np.concatenate([t[:, -1:], gaps], axis=1), axis=1)   # t_acc += dt, in order
            t = np.concatenate([t, ext[:, 1:]], axis=1)
        lim = min_T[cust, None]
        gen = np.ones(t.shape, bool)
        gen[:, 1:] = t[:, :-1] < lim                                   # appended while t_acc < min_T
        tl, Tz = tau[cust, None], T_zero[cust, None]
        ta = t + Tz
        keep_tau = gen & (t <= tl)                                     # ts[ts <= tau] + T_zero
        keep = keep_tau & (ta <= t_end)
        cal = keep & (ta <= T_fix)
        later = gen.copy()
        later[:, 0] = False
        mg = np.where(later, np.minimum(_rel(t, tl), _rel(t, lim)), np.inf)
        mg = np.minimum(mg, np.where(later & keep_tau, _rel(ta, t_end), np.inf))
        thr = np.where(later & keep, _rel(ta, T_fix), np.inf)
        for k in range(T_star.size):
            x_star[k, cust] = (keep & ~cal & (ta <= T_fix + T_star[k])).sum(axis=1)
            thr = np.minimum(thr, np.where(later & keep, _rel(ta, T_fix + T_star[k]), np.inf))
        margin[cust] = np.minimum(mg, thr).min(axis=1)
        x[cust] = np.clip(cal.sum(axis=1) - 1, 0, None)
        t_x[cust] = np.where(cal, ta, -np.inf).max(axis=1)
        n_events[cust] = keep.sum(axis=1)
        rr, cc = np.nonzero(keep)                                      # row-major: customer, then time order
        rows_c.append(cust[rr] + 1.0)
        rows_t.append(ta[rr, cc])
    return dict(x=x, t_x=t_x, alive=(T_zero + tau) > T_fix, x_star=x_star, n_events=n_events,
                elog_cust=np.concatenate(rows_c), elog_t=np.concatenate(rows_t), margin=margin)


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_analysis_stream.py (the CPU module asserts the borderline cap of the
# model alone on exactly these inputs)
# ---------------------------------------------------------------------------------------------
P1_MEANS = (0.0, 0.3, 9.99, float(np.nextafter(10.0, 0.0)), 10.0, 37.5, 600.0, 1e5)
P1_T_STAR = 32.0   # tau_star is 32, 16 or 0: a power of two, so lambda = mean / tau_star hits the mean exactly


def predict_case_p1():
    """n = 257 (a full workgroup plus one lane), 3 draws, width 4.  Per lane: a target mean of
    P1_MEANS and one of four tau_star modes — 0 alive, 1 dead with tau < T_cal (mean 0), 2 dead with
    0 < tau - T_cal = 16 < T_star, 3 dead with tau - T_cal > T_star; z in {0, 0.5, 0.75, 1}."""
    n, nd = 257, 3
    i, d = np.meshgrid(np.arange(n), np.arange(nd))
    target = np.array(P1_MEANS)[(i + d) % 8]
    mode = (i // 8 + d) % 4
    T_cal = 30.0 + (np.arange(n) % 5)
    l1 = np.zeros((nd, n, 4))
    l1[..., 0] = target / np.where(mode == 2, 16.0, P1_T_STAR)
    l1[..., 1] = 0.02
    l1[..., 2] = np.select([mode == 0, mode == 1, mode == 2], [5.0, T_cal[None, :] - 3.0, T_cal[None, :] + 16.0],
                           T_cal[None, :] + 100.0)
    l1[..., 3] = np.where(mode == 0, np.where(i % 2 == 0, 0.75, 1.0), np.where(i % 2 == 0, 0.5, 0.0))
    return dict(level1=l1, T_cal=T_cal, T_star=P1_T_STAR, target=target, mode=mode)


P2_MEANS = (0.0, 0.7, 1.5, 2.5, 3.0, 600.0)


def predict_case_p2():
    """Width 5 with spend: n = 200, 2 draws, all alive, means P2_MEANS (counts 0, 1, 2, 3, ... and about
    600), eta spread over [-2, 3]."""
    n, nd = 200, 2
    i, d = np.meshgrid(np.arange(n), np.arange(nd))
    l1 = np.zeros((nd, n, 5))
    l1[..., 0] = np.array(P2_MEANS)[(i + 2 * d) % 6] / 39.0
    l1[..., 1] = 0.02
    l1[..., 2] = 50.0
    l1[..., 3] = 1.0
    l1[..., 4] = -2.0 + 5.0 * ((i * 37 + d * 11) % 200) / 199.0
    return dict(level1=l1, T_cal=np.full(n, 30.0), T_star=39.0)


P3_MEANS = (0.3, 4.0, 9.99, 12.0, 37.5, 600.0)


def predict_case_p3():
    """n = 1, 65,537 draws: one more than a grid's y extent, so the last draw is reached by the stride."""
    nd = 65537
    l1 = np.zeros((nd, 1, 4))
    l1[:, 0, 0] = np.array(P3_MEANS)[np.arange(nd) % 6] / 39.0
    l1[:, 0, 1] = 0.02
    l1[:, 0, 2] = 50.0
    l1[:, 0, 3] = 1.0
    return dict(level1=l1, T_cal=np.full(1, 30.0), T_star=39.0)


def _l1_track(lam, tau):
    l1 = np.zeros(lam.shape + (4,))
    l1[..., 0], l1[..., 1], l1[..., 2], l1[..., 3] = lam, 0.02, tau, 1.0
    return l1


def track_case_t1():
    """1 draw, n = 130, weeks 1..78.  Births and lifetimes on the integers (two in three births equal
    a week exactly; three in four b + tau do, exactly representable), births from before week 1 to
    after week 78."""
    rng = np.random.default_rng(101)
    n = 130
    b = rng.integers(-3, 83, n).astype(np.float64)
    b[::3] += 0.5
    tau = rng.integers(0, 40, n).astype(np.float64)
    tau[::4] += 0.25
    lam = np.exp(rng.normal(-0.5, 1.0, n))
    return dict(level1=_l1_track(lam[None, :], tau[None, :]), birth=b, times=np.arange(1.0, 79.0))


def track_case_t2(n_times):
    """n_times = 113 / 225 (two / three passes of 112 weeks), 5 draws, n = 150: times, births and
    lifetimes on a grid of 0.5, so neighbouring times tie and births / ends meet times exactly; long
    lifetimes keep customers active across the pass boundaries."""
    rng = np.random.default_rng(200 + n_times)
    n, nd = 150, 5
    times = np.sort(np.round(rng.uniform(0.0, 100.0, n_times) * 2.0) / 2.0)
    b = np.round(rng.uniform(-5.0, 105.0, n) * 2.0) / 2.0
    tau = np.round(rng.exponential(40.0, (nd, n)) * 2.0) / 2.0
    lam = np.exp(rng.normal(-2.0, 1.0, (nd, n)))
    return dict(level1=_l1_track(lam, tau), birth=b, times=times)


def track_case_t3():
    """n = 1000, 2 draws, weeks 1..78: everybody is born in weeks 10..19 and gone by week 50, so the
    summed rate climbs to ~9e4 (PTRS) and falls back to weeks whose exact rate is 0."""
    rng = np.random.default_rng(303)
    n, nd = 1000, 2
    b = rng.uniform(10.0, 20.0, n)
    tau = rng.uniform(1.0, 30.0, (nd, n))
    lam = rng.uniform(40.0, 140.0, (nd, n))
    return dict(level1=_l1_track(lam, tau), birth=b, times=np.arange(1.0, 79.0))


GEN_GAMMA = np.array([[0.6, 0.1], [0.1, 0.9]])
GEN_GAMMA_TIGHT = np.array([[0.01, 0.002], [0.002, 0.02]])


def gen_cases():
    """name -> arguments of generate_pareto_abe (n, T_cal, T_star, beta, gamma, covars)."""
    rng = np.random.default_rng(404)
    b3 = np.array([[-1.2, -2.5], [0.3, -0.2], [-0.2, 0.4]])
    b6 = np.array([[-1.0, -2.8], [0.4, 0.1], [-0.3, 0.5], [0.2, -0.1], [-0.15, 0.25], [0.1, 0.3]])
    cov = rng.uniform(-1.0, 1.0, size=(200, 2))
    return {
        "G1": dict(n=300, T_cal=32.0, T_star=[20.0, 32.0], beta=b3, gamma=GEN_GAMMA, covars=None),
        "G2": dict(n=300, T_cal=rng.choice([8.0, 20.5, 32.0], size=300), T_star=[32.0, 0.0, 5.5, 20.0, 1.0, 64.0, 13.0, 26.0],
                   beta=b6, gamma=GEN_GAMMA, covars=None),
        "G3_supplied": dict(n=200, T_cal=32.0, T_star=[32.0], beta=b3, gamma=GEN_GAMMA, covars=cov),
        "G3_supplied_ones": dict(n=200, T_cal=32.0, T_star=[32.0], beta=b3, gamma=GEN_GAMMA,
                                 covars=np.column_stack([np.ones(200), cov])),
        "G3_k1": dict(n=200, T_cal=32.0, T_star=[32.0], beta=np.array([[-0.5, -3.0]]), gamma=GEN_GAMMA, covars=None),
        "G4_busy": dict(n=64, T_cal=52.0, T_star=[52.0], beta=np.array([[math.log(50.0), -5.5]]), gamma=GEN_GAMMA_TIGHT,
                        covars=None),
        "G4_dead": dict(n=64, T_cal=52.0, T_star=[52.0], beta=np.array([[math.log(50.0), math.log(1e6)]]),
                        gamma=GEN_GAMMA_TIGHT, covars=None),
    }

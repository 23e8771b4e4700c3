"""float64 model of csrc/ic.hip (pointwise log-likelihood, WAIC, PSIS-LOO per customer), the same
definitions in 40-digit mpmath, and the inputs the tests share.

The model follows include/clvmcmc.h's definitions with numpy's vectorised functions; its sums are
numpy's, not the device's, so the device is compared with a tolerance (tests/test_ic_cpu.py measures
the model's own error against mpmath: E_L and E_STAT there).  The mpmath functions take the same
float64 inputs as exact numbers, so every decision (the tail's members, a dropped weight) is the
model's."""
import math

import numpy as np

STATS = ("lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "pareto_k", "tail_len")
EPS = float(np.finfo(np.float64).eps)
LOG_TINY = float(np.log(np.finfo(np.float64).tiny))
MIN_FIT = 5
ULP = 2.0 ** -52
# The model's largest deviation from mpmath ON THE 64 x 100 FIXTURES of tests/test_ic_cpu.py, which
# measures and asserts them (its header says how): relative for the pointwise log-likelihood;
# relative for lppd, p_waic and elpd_loo and absolute for pareto_k.  They are the unit of the GPU
# tolerances, not a bound on the model elsewhere: on the larger matrices of tests/test_gpu_ic.py the
# model's own pareto_k deviates from mpmath by up to 1.9 E_STAT, so the device is held to mpmath there,
# not to the model.
E_L = 7e-16
E_STAT = 8e-16


# ---- inputs ---------------------------------------------------------------------------------------
def synth_case(S, N, width, seed, extremes=False):
    """(level1 [S][N][width], data dict x int32 / t_x / T_cal / log_s) of N customers.  Customer 0
    never bought (x = 0, t_x = 0), customer 1 bought last at T_cal.  extremes: draws 0 .. 5 carry
    log lambda = +-70 and mu = e^5 (where lambda exp(-(lambda + mu)(T_cal - t_x)) underflows) in
    turn over the customers."""
    g = np.random.default_rng(seed)
    x = g.poisson(2.0, N).astype(np.int32)
    T_cal = g.uniform(27.0, 39.0, N)
    t_x = np.where(x > 0, g.uniform(0.0, 1.0, N) * T_cal, 0.0)
    x[0], t_x[0] = 0, 0.0
    if N > 1:
        x[1], t_x[1] = 5, T_cal[1]
    log_s = g.normal(3.5, 0.6, N)
    base_lam = np.exp(g.normal(-2.5, 0.8, N))
    base_mu = np.exp(g.normal(-3.5, 0.8, N))
    l1 = np.empty((S, N, width))
    l1[..., 0] = base_lam * np.exp(g.normal(0.0, 0.25, (S, N)))
    l1[..., 1] = base_mu * np.exp(g.normal(0.0, 0.35, (S, N)))
    l1[..., 2] = g.exponential(30.0, (S, N))
    l1[..., 3] = (g.random((S, N)) < 0.6).astype(np.float64)
    if width == 5:
        l1[..., 4] = np.exp(log_s + g.normal(0.0, 0.15, (S, N)))
    if extremes:
        i = np.arange(N)
        l1[0, i % 3 == 0, 0] = np.exp(70.0)
        l1[1, i % 3 == 1, 0] = np.exp(-70.0)
        l1[2, i % 3 == 2, 1] = np.exp(5.0)
        l1[3, i % 2 == 0, 0], l1[3, i % 2 == 0, 1] = np.exp(-70.0), np.exp(5.0)
        l1[4, i % 2 == 1, 0], l1[4, i % 2 == 1, 1] = np.exp(70.0), np.exp(-70.0)
        l1[5, :, 1] = np.exp(-70.0)
    return l1, dict(x=x, t_x=t_x, T_cal=T_cal, log_s=log_s)


TIED, CONST, DOMINANT = 3, 4, 5


def planted_matrix(S, N, seed):
    """[S][N] log-likelihood matrix (the spend term included) of synth_case's moderate customers with
    three planted series: TIED has ties straddling the PSIS cutoff (two tail values fall out), CONST
    is constant, DOMINANT has one draw whose importance ratio is e^8 times the next (pareto_k > 0.7)."""
    l1, d = synth_case(S, N, 5, seed)
    ll = loglik(l1, d, True, 0.37)
    g = np.random.default_rng(seed + 1)
    M = tail_max(S)
    srt = np.sort(ll[:, TIED])
    srt[max(M - 2, 0):M + 3] = srt[M]
    ll[:, TIED] = g.permutation(srt)
    ll[:, CONST] = -4.75
    ll[g.integers(S), DOMINANT] = ll[:, DOMINANT].min() - 8.0
    return ll


def gpd_series(k, S=4000, seed=1):
    """A log-likelihood series whose importance ratios exp(-l) are S generalised-Pareto(k, sigma = 1)
    draws."""
    u = np.random.default_rng(seed).random(S)
    return -np.log(np.expm1(-k * np.log1p(-u)) / k)


# ---- the float64 model ----------------------------------------------------------------------------
def loglik(l1, d, spend=False, omega2=None):
    """[S][N] pointwise log-likelihood, the operations in the device's order."""
    lam, mu = l1[..., 0], l1[..., 1]
    x, t_x = d["x"].astype(np.float64), d["t_x"]
    dT = d["T_cal"] - t_x
    ml = lam + mu
    with np.errstate(all="ignore"):
        l = ((x * np.log(lam) - np.log(ml)) - ml * t_x) + np.log(mu + lam * np.exp(-(ml * dT)))
        if spend:
            c = -0.5 * np.log(2.0 * np.pi * omega2)
            dev = d["log_s"] - np.log(l1[..., 4])
            l = l + (c - (dev * dev) / (2.0 * omega2))
    return l


def loglik_scale(l1, d, spend=False, omega2=None):
    """[S][N] the largest magnitude among the terms loglik adds: where they cancel, an evaluation in
    float64 is good to a few ulp of this, not of the sum."""
    lam, mu = l1[..., 0], l1[..., 1]
    x, t_x = d["x"].astype(np.float64), d["t_x"]
    ml = lam + mu
    with np.errstate(all="ignore"):
        terms = [x * np.log(lam), np.log(ml), ml * t_x, np.log(mu + lam * np.exp(-(ml * (d["T_cal"] - t_x))))]
        if spend:
            dev = d["log_s"] - np.log(l1[..., 4])
            terms += [np.full(lam.shape, -0.5 * np.log(2.0 * np.pi * omega2)), (dev * dev) / (2.0 * omega2)]
    return np.max(np.abs(np.stack(terms)), axis=0)


def tail_max(S, reff=1.0):
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / reff))))


def logsumexp(v):
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def gpdfit(t):
    """Zhang & Stephens' estimator on the ascending tail t as ArviZ's _gpdfit: (khat, sigma)."""
    n = len(t)
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1)
    c = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * t[int(math.floor(n / 4.0 + 0.5)) - 1])
    b = c + 1.0 / t[-1]
    u = (t[-1] - t) / t[-1]

    def mean_log(bj, cj):
        """mean(log1p(-b t)) with b = c + 1 / t_n; where b t_i nears 1 the argument 1 - b t_i is formed
        as (t_n - t_i) / t_n - c t_i, two terms of one sign, not as a difference of near-equal numbers."""
        bt = bj * t
        return math.fsum(np.where(bt < 0.5, np.log1p(-np.minimum(bt, 0.5)), np.log(u - cj * t))) / n
    k = np.array([mean_log(bj, cj) for bj, cj in zip(b, c)])      # the n-term sums rounded once
    L = n * ((np.log(-(b / k)) - k) - 1.0)
    w = 1.0 / np.array([math.fsum(np.exp(L - Lj)) for Lj in L])
    w = np.where(w < 10.0 * EPS, 0.0, w)        # a NaN weight is not below: it stays and ends in khat
    w = w / math.fsum(w)
    bhat, chat = math.fsum(b * w), math.fsum(c * w)
    k = mean_log(bhat, chat)
    return (n * k + 5.0) / (n + 10.0), -(k / bhat)


def psis_one(l, reff=1.0):
    """One customer's series: (elpd_loo, khat, tail_len, normalised log weights in the order of
    ascending l)."""
    S = len(l)
    a = np.sort(l)
    x = a[0] - a                                  # (-l) - max(-l), exactly
    M = tail_max(S, reff)
    cutoff = max(x[M], LOG_TINY)
    n = int((x > cutoff).sum())
    khat, lw = np.inf, x.copy()
    if n >= MIN_FIT:
        with np.errstate(all="ignore"):
            ec = np.exp(cutoff)
            # exp(x) - exp(cutoff) = exp(cutoff) expm1(x - cutoff) without its cancellation, and
            # x - cutoff = l_(M) - l from the values themselves, one rounding, where the cutoff is x_(M)
            xc = a[M] - a[:n] if cutoff == x[M] else x[:n] - cutoff
            t = (ec * np.expm1(xc))[::-1]
            kh, sigma = gpdfit(t)
            if np.isfinite(kh):
                khat = kh
                lp = np.log1p(-((np.arange(1, n + 1) - 0.5) / n))
                g = -(sigma * lp) if abs(kh) < EPS else (sigma * np.expm1(-(kh * lp))) / kh
                lw[:n] = np.fmin(np.log(g + ec), 0.0)[::-1]
    logw = lw - logsumexp(lw)
    return logsumexp(logw + a), khat, n, logw


def model(ll, reff=1.0):
    """[N][7] statistics (STATS) of the matrix ll [S][N]; a customer with a non-finite value: NaN."""
    S, N = ll.shape
    out = np.full((N, len(STATS)), np.nan)
    for i in range(N):
        l = ll[:, i]
        if not np.isfinite(l).all():
            continue
        lppd = logsumexp(l) - np.log(S)
        pw = l.var()
        elpd, khat, n, _ = psis_one(l, reff)
        out[i] = (lppd, pw, lppd - pw, elpd, lppd - elpd, khat, n)
    return out


def bad_k_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def totals(col):
    """(sum, se = sqrt(N var(ddof 0))) of a per-customer column, numpy's sums."""
    col = np.asarray(col, np.float64)
    return col.sum(), math.sqrt(len(col) * col.var())


# ---- the same in mpmath ---------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath.mp


def mp_loglik(lam, mu, eta, x, t_x, T_cal, log_s=None, omega2=None):
    mp = _mp()
    lam, mu, t_x, T_cal = mp.mpf(float(lam)), mp.mpf(float(mu)), mp.mpf(float(t_x)), mp.mpf(float(T_cal))
    ml = lam + mu
    l = int(x) * mp.log(lam) - mp.log(ml) - ml * t_x + mp.log(mu + lam * mp.exp(-ml * (T_cal - t_x)))
    if log_s is not None:
        w2 = mp.mpf(float(omega2))
        d = mp.mpf(float(log_s)) - mp.log(mp.mpf(float(eta)))
        l += -mp.log(2 * mp.pi * w2) / 2 - d * d / (2 * w2)
    return l


def mp_loglik_matrix(l1, d, spend=False, omega2=None):
    """[S][N] object array of mpf."""
    S, N, w = l1.shape
    out = np.empty((S, N), object)
    for s in range(S):
        for i in range(N):
            out[s, i] = mp_loglik(l1[s, i, 0], l1[s, i, 1], l1[s, i, 4] if w == 5 else 1.0, d["x"][i], d["t_x"][i],
                                  d["T_cal"][i], d["log_s"][i] if spend else None, omega2)
    return out


def _mp_lse(v):
    mp = _mp()
    m = max(v)
    return m + mp.log(mp.fsum(mp.exp(e - m) for e in v))


def mp_stats(l, reff=1.0):
    """dict lppd, p_waic, elpd_loo, pareto_k (mpf; pareto_k inf where not fitted), tail_len of one
    float64 series."""
    mp = _mp()
    S = len(l)
    a = [mp.mpf(float(v)) for v in np.sort(l)]
    lppd = _mp_lse(a) - mp.log(S)
    mean = mp.fsum(a) / S
    pw = mp.fsum((v - mean) ** 2 for v in a) / S
    x = [a[0] - v for v in a]
    cutoff = max(x[tail_max(S, reff)], mp.mpf(LOG_TINY))
    n = sum(1 for v in x if v > cutoff)
    khat, lw = mp.inf, list(x)
    if n >= MIN_FIT:
        ec = mp.exp(cutoff)
        t = [mp.exp(v) - ec for v in x[:n]][::-1]
        m = 30 + int(math.floor(math.sqrt(n)))
        tq, tn = t[int(math.floor(n / 4.0 + 0.5)) - 1], t[-1]
        b = [(1 - mp.sqrt(mp.mpf(m) / (j - mp.mpf(0.5)))) / (3 * tq) + 1 / tn for j in range(1, m + 1)]
        k = [mp.fsum(mp.log1p(-bj * ti) for ti in t) / n for bj in b]
        L = [n * (mp.log(-bj / kj) - kj - 1) for bj, kj in zip(b, k)]
        Lm = max(L)
        E = [mp.exp(v - Lm) for v in L]
        Es = mp.fsum(E)
        w = [e / Es for e in E]                   # = 1 / sum_i exp(L_i - L_j)
        w = [mp.mpf(0) if v < 10 * EPS else v for v in w]
        ws = mp.fsum(w)
        bhat = mp.fsum(bj * wj / ws for bj, wj in zip(b, w))
        kk = mp.fsum(mp.log1p(-bhat * ti) for ti in t) / n
        sigma = -kk / bhat
        khat = (n * kk + 5) / (n + 10)
        for q in range(1, n + 1):
            lp = mp.log1p(-(mp.mpf(q) - mp.mpf(0.5)) / n)
            g = -sigma * lp if abs(khat) < EPS else sigma * mp.expm1(-khat * lp) / khat
            lw[n - q] = min(mp.log(g + ec), mp.mpf(0))
    lse = _mp_lse(lw)
    elpd = _mp_lse([u - lse + v for u, v in zip(lw, a)])
    return dict(lppd=lppd, p_waic=pw, elpd_loo=elpd, pareto_k=khat, tail_len=n)


def rel_dev(got, want):
    """|got - want| / |want| of a float64 against an mpf."""
    mp = _mp()
    want = mp.mpf(want)
    return float(abs(mp.mpf(float(got)) - want) / abs(want))


def abs_dev(got, want):
    mp = _mp()
    return float(abs(mp.mpf(float(got)) - mp.mpf(want)))

"""Float64 model of scoring customers outside the fit (csrc/score.hip) — TEST INFRASTRUCTURE ONLY, plain
numpy.  Built from the pieces the production sweep is held to: ``sweep_level1``, ``l2_unpack`` and
``oracle_variates`` of tests/philox_sweep_ref.py and oracle/philox.py's Philox stream.  It is not a
transliteration of the kernel: libm exp / log, ``np.linalg.inv`` for the precision block, divisions
where the kernel multiplies.

The scheme (ISSUE): for chain c and new customer i one shadow chain runs over
that chain's level-2 records.  Inner sweep number t (1-based from ``sweep_first``, warm-up counted)
is one production level-1 sweep (``sweep_level1``) with the variates of key chain_key(seed +
chain_first + c) and counter (customer_offset + i, t, slot, customer stream); ``warmup`` sweeps run
against record 0 and record nothing, then ``inner`` sweeps against each record, the state after the
last being that record's draw (lambda, mu, tau, z, [eta]).

The module also holds the synthetic level-2 records of the tests (``synth_level2``), the GPU
module's cases (``CASES``) and the oracle of the distribution test: each customer's posterior means
of log lambda, log mu and P(alive) by two-dimensional Simpson quadrature (``quadrature_means``).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import philox as oph
from oracle import ref_cpu as orc
from tests import ic_ref
from tests import philox_sweep_ref as M

SUM_STATS = ("lambda", "mu", "z", "log_lambda", "log_mu", "lambda2", "mu2", "eta", "log_eta", "mu_capped", "tau")
MU_CAP_SUMMARY = 0.05


# ---------------------------------------------------------------------------------------------
# the problem, the records, the variates
# ---------------------------------------------------------------------------------------------
class ScoreProblem:
    """The new customers as the model sees them (no prior, no initial state: none is needed)."""

    def __init__(self, df, covariates, D, omega2=None):
        cbs, self.X = orc.design_matrix(df, covariates)
        self.D, (self.N, self.K) = D, self.X.shape
        self.covs = list(covariates)
        self.df = df
        self.x = cbs["x"].to_numpy()
        self.t_x = cbs["t_x"].to_numpy().astype(np.float64)
        self.T_cal = cbs["T_cal"].to_numpy().astype(np.float64)
        self.log_s = self.omega2 = None
        if D == 3:
            self.log_s = cbs["log_s"].to_numpy().astype(np.float64)
            self.omega2 = float(cbs["log_s"].var()) if omega2 is None else float(omega2)

    def level1(self, lam, mu, beta, Sigma, var, rows=slice(None)):
        ls = None if self.log_s is None else self.log_s[rows]
        return M.sweep_level1(self.x[rows], self.t_x[rows], self.T_cal[rows], self.X[rows], lam, mu, beta, Sigma, var,
                              log_s=ls, omega2=self.omega2)


def synth_level2(D, K, chains, n_draws, seed, plant=True):
    """[chain][draw][D K + D (D + 1) / 2] records in l2_record's layout: beta's intercept row near
    (log 0.05, log 0.05, 3.0) with N(0, 0.1^2) noise and N(0, 0.3^2) covariate rows; Sigma = L L' with
    diagonals around (1.0, 2.5, 0.5) and random correlations.  ``plant``: per chain record 1 has
    Sigma_11 = 40 (proposals reach the mu cap and the +-70 clip) and record 2 a correlation of 0.99
    between log lambda and log mu (both where n_draws allows)."""
    rng = np.random.default_rng(seed)
    out = np.empty((chains, n_draws, D * K + D * (D + 1) // 2))
    base = np.array([math.log(0.05), math.log(0.05), 3.0])[:D]
    diag = np.array([1.0, 2.5, 0.5])[:D]
    for c in range(chains):
        for d in range(n_draws):
            beta = rng.normal(0.0, 0.3, size=(K, D))
            beta[0] = base + rng.normal(0.0, 0.1, size=D)
            sd = np.sqrt(diag * np.exp(rng.normal(0.0, 0.1, size=D)))
            A = rng.normal(size=(D, D + 2))
            R = A @ A.T
            R = R / np.sqrt(np.outer(np.diag(R), np.diag(R)))       # a random correlation matrix
            Sigma = R * np.outer(sd, sd)
            if plant and d == 1:
                s1 = math.sqrt(40.0)
                scale = np.ones(D)
                scale[1] = s1 / sd[1]
                Sigma = Sigma * np.outer(scale, scale)
            if plant and d == 2:
                r = 0.99 / R[0, 1]
                Sigma[0, 1] = Sigma[1, 0] = Sigma[0, 1] * r
                if D == 3:   # keep it positive definite: the third coordinate uncorrelated with the first two
                    Sigma[0, 2] = Sigma[2, 0] = Sigma[1, 2] = Sigma[2, 1] = 0.0
            Sigma = 0.5 * (Sigma + Sigma.T)
            assert np.linalg.eigvalsh(Sigma).min() > 0
            out[c, d] = M.l2_record(beta, Sigma)
    return out


def variates_at(seed, chain, sweep, customers, S):
    """philox_sweep_ref.oracle_variates for the given global customer indices (oracle.philox's
    sweep_variates takes customers 0 .. n - 1 only): the same words, the same casts."""
    cust = np.asarray(customers, dtype=np.int64)
    r = oph.customer_blocks(seed, chain, cust, sweep, oph.SLOT_ZTAU)
    out = dict(u_z=oph.u53(r[:, 0], r[:, 1]), u_tau=oph.u53(r[:, 2], r[:, 3]),
               e_alive=-np.log(oph.u53_open0(r[:, 2], r[:, 3])))
    re = oph.customer_blocks(seed, chain, cust, sweep, oph.SLOT_ETA)
    out["eta_z"] = (np.sqrt(-2.0 * np.log(oph.u53_open0(re[:, 0], re[:, 1])))
                    * np.cos(2.0 * np.pi * oph.u53(re[:, 2], re[:, 3])))
    n = cust.shape[0]
    tl, tm, ua = (np.empty((S, n), np.float32) for _ in range(3))
    for j in range(S):
        ul, um, al, am, uacc = oph.mh_step_words(seed, chain, cust, sweep, j)
        tl[j], tm[j], ua[j] = oph.t3_f32(ul, al), oph.t3_f32(um, am), uacc
    out.update(t_l=tl, t_m=tm, u_acc=ua)
    out["log2_u"] = np.log2(ua.astype(np.float64)).astype(np.float32)
    return out


def default_init(level2, X, D, K):
    """lambda_0 = exp(x_i' beta_{c,0}[:, 0]), mu_0 = exp(x_i' beta_{c,0}[:, 1]): [chain][N] each."""
    lam, mu = [], []
    for c in range(level2.shape[0]):
        beta, _ = M.l2_unpack(level2[c, 0], D, K)
        mv = X @ beta
        lam.append(np.exp(mv[:, 0]))
        mu.append(np.exp(mv[:, 1]))
    return np.stack(lam), np.stack(mu)


# ---------------------------------------------------------------------------------------------
# the model of one call
# ---------------------------------------------------------------------------------------------
def run_chain(sp: ScoreProblem, records, lam, mu, *, seed, chain, S, inner, warmup=0, sweep_first=1, offset=0,
              variates=None):
    """One chain of one call from the state (lam, mu): returns dict(level1 [n_draws][N][D + 2], lam,
    mu, lam_in, mu_in (the state entering the last inner sweep: tau's tolerance is in its terms),
    margin [N] (the smallest decision margin over every inner sweep of the call), hit_clip,
    hit_cap, z0, z1 [N] flags, next_sweep).  ``variates(chain, t)``: the variates of inner sweep t
    (default: the oracle's of (seed, chain) at customers offset, offset + 1, ...)."""
    D, K, N = sp.D, sp.K, sp.N
    cust = offset + np.arange(N)
    variates = variates or (lambda c, t: variates_at(seed, c, t, cust, S))
    nd = records.shape[0]
    l1 = np.empty((nd, N, D + 2))
    margin = np.full(N, np.inf)
    flags = {k: np.zeros(N, bool) for k in ("hit_clip", "hit_cap", "z0", "z1")}
    lam, mu = np.asarray(lam, np.float64).copy(), np.asarray(mu, np.float64).copy()
    t = sweep_first
    for d in range(-1 if warmup > 0 else 0, nd):
        beta, Sigma = M.l2_unpack(records[max(d, 0)], D, K)
        for _ in range(warmup if d < 0 else inner):
            lam_in, mu_in = lam, mu
            r = sp.level1(lam, mu, beta, Sigma, variates(chain, t))
            lam, mu = r["lam"], r["mu"]
            margin = np.minimum(margin, r["margin"])
            flags["hit_clip"] |= r["hit_clip"]
            flags["hit_cap"] |= r["hit_cap"]
            flags["z1"] |= r["z"]
            flags["z0"] |= ~r["z"]
            t += 1
        if d >= 0:
            l1[d, :, 0], l1[d, :, 1], l1[d, :, 2], l1[d, :, 3] = lam, mu, r["tau"], r["z"].astype(np.float64)
            if D == 3:
                l1[d, :, 4] = r["eta"]
    return dict(level1=l1, lam=lam, mu=mu, lam_in=lam_in, mu_in=mu_in, margin=margin, next_sweep=t, **flags)


def summary_sums(l1, log=np.log):
    """[stat][N] sums of one chain's recorded draws [n_draws][N][D + 2], sequential in record order
    (np.cumsum's last row), as the summary sink defines them: functions of the recorded draws."""
    lam, mu, tau, z = l1[..., 0], l1[..., 1], l1[..., 2], l1[..., 3]
    cols = dict(lambda_=lam, mu=mu, z=z, log_lambda=log(lam), log_mu=log(mu), lambda2=lam * lam, mu2=mu * mu,
                mu_capped=np.minimum(mu, MU_CAP_SUMMARY), tau=tau)
    if l1.shape[-1] == 5:
        cols.update(eta=l1[..., 4], log_eta=log(l1[..., 4]))
    out = np.zeros((len(SUM_STATS), l1.shape[1]))
    for k, name in enumerate(SUM_STATS):
        v = cols.get("lambda_" if name == "lambda" else name)
        if v is not None:
            out[k] = np.cumsum(v, axis=0)[-1]
    return out


# ---------------------------------------------------------------------------------------------
# the GPU module's cases (ISSUE table)
# ---------------------------------------------------------------------------------------------
def _case(D, K, N, chains, chain_first, records, R, S, offset, seed):
    return dict(D=D, K=K, N=N, chains=chains, chain_first=chain_first, records=records, R=R, S=S, offset=offset,
                seed=seed, covs=[f"c{k}" for k in range(1, K)])


CASES = {
    "bi1": _case(2, 1, 1, 1, 0, 6, 1, 20, 0, 9101),
    "bi2": _case(2, 2, 255, 3, 0, 6, 1, 7, 0, 9102),
    "bi5": _case(2, 5, 257, 2, 2, 6, 3, 20, 70000, 9103),
    "bi9": _case(2, 9, 600, 1, 0, 4, 1, 20, 0, 9104),
    "tri3": _case(3, 3, 257, 2, 0, 6, 3, 23, 0, 9105),
    "tri9": _case(3, 9, 384, 2, 0, 4, 1, 20, 0, 9106),
    "bi1_s0": _case(2, 1, 300, 2, 0, 4, 1, 0, 0, 9107),
}
# Coverage events each case must show among its compared lanes (asserted on the model alone by
# tests/test_score_cpu.py and on the device by tests/test_gpu_score.py): a proposal above the mu cap,
# a proposal at the +-70 clip, both z outcomes.  One customer (bi1) cannot show both z outcomes in
# every run, and without MH steps (bi1_s0) nothing is proposed: recorded here, not dropped silently.
COVERAGE = {name: ("hit_cap", "hit_clip", "z0", "z1") for name in CASES}
COVERAGE["bi1_s0"] = ("z0", "z1")


def case_problem(case):
    from tests.helpers import cdnow_tiled, with_covariates
    df = cdnow_tiled(case["N"])
    if case["K"] > 1:
        df = with_covariates(df, case["K"] - 1)
    return ScoreProblem(df, case["covs"], case["D"])


def case_level2(case):
    return synth_level2(case["D"], case["K"], case["chains"], case["records"], case["seed"])


# ---------------------------------------------------------------------------------------------
# the distribution test's oracle: posterior means by quadrature
# ---------------------------------------------------------------------------------------------
DIST_SEED = 20250101
DIST = dict(chains=4, records=2000, R=2, warmup=50, S=20, n=64)
DIST_MODELS = {"bi2": (2, ["first_sales_scaled"]), "tri3": (3, ["gender_F", "age_scaled"])}


@functools.lru_cache(maxsize=None)
def dist_quadrature(name, n_grid=401):
    """quadrature_means of a distribution-test model, computed once per grid."""
    return quadrature_means(dist_problem(name), dist_record(name), n_grid)


def dist_problem(name):
    from tests.helpers import cdnow
    D, covs = DIST_MODELS[name]
    return ScoreProblem(cdnow("abe", DIST["n"]), covs, D)


def dist_record(name):
    """The one constant (beta, Sigma) of the distribution test, every chain's every record."""
    D, covs = DIST_MODELS[name]
    return synth_level2(D, len(covs) + 1, 1, 1, 424242 + D, plant=False)[0, 0]


def _simpson_weights(n):
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    return w / 3.0


def quadrature_means(sp, record, n_grid=401, span=12.0):
    """Per customer (E log lambda, E log mu, E P(alive), sd log lambda, sd log mu) under the target of the scoring chain with
    all records equal: the Pareto/NBD likelihood marginal over z and tau (ic_ref.loglik's closed
    form) times the Gaussian of (log lambda, log mu) with mean x' beta[:, :2] and precision
    inv_sigma_block(Sigma) (quirk Q4 for D = 3), truncated at log mu <= 5 (quirk Q3).  Composite
    Simpson on an n_grid x n_grid grid (odd) over mean +- span sd of that Gaussian; the log mu axis
    ends at 5 exactly where the box would pass it."""
    assert n_grid % 2 == 1
    beta, Sigma = M.l2_unpack(record, sp.D, sp.K)
    P = M.inv_sigma_block(Sigma)
    sd = np.sqrt(np.diag(np.linalg.inv(P)))
    mv = sp.X @ beta
    w = np.outer(_simpson_weights(n_grid), _simpson_weights(n_grid))
    out = np.empty((sp.N, 5))
    for i in range(sp.N):
        a = np.linspace(mv[i, 0] - span * sd[0], mv[i, 0] + span * sd[0], n_grid)
        b = np.linspace(mv[i, 1] - span * sd[1], min(mv[i, 1] + span * sd[1], M.MU_CAP), n_grid)
        A, B = np.meshgrid(a, b, indexing="ij")
        lam, mu = np.exp(A), np.exp(B)
        d = dict(x=np.array([sp.x[i]]), t_x=sp.t_x[i], T_cal=sp.T_cal[i])
        ll = ic_ref.loglik(np.stack([lam, mu], axis=-1), d)
        da, db = A - mv[i, 0], B - mv[i, 1]
        lp = ll - 0.5 * (da * da * P[0, 0] + 2.0 * da * db * P[0, 1] + db * db * P[1, 1])
        dens = np.exp(lp - lp.max()) * w          # the cell sizes cancel in the ratios
        tot = dens.sum()
        with np.errstate(under="ignore"):
            pa = orc.p_alive(sp.t_x[i], sp.T_cal[i], lam, mu)
        ma, mb = (dens * A).sum() / tot, (dens * B).sum() / tot
        out[i] = (ma, mb, (dens * pa).sum() / tot, math.sqrt((dens * (A - ma) ** 2).sum() / tot),
                  math.sqrt((dens * (B - mb) ** 2).sum() / tot))
    return out


def dist_series(l1, sp: ScoreProblem):
    """The three series of the distribution test from level-1 draws [chain][draw][N][D + 2]:
    log lambda, log mu and the Rao-Blackwellised P(alive) = p_alive(lambda, mu): [3][chain][draw][N]."""
    lam, mu = l1[..., 0], l1[..., 1]
    with np.errstate(under="ignore"):
        pa = orc.p_alive(sp.t_x, sp.T_cal, lam, mu)
    return np.stack([np.log(lam), np.log(mu), pa])


def dist_check(series, quad):
    """Per (quantity, customer): (|mean of the series - quadrature|, MCSE), the MCSE being that of
    diagnostics_ref.series_stats on the series itself: two [3][N] arrays.  A series that never moves
    (P(alive) of a customer with t_x = T_cal is exactly 1 in every draw) has MCSE 0: it must then
    equal the quadrature's value exactly (both are 1: the bound |diff| <= 5 MCSE then reads 0 <= 0)."""
    from tests.diagnostics_ref import series_stats
    n = series.shape[-1]
    diff, mcse = np.empty((3, n)), np.empty((3, n))
    for q in range(3):
        for i in range(n):
            y = series[q, :, :, i]
            if y.min() == y.max():
                diff[q, i], mcse[q, i] = abs(y.flat[0] - quad[i, q]), 0.0
                continue
            st, _ = series_stats(y)
            diff[q, i], mcse[q, i] = abs(st[0] - quad[i, q]), st[2]
    return diff, mcse


DIST_SIGMAS = 5.0


def dist_ok(diff, mcse):
    return diff <= DIST_SIGMAS * mcse


def model_dist_run(name):
    """The float64 model's own run of the distribution test: level-1 draws [chain][draw][N][D + 2].
    The chains share one constant record, so they run as one batch of chains x N lanes."""
    sp = dist_problem(name)
    rec = dist_record(name)
    C, nd, R, W, S, n = (DIST[k] for k in ("chains", "records", "R", "warmup", "S", "n"))
    beta, Sigma = M.l2_unpack(rec, sp.D, sp.K)
    lam0, mu0 = default_init(np.broadcast_to(rec, (C, 1, rec.shape[0])), sp.X, sp.D, sp.K)
    rows = np.tile(np.arange(n), C)
    lam, mu = lam0.ravel(), mu0.ravel()
    l1 = np.empty((C, nd, n, sp.D + 2))
    total = W + R * nd
    t, BATCH = 1, 64               # the variates of BATCH inner sweeps drawn in one Philox call per chain
    cache = {}

    def var(t):
        if t not in cache:
            cache.clear()
            ts = np.arange(t, min(t + BATCH, total + 1))
            parts = []
            for c in range(C):
                v = _variates_block(DIST_SEED, c, ts, np.arange(n), S)
                parts.append(v)
            for j, tt in enumerate(ts):
                cache[int(tt)] = {k: np.concatenate([p[k][j] for p in parts], axis=-1) for k in parts[0]}
        return cache[t]

    for d in range(-1, nd):
        for _ in range(W if d < 0 else R):
            r = sp.level1(lam, mu, beta, Sigma, var(t), rows=rows)
            lam, mu = r["lam"], r["mu"]
            t += 1
        if d >= 0:
            cols = [lam, mu, r["tau"], r["z"].astype(np.float64)] + ([r["eta"]] if sp.D == 3 else [])
            l1[:, d] = np.stack(cols, axis=-1).reshape(C, n, sp.D + 2)
    return sp, rec, l1


def _variates_block(seed, chain, sweeps, customers, S):
    """variates_at for several inner sweeps at once: dict of arrays with a leading sweep axis."""
    ns, n = len(sweeps), len(customers)
    cust = np.tile(np.asarray(customers, np.int64), ns)
    sw = np.repeat(np.asarray(sweeps, np.int64), n)
    v = variates_at(seed, chain, sw, cust, S)
    out = {}
    for k, a in v.items():
        out[k] = a.reshape(ns, n) if a.ndim == 1 else a.reshape(S, ns, n).transpose(1, 0, 2)
    return out

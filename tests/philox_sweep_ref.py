"""Float64 model of ONE Philox-mode (production) sweep — TEST INFRASTRUCTURE ONLY, plain numpy.

Written from the reference's equations as ``oracle/ref_cpu.py`` restates them (``p_alive``,
``tau_churned``, ``log_posterior``, ``draw_eta``, ``level2_posterior``, ``invwishart_from_variates``,
``lik_terms``) and from the documented Philox stream layout (``oracle/philox.py``).  It is NOT a
transliteration of ``csrc/kernels.hip``: it divides where the kernel multiplies, evaluates the log
posterior in the reference's direct form (no expanded quadratic), calls libm exp/log, and draws
nothing ahead.  ``tests/test_philox_sweep_cpu.py`` pins it to the reference's recorded outputs and to
``run_chain_bi`` / ``run_chain_tri``; ``tests/test_gpu_production_sweep.py`` holds the device to it.

It follows the reference's semantics with the production path's documented deviations only:

* Q3 cap: a proposal with ``lm > 5`` has log posterior ``-inf`` and NaN never accepts (the
  reference's own behaviour, taken in the log domain: accept iff ``pm <= 5`` and
  ``lp' - lp > ln 2 * log2 U``);
* the proposal clipped to [-70, 70] (bi:323-324);
* ``min(700, .)`` in tau's exponents (bi:223);
* natural-scale ``lambda = exp(ll)`` after the MH steps, with no exp(log(.)) storage round trip
  (quirk Q5), and level 2 sees the log-scale state itself.

Every accept/reject and the alive/churned draw is a comparison of two computed numbers; the model
returns, per customer, the smallest relative distance of any of them from its threshold (the
"decision margin"), so a caller can set aside the lanes where two correct float64 evaluations may
legitimately decide differently.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import philox as oph
from oracle import ref_cpu as orc

LN2 = math.log(2.0)
MU_CAP = 5.0           # quirk Q3 (bi:309)
CLIP = 70.0            # bi:323-324
# comparison tolerance of lambda, mu, tau, eta and the likelihood term; a lane whose decision margin
# is below it is "borderline"
RTOL = 1e-12
# tau's absolute term is TAU_ATOL_ULPS * 2^-52 / (lambda + mu): see tau_atol()
TAU_ATOL_ULPS = 8.0
BORDERLINE_CAP = 1e-3  # at most 0.1% of compared lanes per case may be borderline
# level-2 record: the project's replay-parity figures (S_n summed in another order); ten times the
# sensitivity measured by test_level2_tolerance_covers_the_measured_sensitivity stays below L2_RTOL
L2_RTOL, L2_ATOL = 1e-10, 1e-12


def l2_deviation(got, ref):
    """Relative deviation of a level-2 quantity after the absolute allowance: <= L2_RTOL passes."""
    ref = np.asarray(ref, dtype=np.float64)
    return np.maximum(np.abs(np.asarray(got) - ref) - L2_ATOL, 0.0) / np.maximum(np.abs(ref), 1e-300)


def near_edges(mp, z, tau, frac=0.05):
    """Churned draws whose tau lies in the first / last ``frac`` of [t_x, T_cal]: where the truncated
    exponential's log argument is closest to its ends."""
    span = mp.T_cal - mp.t_x
    churned = ~np.asarray(z, dtype=bool)
    return churned & (tau - mp.t_x < frac * span), churned & (mp.T_cal - tau < frac * span)


def tau_atol(lam, mu):
    """Absolute tolerance of tau.  Churned: tau = -log(arg) / ml with arg = (1-u) e^-ml tx + u e^-ml T.
    d tau = -(d arg / arg) / ml: the condition number of log at arg -> 1 is 1 / |log arg|, so a
    relative error of arg passes to tau as an ABSOLUTE error (d arg / arg) / ml however small tau is.
    arg's relative error between two correct evaluations: the two exps at <= 2 ulp (table exp) + 1 ulp
    (libm) = 3, two products and a sum rounded once each on either side = 3, the log's own rounding 2:
    8 ulp of 2^-52, divided by ml."""
    return TAU_ATOL_ULPS * 2.0 ** -52 / (np.asarray(lam) + np.asarray(mu))


# ---------------------------------------------------------------------------------------------
# level 1
# ---------------------------------------------------------------------------------------------
def draw_z_tau(t_x, T_cal, lam, mu, u_z, u_tau, e_alive, swap_tau_branch=False, no_cap700=False, swap_span=False):
    """bi:193-227 with the sweep's Philox variates: z = u_z < P(alive); tau = T + E / mu (alive, E =
    -log U' of the SLOT_ZTAU words (z, w)) or the truncated-exponential inverse CDF at U of the same
    words (churned).  Returns (z, tau, relative margin of the z decision).
    Power checks only: ``swap_tau_branch`` puts each branch's formula on the other branch's lanes;
    ``no_cap700`` leaves min(700, .) out of tau's exponents (bi:223); ``swap_span`` forms P(alive)'s
    exponential from ml (t_x - T) instead of ml (T - t_x)."""
    ml = mu + lam
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(-(ml * ((t_x - T_cal) if swap_span else (T_cal - t_x))))
    a = ml * e
    b = a + mu * (1.0 - e)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = u_z < a / b
    lhs = u_z * b
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.abs(lhs - a) / (lhs + a)   # both sides carry a few ulp of their own size
    margin = np.where(np.isfinite(margin), margin, 0.0)
    with np.errstate(under="ignore", divide="ignore"):
        if no_cap700:
            churned = -np.log((1 - u_tau) * np.exp(-(ml * t_x)) + u_tau * np.exp(-(ml * T_cal))) / ml
        else:
            churned = orc.tau_churned(t_x, T_cal, ml, u_tau)
    alive = T_cal + (1.0 / mu) * e_alive
    tau = np.where(z != bool(swap_tau_branch), alive, churned)
    return z, tau, margin


def inv_sigma_block(Sigma):
    """bi:281 / tri:402: the [0:2, 0:2] block of the full inverse (quirk Q4 for D = 3)."""
    return np.linalg.inv(np.asarray(Sigma, dtype=np.float64))[:2, :2]


def lp_magnitude(x, w, mv, P, ll, lm, pl, pm):
    """Size of the terms that make up lp(pl, pm) - lp(ll, lm): the scale its rounding error is
    relative to (as ``mag`` in test_device_mh_step_matches_reference_log_posterior)."""
    pmax = np.abs(P).max()
    quad = lambda a, b: (np.abs(a - mv[:, 0]) + np.abs(b - mv[:, 1])) ** 2 * pmax  # noqa: E731
    with np.errstate(over="ignore"):
        ex = np.exp(np.minimum(ll, 700)) + np.exp(np.minimum(lm, 700)) + np.exp(pl) + np.exp(np.minimum(pm, 700))
    return (np.abs(x * ll) + np.abs(x * pl) + np.abs(lm) + np.abs(pm) + w * ex
            + quad(ll, lm) + quad(pl, pm) + np.abs(mv).sum(1) ** 2 * pmax + 1.0)


def mh_steps(x, T_cal, z, tau, mv, P, s00, s11, ll, lm, t_l, t_m, log2_u, stages=None, clip=CLIP):
    """bi:312-335 for S = len(t_l) steps from (ll, lm): proposal ll + Sigma[0,0] t (variance as the
    scale, quirk Q2) clipped to [-70, 70]; accept iff pm <= 5 and lp' - lp > ln2 log2 U (false on NaN;
    any finite lp' from lp = -inf).  Returns (ll, lm, cur, margin, hit_clip, hit_cap).
    ``clip`` (power checks only): another clip than the reference's 70."""
    n = ll.shape[0]
    ll, lm = ll.copy(), lm.copy()
    w = np.where(z, T_cal, tau)
    xf = np.asarray(x, dtype=np.float64)
    zf = z.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cur = orc.log_posterior(ll, lm, xf, zf, T_cal, tau, mv, P)
    margin = np.full(n, np.inf)
    hit_clip = np.zeros(n, bool)
    hit_cap = np.zeros(n, bool)
    for j in range(len(t_l)):
        raw_l = ll + s00 * t_l[j].astype(np.float64)
        raw_m = lm + s11 * t_m[j].astype(np.float64)
        pl = np.clip(raw_l, -clip, clip)
        pm = np.clip(raw_m, -clip, clip)
        hit_clip |= (np.abs(raw_l) >= clip) | (np.abs(raw_m) >= clip)
        with np.errstate(invalid="ignore", over="ignore"):
            plp = orc.log_posterior(pl, pm, xf, zf, T_cal, tau, mv, P)
            thr = LN2 * log2_u[j].astype(np.float64)
            d = plp - cur                               # NaN for -inf - -inf: never accepted
            capped = pm > MU_CAP
            hit_cap |= capped
            acc = ~capped & (d > thr)
            m_lp = np.abs(d - thr) / lp_magnitude(xf, w, mv, P, ll, lm, pl, pm)
        m_lp = np.where(capped | ~np.isfinite(d), np.inf, m_lp)   # decided by the cap / an infinity
        margin = np.minimum(margin, np.minimum(m_lp, np.abs(MU_CAP - pm)))
        if stages is not None:
            stages.append(dict(pl=pl, pm=pm, plp=plp, cur=cur.copy(), accept=acc))
        ll[acc] = pl[acc]
        lm[acc] = pm[acc]
        cur[acc] = plp[acc]
    return ll, lm, cur, margin, hit_clip, hit_cap


class _One:
    """The ``Stream`` face draw_eta needs: hands out the given standard normals."""
    def __init__(self, zeta):
        self.zeta = zeta

    def standard_normal(self, n, key):
        assert n == self.zeta.shape[0]
        return self.zeta


def sweep_level1(x, t_x, T_cal, X, lam, mu, beta, Sigma, var, log_s=None, omega2=None,
                 swap_tau_branch=False, stages=False, no_cap700=False, swap_span=False, clip=CLIP):
    """One chain, one sweep's level-1 half (bi:388-396; tri:511-526) from the state (lam, mu) entering
    it, the (beta K x D, Sigma D x D) its MH uses, and its variates ``var``: u_z, u_tau, e_alive (n),
    t_l / t_m / log2_u (S x n, the device's fp32 values or the oracle's), eta_z (n, D = 3).
    Returns a dict: z, tau, lam, mu, ll, lm, (eta, leta), lik (the likelihood term, bi:415-427),
    margin (the smallest of margin_z, margin_mh) and hit_clip / hit_cap flags; ``stages=True`` adds
    the per-step proposals and log posteriors under "steps" and the coefficients mv, P.
    ``no_cap700``, ``swap_span``, ``clip``: the power checks' wrong models (draw_z_tau, mh_steps)."""
    lam = np.asarray(lam, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    Sigma = np.asarray(Sigma, dtype=np.float64)
    z, tau, margin_z = draw_z_tau(t_x, T_cal, lam, mu, var["u_z"], var["u_tau"], var["e_alive"], swap_tau_branch,
                                   no_cap700, swap_span)
    mv = X @ beta
    P = inv_sigma_block(Sigma)
    steps = [] if stages else None
    ll, lm, cur, margin_mh, hit_clip, hit_cap = mh_steps(
        x, T_cal, z, tau, mv, P, Sigma[0, 0], Sigma[1, 1], np.log(lam), np.log(mu),
        var["t_l"], var["t_m"], var["log2_u"], steps, clip)
    out = dict(z=z, tau=tau, ll=ll, lm=lm, lam=np.exp(ll), mu=np.exp(lm), cur=cur, margin_z=margin_z,
               margin_mh=margin_mh, margin=np.minimum(margin_z, margin_mh), hit_clip=hit_clip, hit_cap=hit_cap)
    if Sigma.shape[0] == 3:
        leta = orc.draw_eta(log_s, X, beta, Sigma, omega2, _One(var["eta_z"]))   # tri:306-333 (log scale)
        out.update(leta=leta, eta=np.exp(leta))
    zf = z.astype(np.float64)
    # bi:415-427 on the natural-scale state (log(exp(ll)) = ll: no round trip)
    out["lik"] = x * ll + (1 - zf) * lm - (out["lam"] + out["mu"]) * (zf * T_cal + (1 - zf) * tau)
    if stages:
        out.update(steps=steps, mv=mv, P=P)
    return out


# ---------------------------------------------------------------------------------------------
# level 2
# ---------------------------------------------------------------------------------------------
def level2_draw(X, Y, hyper, iw_normal, iw_chi2, beta_z):
    """bi:233-262 / tri:340-380 from the variates: Sigma ~ IW by scipy's Bartlett form, then
    beta = B_hat + kron(chol Sigma, chol V) z paired with B_hat's row-major ravel (quirk Q1) — the
    lower-Cholesky factor of the reference's kron(Sigma, V) covariance.  Returns a dict."""
    V, B_hat, S_n, nu_n = orc.level2_posterior(X, Y, hyper)
    Sigma = orc.invwishart_from_variates(S_n, np.asarray(iw_normal, dtype=np.float64), np.asarray(iw_chi2, dtype=np.float64))
    F = np.kron(np.linalg.cholesky(Sigma), np.linalg.cholesky(V))
    beta = (B_hat.ravel() + F @ np.asarray(beta_z, dtype=np.float64)).reshape(B_hat.shape)
    return dict(beta=beta, Sigma=Sigma, B_hat=B_hat, S_n=S_n, nu_n=nu_n, V=V, factor=F)


def hyper_variates(seed, chain, hsweep, D, K, nu_n, beta_slot_shift=0):
    """The hyper stream's variates of the level-2 draw that BELONGS TO sweep ``hsweep`` (the sweep
    whose MH uses it for D = 2 — drawn after sweep hsweep - 1, the first from the initial state; the
    sweep it follows for D = 3): Bartlett normals in slots HSLOT_NORMAL0 + [0, D(D-1)/2), the beta
    normals in HSLOT_BETA_NORMAL0 + [0, D K), chi-square q with nu_n - D + 1 + q degrees of freedom.
    ``beta_slot_shift`` (power checks only) moves the beta normals' slots."""
    iw = np.array([oph.hyper_normal(seed, chain, oph.HSLOT_NORMAL0 + i, hsweep) for i in range(D * (D - 1) // 2)])
    chi = np.array([oph.chi2_draw(seed, chain, hsweep, q, nu_n - D + 1 + q) for q in range(D)])
    bz = np.array([oph.hyper_normal(seed, chain, oph.HSLOT_BETA_NORMAL0 + beta_slot_shift + j, hsweep)
                   for j in range(D * K)])
    return iw, chi, bz


def l2_record(beta, Sigma):
    """The stored level-2 row (bi:411-412, tri:549-554): beta.T.ravel(), then Sigma's upper triangle."""
    D = Sigma.shape[0]
    return np.concatenate([np.asarray(beta).T.ravel(), Sigma[np.triu_indices(D)]])


def l2_unpack(row, D, K):
    beta = np.asarray(row[: D * K]).reshape(D, K).T.copy()
    Sigma = np.zeros((D, D))
    Sigma[np.triu_indices(D)] = row[D * K:]
    Sigma = Sigma + np.triu(Sigma, 1).T
    return beta, Sigma


# ---------------------------------------------------------------------------------------------
# a problem as the model sees it, the test cases, and a free-running model chain
# ---------------------------------------------------------------------------------------------
class ModelProblem:
    """The reference's setup (bi:367-374, 467-479; tri:488-499, 615-626) from a CBS DataFrame."""

    def __init__(self, df, covariates, D):
        cbs, self.X = orc.design_matrix(df, covariates)
        self.D, (self.N, self.K) = D, self.X.shape
        self.x = cbs["x"].to_numpy()
        self.t_x = cbs["t_x"].to_numpy().astype(np.float64)
        self.T_cal = cbs["T_cal"].to_numpy().astype(np.float64)
        self.hyper = orc.default_hyper(self.K, D)
        _, self.lam0, self.mu0 = orc.init_state(self.x, self.t_x, self.T_cal)
        self.hyper["beta_0"][0, 0] = math.log(self.lam0.mean())
        self.hyper["beta_0"][0, 1] = math.log(self.mu0.mean())
        self.log_s = self.omega2 = None
        if D == 3:
            self.log_s = cbs["log_s"].to_numpy()
            self.omega2 = float(cbs["log_s"].var())
            self.hyper["beta_0"][0, 2] = cbs["log_s"].mean()
        self.nu_n = self.hyper["nu_00"] + self.N

    def level1(self, lam, mu, beta, Sigma, var, **kw):
        return sweep_level1(self.x, self.t_x, self.T_cal, self.X, lam, mu, beta, Sigma, var,
                            log_s=self.log_s, omega2=self.omega2, **kw)

    def level2(self, seed, chain, hsweep, Y, hsweep_of_variates=None, beta_slot_shift=0, rows=None):
        """``rows`` (power checks only): the customers whose rows of X and Y enter the statistics; the
        variates keep the whole problem's nu_n."""
        hv = hyper_variates(seed, chain, hsweep if hsweep_of_variates is None else hsweep_of_variates,
                            self.D, self.K, self.nu_n, beta_slot_shift)
        X = self.X if rows is None else self.X[rows]
        return level2_draw(X, Y if rows is None else Y[rows], self.hyper, *hv)


# The GPU module's cases (ISSUE table): name -> D, covariates, data, N, S, chains, chain_first, seed,
# burnin, mcmc, thin and the driving ("run" n sweeps / "state" = get_state).
CASES = {
    "bi_k1": dict(D=2, covs=[], data=("abe", 300, 0), S=20, chains=3, chain_first=0, seed=20240611,
                  burnin=0, mcmc=6, thin=1, drive=[("run", 6)]),
    "bi_k2": dict(D=2, covs=["first_sales_scaled"], data=("abe", 600, 0), S=7, chains=2, chain_first=0, seed=77,
                  burnin=5, mcmc=4, thin=1, drive=[("run", 5), ("state",), ("run", 4)]),
    "bi_k5": dict(D=2, covs=["c1", "c2", "c3", "c4"], data=("abe", 384, 4), S=20, chains=1, chain_first=2, seed=1234,
                  burnin=2, mcmc=6, thin=3, drive=[("run", 1), ("state",)] * 8),
    "tri_k3": dict(D=3, covs=["gender_F", "age_scaled"], data=("abe", 300, 0), S=23, chains=2, chain_first=0,
                   seed=99, burnin=0, mcmc=6, thin=1, drive=[("run", 6)]),
    "tri_k9": dict(D=3, covs=[f"c{k}" for k in range(1, 9)], data=("abe", 384, 8), S=20, chains=2, chain_first=0,
                   seed=4242, burnin=0, mcmc=5, thin=1, drive=[("run", 5)]),
    "bi_k1_s0": dict(D=2, covs=[], data=("abe", 300, 0), S=0, chains=2, chain_first=0, seed=5,
                     burnin=0, mcmc=6, thin=1, drive=[("run", 6)]),
}


BLOCK = 256            # customers per workgroup (CLV_BLOCK)
NT = 256               # lanes of the level-2 workgroup: it holds units u, u + NT, then strides by NT


def _instance_case(D, K):
    """One case per compiled (D, K) instance.  N = 257 / 512 / 256 by (K - 1) % 3 — a last block of one
    active lane, no partly filled block, one single full block — so each occurs for K < 6 and K >= 6
    (covariates in registers / in LDS) for both D.  S = 6: one full MH chunk of 4 and a partial one."""
    n = (257, 512, 256)[(K - 1) % 3]
    return dict(D=D, covs=[f"c{k}" for k in range(1, K)], data=("abe", n, K - 1), S=6, chains=2, chain_first=K % 2,
                seed=1000 + 10 * D + K, burnin=0, mcmc=3, thin=1, drive=[("run", 3)])


INSTANCE_CASES = {f"{'bi' if D == 2 else 'tri'}{K}": _instance_case(D, K) for D in (2, 3) for K in range(1, 10)}

# Coverage events the model's free run of each instance case produces (chains x 3 sweeps; recorded and
# asserted by test_philox_sweep_cpu.test_instance_coverage_table_is_what_the_model_produces): an x = 0
# customer, a churned tau in the first / last 5% of [t_x, T], a proposal at the +-70 clip, a proposal
# above the mu cap.  The GPU module asserts exactly these per case.  Every case has x0, near_tx and
# near_T.  The trivariate cases propose sweep 1 with gamma_00's variances (4 + K), so all of them hit
# the clip (6..117 lanes) and the cap (337..967 lanes).  The bivariate cases propose with a drawn
# Sigma: 257..512 customers x 2 chains x 3 sweeps x 6 steps never reach the +-70 clip, and K = 1..4
# never propose above the mu cap either (K = 5..9: 1 or 2 lanes; bi_k1 of CASES: 19) — the clip's code is shared and the
# trivariate cases cover it.
COVERAGE_EVENTS = ("x0", "near_tx", "near_T", "clip", "cap")
_EDGES = ("x0", "near_tx", "near_T")
INSTANCE_COVERAGE = {**{f"bi{K}": _EDGES for K in (1, 2, 3, 4)},
                     **{f"bi{K}": _EDGES + ("cap",) for K in (5, 6, 7, 8, 9)},
                     **{f"tri{K}": COVERAGE_EVENTS for K in range(1, 10)}}


def grid_geometry(case):
    """(blocks, blocks per unit, units per rank, global units) of a world-size-1 run: the library's
    plan rule (clv_create) restated, so a case can assert the geometry it is meant to reach."""
    nb = -(-case["data"][1] // BLOCK)
    bpu = case["blocks_per_unit"]
    if not bpu:  # clv_default_blocks_per_unit: at most 2 NT units
        bpu = 1
        while -(-nb // bpu) > 2 * NT:
            bpu *= 2
    units = -(-nb // bpu)
    return nb, bpu, units, units


def _grid_case(D, K, n, chains, bpu, modes, seed, geometry, drop):
    return dict(D=D, covs=[f"c{k}" for k in range(1, K)], data=("tiled", n, K - 1), S=4, chains=chains, chain_first=0,
                seed=seed, burnin=0, mcmc=2, thin=1, drive=[("run", 2)], blocks_per_unit=bpu, modes=modes,
                geometry=geometry, drop=drop)


# The level-2 reduction paths and large customer indices.  modes: kernel -> the persistent flag asserted;
# geometry: (blocks, blocks per unit, units per rank, global units) asserted before the run; drop: the
# customer ranges [lo, hi) left out of the level-2 model and the log-likelihood mean by the power
# checks (blocks 0, 256 and the last; or the whole last unit).
_N300, _N600, _N41 = 299 * BLOCK + 1, 599 * BLOCK + 1, 10300
_BOTH_KERNELS = dict(default=True, launch_per_sweep=False)
_BLOCKS_300 = {"block 0": (0, BLOCK), "block 256": (256 * BLOCK, 257 * BLOCK), "last block": (299 * BLOCK, _N300)}
GRID_CASES = {
    # persistent: lanes 0..43 of the level-2 workgroup hold two blocks, level-2 workgroup alone on its
    # CU, a last block of one lane; fused tail: hyper_sum_units' two-unit branch, second unit in 44 lanes
    "g_bi1_300": _grid_case(2, 1, _N300, 1, 0, dict(default=True, launch_per_sweep=False), 3101,
                            (300, 1, 300, 300), _BLOCKS_300),
    # NS = 19 > 16: hyper_variates, then the strided loop (two trips)
    "g_tri4_300": _grid_case(3, 4, _N300, 1, 0, dict(default=True, launch_per_sweep=False), 3102,
                             (300, 1, 300, 300), _BLOCKS_300),
    # 600 units > 2 NT: the strided loop with NS <= 16, three trips (blocks_per_unit = 1 set explicitly)
    "g_bi2_600u": _grid_case(2, 2, _N600, 1, 1, dict(default=False), 3103, (600, 1, 600, 600),
                             {"block 0": (0, BLOCK), "block 256": (256 * BLOCK, 257 * BLOCK),
                              "block 512": (512 * BLOCK, 513 * BLOCK), "last block": (599 * BLOCK, _N600)}),
    # unit arrival counters; unit sums by the tail loop only / one batch of 8 / two batches; a last unit
    # of 1 / 1 / 9 blocks over zero padding; two chains' counters side by side
    "g_bi5_u2": _grid_case(2, 5, _N41, 2, 2, dict(default=False), 3104, (41, 2, 21, 21), {"last unit": (20 * 2 * BLOCK, _N41)}),
    "g_bi5_u8": _grid_case(2, 5, _N41, 2, 8, dict(default=False), 3105, (41, 8, 6, 6), {"last unit": (5 * 8 * BLOCK, _N41)}),
    "g_bi5_u16": _grid_case(2, 5, _N41, 2, 16, dict(default=False), 3106, (41, 16, 3, 3), {"last unit": (2 * 16 * BLOCK, _N41)}),
    # the same through the NS > 16 branch (NS = 34, covariates in LDS)
    "g_tri9_u16": _grid_case(3, 9, _N41, 2, 16, dict(default=False), 3107, (41, 16, 3, 3), {"last unit": (2 * 16 * BLOCK, _N41)}),
    # The unsharded side of tests/shard_edge_cases.py, row by row (D, K, N, blocks_per_unit): the sharded
    # exchanges are held to these runs bit for bit, so these runs are held to the model.  Small grids: a
    # last block of one lane, a single full block, a 44-lane block; 6 / 10 blocks as 6 / 10 units; and
    # blocks_per_unit 4 and 2 set explicitly at 6 and 5 blocks (fused tail with unit arrival counters:
    # a last unit of 2 of 4 blocks / 1 of 2 blocks over zero padding).
    "g_bi2_257": _grid_case(2, 2, 257, 2, 0, _BOTH_KERNELS, 3111, (2, 1, 2, 2), {"last block": (BLOCK, 257)}),
    "g_bi1_256": _grid_case(2, 1, 256, 2, 0, _BOTH_KERNELS, 3112, (1, 1, 1, 1), {"wave rows 2-3": (BLOCK // 2, BLOCK)}),
    "g_tri3_300": _grid_case(3, 3, 300, 2, 0, _BOTH_KERNELS, 3113, (2, 1, 2, 2), {"last block": (BLOCK, 300)}),
    "g_bi2_1281": _grid_case(2, 2, 1281, 2, 0, _BOTH_KERNELS, 3114, (6, 1, 6, 6),
                             {"block 4": (4 * BLOCK, 5 * BLOCK), "last block": (5 * BLOCK, 1281)}),
    "g_tri3_1281_u4": _grid_case(3, 3, 1281, 2, 4, dict(default=False), 3115, (6, 4, 2, 2), {"last unit": (4 * BLOCK, 1281)}),
    "g_bi5_1025_u2": _grid_case(2, 5, 1025, 2, 2, dict(default=False), 3116, (5, 2, 3, 3), {"last unit": (4 * BLOCK, 1025)}),
    "g_bi2_abe": dict(_grid_case(2, 2, 2357, 2, 0, _BOTH_KERNELS, 3117, (10, 1, 10, 10), {"last block": (9 * BLOCK, 2357)}),
                      covs=["first_sales_scaled"], data=("abe", 2357, 0)),  # the sample itself, not the tiled frame
}
# the GRID_CASES row of each tests/shard_edge_cases.py case
SHARD_EDGE_GRID = dict(one_lane="g_bi2_257", exact_empty="g_bi1_256", two_empty="g_tri3_300", tail_empty="g_bi2_1281",
                       part_unit="g_tri3_1281_u4", part_unit3="g_bi5_1025_u2", abe_world8="g_bi2_abe")
GRID_RUNS = [(n, m) for n, c in GRID_CASES.items() for m in c["modes"]]


# ---------------------------------------------------------------------------------------------
# the split layout of the persistent sweep (persist_kernel_split; tests/test_gpu_split_model.py)
# ---------------------------------------------------------------------------------------------
ROW = 64               # customers per wave row; a block is 4 rows, a split workgroup hosts 6
SPLIT_MAX_NB = 256     # one level-2 lane per block: the split layout's largest chain
SPLIT_S = 14           # above both supported relay points (8, 12), a partial last chunk under either


def split_wgs(nb):
    """Customer workgroups per chain of the split layout: a chain's 4 nb wave rows dealt six at a time
    (the plan rule restated; the level-2 workgroup comes on top)."""
    return -(-4 * nb // 6)


def _split_instance_case(K):
    """One case per compiled bivariate split instance (helper and relay).  N = 769: 4 blocks in 3
    workgroups — block 1 split with live lanes in both halves (its extension records are customers
    384..511); workgroup 1 with all six rows live, its relayed rows customers 640..767; workgroup 2 with
    one live lane, in block 3, and no block 4.  The state read between the launches forces the deferred
    level-2 draw through the flush kernel and gives a launch whose first sweep waits on a pending draw."""
    return dict(D=2, covs=[f"c{k}" for k in range(1, K)], data=("tiled", 769, K - 1), S=SPLIT_S, chains=2,
                chain_first=K % 2, seed=3300 + K, burnin=0, mcmc=3, thin=1,
                drive=[("run", 1), ("state",), ("run", 2)])


SPLIT_INSTANCE_CASES = {f"split_bi{K}": _split_instance_case(K) for K in range(1, 10)}
# customer ranges [lo, hi) the instance cases' power checks leave out (as GRID_CASES' drop)
SPLIT_INSTANCE_DROP = {"block 1's extension records": (BLOCK + 2 * ROW, 2 * BLOCK),
                       "workgroup 1's relayed rows": (10 * ROW, 12 * ROW)}


def _rows(b, first, n_rows=1):
    """Customers of rows [first, first + n_rows) of block b."""
    return (b * BLOCK + first * ROW, b * BLOCK + (first + n_rows) * ROW)


def _split_grid_case(K, n, layout, env, drop, seed, data="tiled", covs=None, chains=1, S=SPLIT_S):
    return dict(D=2, covs=[f"c{k}" for k in range(1, K)] if covs is None else covs,
                data=(data, n, K - 1 if covs is None else 0), S=S, chains=chains, chain_first=0, seed=seed,
                burnin=0, mcmc=2, thin=1, drive=[("run", 2)], layout=layout, env=env, drop=drop)


# layout: "split" / "block": what the handle must report; "choice": the default environment, where it must
# be what clv_debug_split_choice gives for the device's CU count.  env: the environment of the run.
_N129, _N256, _N257, _NC2 = 128 * BLOCK + 1, 255 * BLOCK + 1, 256 * BLOCK + 1, 23570
SPLIT_GRID_CASES = {
    # nb = 129: level-2 lanes in three wavefronts; block 127 (the only b % 3 == 1 at a wavefront's last
    # lane below 256) pairs with lane 126; a one-customer last block.  130 block workgroups do not
    # double up on 256 CUs, so the layout is forced.
    "sg_bi2_129": _split_grid_case(2, _N129, "split", {"CLV_PERSISTENT": "1", "CLV_PERSIST_LAYOUT": "split"},
                                   {"block 127 row 2": _rows(127, 2), "block 127 row 3": _rows(127, 3),
                                    "block 64 row 3": _rows(64, 3), "block 124 row 3": _rows(124, 3),
                                    "last block": (128 * BLOCK, _N129)}, 3401),
    # nb = SPLIT_MAX_NB: every level-2 lane holds a block, 171 + 1 physical workgroups, 256 + 170 records
    "sg_bi1_256": _split_grid_case(1, _N256, "choice", {},
                                   {"block 253 rows 2-3": _rows(253, 2, 2), "block 255 (one customer)": (255 * BLOCK, _N256),
                                    "block 0": (0, BLOCK)}, 3402),
    # nb = 257: the forced split layout is declined; lane 0 of the block layout's level-2 workgroup holds
    # blocks 0 and 256; customer 65,536 is the first large index
    "sg_bi1_257": _split_grid_case(1, _N257, "block", {"CLV_PERSIST_LAYOUT": "split"},
                                   {"block 0": (0, BLOCK), "block 256 (one customer)": (256 * BLOCK, _N257),
                                    "block 255": (255 * BLOCK, 256 * BLOCK)}, 3403),
    # the benchmark's own grid (c2): 4 x 63 workgroups on a 4-CU margin, chain-major
    "sg_c2": _split_grid_case(2, _NC2, "choice", {},
                              {"chain-last block": (92 * BLOCK, _NC2), "block 91 rows 2-3": _rows(91, 2, 2),
                               "block 64 row 3": _rows(64, 3)}, 42, data="full", covs=["first_sales_scaled"],
                              chains=4, S=20),
}


# ---------------------------------------------------------------------------------------------
# customers far from CDNOW (tests/helpers.edge_cbs; tests/test_gpu_edge_sweep.py): daily units, heavy
# buyers, long histories, spans of 0 and of 2^-40 T.  N = 385: two blocks and two split workgroups, the
# second of either with one live lane; S = 13: a partial last MH chunk.  Every sweep is stored.
# ---------------------------------------------------------------------------------------------
def _edge_case(D, K, n, S, chains, seed, drive):
    sweeps = sum(a[1] for a in drive if a[0] == "run")
    return dict(D=D, covs=[f"c{k}" for k in range(1, K)], data=("edge", n, K - 1), S=S, chains=chains, chain_first=0,
                seed=seed, burnin=0, mcmc=sweeps, thin=1, drive=drive)


EDGE_CASES = {
    "e_bi1": _edge_case(2, 1, 385, 20, 2, 20250101, [("run", 4), ("state",), ("run", 4)]),
    "e_bi2": _edge_case(2, 2, 385, 13, 1, 20250102, [("run", 6)]),
    "e_tri1": _edge_case(3, 1, 257, 20, 2, 20250103, [("run", 6)]),
}
# What the edge frame is for, per (chain, sweep, customer) lane, from the state (lambda, mu) entering the
# sweep, ml = lambda + mu: a churned draw with ml t_x >= 700 / with ml T >= 700 (tau's exponents on the
# cap, bi:223); ml (T - t_x) > 700 (P(alive)'s exponential on the kernel's cap); T == t_x (P(alive) = 1);
# a churned tau below t_x (both exponents capped: tau = 700 / ml, as the reference gives it); a state at
# +-70 after the sweep (a clipped proposal accepted and carried).  |log eta| > 70 is not among them: the
# conjugate draw's mean lies between the prior mean and log_s (|log_s| <= 14) and its standard deviation
# is below sqrt(omega2) ~ 11, so no frame within the prior reaches it — the kernel's |xe| <= 700 guard
# is exercised on its taken side only.
EDGE_EVENTS = ("cap_tx", "cap_T", "zz700", "span0", "tau_lt_tx", "clip_state")
CDNOW_EVENTS = COVERAGE_EVENTS
COVERAGE_EVENTS = CDNOW_EVENTS + EDGE_EVENTS
# near_T (a churned tau in the last 5% of [t_x, T]) is neither required nor forbidden: at these rates a
# churned tau sits at t_x, and the model's free runs show 0, 0 and 5 such lanes — the CDNOW cases hold it
EDGE_UNASSERTED = ("near_T",)
EDGE_COVERAGE = {name: tuple(e for e in COVERAGE_EVENTS if e not in EDGE_UNASSERTED) for name in EDGE_CASES}
EDGE_MIN_LANES = 10    # every event of EDGE_COVERAGE on at least this many lanes of a case's run


def edge_events(mp, lam, mu, z, tau, lam_after, mu_after):
    """Masks of EDGE_EVENTS for one (chain, sweep): (lam, mu) the state entering it, (z, tau) its draw,
    (lam_after, mu_after) the state it leaves (at the clip if within 1e-9 of +-70 on the log scale)."""
    ml = lam + mu
    churned = ~np.asarray(z, dtype=bool)
    at_clip = lambda v: np.abs(np.abs(np.log(v)) - CLIP) < 1e-9  # noqa: E731
    return dict(cap_tx=churned & (ml * mp.t_x >= 700.0), cap_T=churned & (ml * mp.T_cal >= 700.0),
                zz700=ml * (mp.T_cal - mp.t_x) > 700.0, span0=mp.T_cal == mp.t_x,
                tau_lt_tx=churned & (tau < mp.t_x), clip_state=at_clip(lam_after) | at_clip(mu_after))


ALL_CASES = {**CASES, **INSTANCE_CASES, **GRID_CASES, **SPLIT_INSTANCE_CASES, **SPLIT_GRID_CASES, **EDGE_CASES}


def case_frame(case):
    from tests.helpers import cdnow, cdnow_tiled, edge_cbs, with_covariates
    name, n, n_cov = case["data"]
    df = edge_cbs(n) if name == "edge" else cdnow_tiled(n) if name == "tiled" else cdnow(name, n)
    return with_covariates(df, n_cov) if n_cov else df


def n_sweeps_of(case):
    return sum(a[1] for a in case["drive"] if a[0] == "run")


def oracle_variates(seed, chain, sweep, n, S):
    """oracle.philox.sweep_variates in the form the model takes, cast as the device casts them: the
    accept threshold is log2 of the fp32 uniform, rounded to fp32."""
    v = oph.sweep_variates(seed, chain, sweep, n, S)
    v["log2_u"] = np.log2(v["u_acc"].astype(np.float64)).astype(np.float32)
    return v


def model_chain(mp: ModelProblem, seed, chain, n_sweeps, S, variates=oracle_variates):
    """The model run freely (its own state from sweep to sweep) in the reference's order — bi: level
    2 (the draw belonging to the sweep), then level 1; tri: level 1 with the previous draw (sweep 1:
    beta_0, gamma_00), then level 2.  Yields (sweep, level-1 dict, level-2 dict used / drawn)."""
    lam, mu = mp.lam0.copy(), mp.mu0.copy()
    beta, Sigma = mp.hyper["beta_0"], mp.hyper["gamma_00"].copy()
    for s in range(1, n_sweeps + 1):
        var = variates(seed, chain, s, mp.N, S)
        if mp.D == 2:
            l2 = mp.level2(seed, chain, s, np.column_stack([np.log(lam), np.log(mu)]))
            beta, Sigma = l2["beta"], l2["Sigma"]
        r = mp.level1(lam, mu, beta, Sigma, var)
        if mp.D == 3:
            l2 = mp.level2(seed, chain, s, np.column_stack([r["ll"], r["lm"], r["leta"]]))
            r["beta_in"], r["Sigma_in"] = beta, Sigma
            beta, Sigma = l2["beta"], l2["Sigma"]
        lam, mu = r["lam"], r["mu"]
        yield s, r, l2

"""CPU tests of tests/philox_sweep_ref.py, the float64 model the GPU module
(test_gpu_production_sweep.py) holds the production sweep to.  The model is the yardstick there, so
here it is pinned to the REFERENCE, never to the kernel:

* on G1 ``formulas.npz`` (the reference's recorded draw_z / draw_tau / log_posterior / draw_eta /
  _draw_level_2 inputs and outputs) it reproduces the outputs from the recorded variates: z exact;
  tau, the log posterior, eta, B_hat, S_n and Sigma <= 1e-12 relative; accept decisions equal
  exp(lp' - lp) > U wherever the model's own margin is clear; beta's noise factor F satisfies
  F F' = kron(Sigma, V) (the reference draws through numpy's SVD factor of the same covariance);
* a whole model sweep agrees with run_chain_bi / run_chain_tri sweep by sweep when both consume
  oracle.philox's variates (the oracle through a stub Stream), to the GPU module's tolerances;
* at every shape the GPU module uses, the share of (chain, sweep, customer) lanes whose decision
  margin is below the comparison tolerance stays within the 0.1% cap, and the level-2 tolerance
  covers ten times the measured sensitivity to the variates' and Y's documented uncertainty — for
  CASES, INSTANCE_CASES (every compiled (D, K)), GRID_CASES (up to 153,345 customers) and the split
  layout's SPLIT_INSTANCE_CASES / SPLIT_GRID_CASES (tests/test_gpu_split_model.py) alike, and for
  EDGE_CASES (tests/test_gpu_edge_sweep.py: customers far from CDNOW), which also run whole against the
  oracle's chain and whose coverage table (EDGE_COVERAGE: capped tau exponents, tau below t_x, T == t_x,
  states carried at the +-70 clip) is exactly what the model's free run produces, no lane borderline;
* the coverage events the GPU module asserts per instance case (INSTANCE_COVERAGE) are exactly those
  the model's free run of the case produces;
* at the grid cases' sizes numpy's mean of the likelihood terms and the exactly rounded one differ by
  at most a tenth of the log-likelihood's comparison tolerance.
"""
import math

import numpy as np
import pytest

from oracle import ref_cpu as orc
from tests import philox_sweep_ref as M
from tests.helpers import golden


@pytest.fixture(scope="module")
def F():
    return golden("formulas.npz")


def test_z_and_tau_reproduce_the_reference(F):
    n = F["z_u"].size
    v = F["tau_v"]  # the variate each customer consumed: E if alive, U if churned
    u = np.where(F["z_out"], 0.5, v)
    z, tau, margin = M.draw_z_tau(F["z_tx"], F["z_T"], F["z_lam"], F["z_mu"], F["z_u"], u, v)
    assert np.array_equal(z, F["z_out"])
    assert 0.1 * n < z.sum() < 0.9 * n
    np.testing.assert_allclose(tau, F["tau_out"], rtol=1e-12, atol=0)
    assert (margin > M.RTOL).all()
    # the margin is |u - p| relative to the two sides' size: zero exactly on the threshold
    p = F["z_p"]
    ok = (p > 0) & (p < 1)
    _, _, m0 = M.draw_z_tau(F["z_tx"][ok], F["z_T"][ok], F["z_lam"][ok], F["z_mu"][ok], p[ok], u[ok], v[ok])
    assert (m0 <= 4e-16).all()
    # the wrong pairing of the tau variate with the branches (the GPU module's power check) moves tau
    _, tau_sw, _ = M.draw_z_tau(F["z_tx"], F["z_T"], F["z_lam"], F["z_mu"], F["z_u"], np.full(n, 0.5), v,
                                swap_tau_branch=True)
    assert (~np.isclose(tau_sw, tau, rtol=1e-6, atol=0)).mean() > 0.9


def test_log_posterior_and_accepts_reproduce_the_reference(F):
    n = F["lp_ll"].size
    rng = np.random.default_rng(2024)
    S = F["lp_S"]
    P = np.linalg.inv(S)
    t3 = rng.standard_t(3, (2, 1, n)).astype(np.float32)
    x, z, T, tau, mv = F["lp_x"], F["lp_z"], F["lp_T"], F["lp_tau"], F["lp_mv"]
    ll, lm = F["lp_ll"], F["lp_lm"]
    pl = np.clip(ll + S[0, 0] * t3[0, 0].astype(np.float64), -70, 70)
    pm = np.clip(lm + S[1, 1] * t3[1, 0].astype(np.float64), -70, 70)
    with np.errstate(over="ignore", invalid="ignore"):
        lp_cur = orc.log_posterior(ll, lm, x, z, T, tau, mv, P)
        d_ref = orc.log_posterior(pl, pm, x, z, T, tau, mv, P) - lp_cur
    # log U: half the lanes close to the threshold, half uniform; as the device forms it (fp32 log2)
    lu = np.log(rng.random(n))
    near = (rng.random(n) < 0.5) & np.isfinite(d_ref) & (np.abs(d_ref) < 50)
    lu[near] = np.minimum(d_ref[near], 0.0) + rng.choice([-1, 1], near.sum()) * 10.0 ** rng.uniform(-6, -1, near.sum())
    log2_u = np.minimum(lu / M.LN2, -1e-30).astype(np.float32)
    U = np.exp(M.LN2 * log2_u.astype(np.float64))
    steps = []
    nl, nm, cur, margin, hit_clip, hit_cap = M.mh_steps(x, T, z, tau, mv, P, S[0, 0], S[1, 1], ll, lm,
                                                        t3[0], t3[1], log2_u[None], steps)
    st = steps[0]
    # the log posterior (bi:291-310), -inf above the cap included
    np.testing.assert_allclose(st["cur"], F["lp_out"], rtol=1e-12, atol=0)
    assert np.isneginf(st["cur"][lm > 5]).all() and (lm > 5).sum() > 0
    with np.errstate(over="ignore", invalid="ignore"):
        acc_ref = np.exp(d_ref) > U  # bi:329-330
    clear = margin > M.RTOL
    assert clear.mean() > 0.95
    assert np.array_equal(st["accept"][clear], acc_ref[clear])
    assert 0.05 * n < st["accept"].sum() < 0.95 * n
    assert hit_cap.any() and not st["accept"][pm > 5].any()
    assert hit_clip.any()
    both_inf = (lm > 5) & (pm > 5)
    assert both_inf.any() and not st["accept"][both_inf].any()       # NaN ratio: reject
    from_inf = (lm > 5) & (pm <= 5)
    assert from_inf.any() and st["accept"][from_inf].all()           # +inf ratio: accept
    assert np.array_equal(nl[st["accept"]], pl[st["accept"]]) and np.array_equal(nl[~st["accept"]], ll[~st["accept"]])


def test_eta_reproduces_the_reference(F):
    X = F["eta_X"]
    n = X.shape[0]
    var = dict(u_z=np.full(n, 0.5), u_tau=np.full(n, 0.5), e_alive=np.ones(n), eta_z=F["eta_z"],
               t_l=np.zeros((0, n), np.float32), t_m=np.zeros((0, n), np.float32), log2_u=np.zeros((0, n), np.float32))
    r = M.sweep_level1(np.ones(n), np.ones(n), np.full(n, 30.0), X, np.full(n, 0.1), np.full(n, 0.1),
                       F["eta_beta"], F["eta_Sigma"], var, log_s=F["eta_log_s"], omega2=float(F["eta_omega2"]))
    np.testing.assert_allclose(r["leta"], F["eta_out"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["eta"], np.exp(F["eta_out"]), rtol=1e-12, atol=0)
    # S = 0: the state passes through log / exp unchanged to rounding
    np.testing.assert_allclose(r["lam"], 0.1, rtol=1e-15)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 9])
def test_level2_reproduces_the_reference(F, D, K):
    p = f"l2_D{D}_K{K}_"
    hyper = orc.default_hyper(K, D)
    hyper["beta_0"] = F[p + "B0"]
    r = M.level2_draw(F[p + "X"], F[p + "Y"], hyper, F[p + "iw_normal"], F[p + "iw_chi2"], F[p + "mvn_z"])
    np.testing.assert_allclose(r["B_hat"], F[p + "Bhat"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["S_n"], F[p + "Sn"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["Sigma"], F[p + "Sigma"], rtol=1e-12, atol=0)
    assert r["nu_n"] == int(F[p + "nun"])
    cov = np.kron(F[p + "Sigma"], F[p + "V"])  # the covariance the reference draws beta's noise from
    np.testing.assert_allclose(r["factor"] @ r["factor"].T, cov, rtol=0, atol=1e-12 * np.abs(cov).max())
    w = np.kron(np.linalg.cholesky(F[p + "Sigma"]), np.linalg.cholesky(F[p + "V"])) @ F[p + "mvn_z"]
    np.testing.assert_allclose(r["beta"], (F[p + "Bhat"].ravel() + w).reshape(K, D), rtol=1e-10, atol=1e-12)
    row = M.l2_record(r["beta"], r["Sigma"])
    b2, s2 = M.l2_unpack(row, D, K)
    assert np.array_equal(b2, r["beta"]) and np.allclose(s2, r["Sigma"], rtol=1e-15)


# ---------------------------------------------------------------------------------------------
class PhiloxStream(orc.Stream):
    """Hands the oracle oracle.philox's variates of (seed, chain) in the reference's consumption order.
    ``z_of`` (sweep -> alive mask) scatters the per-customer tau variate as draw_tau consumes it."""

    def __init__(self, mp, seed, chain, S, z_of):
        super().__init__(None, record=True)
        self.mp, self.seed, self.chain, self.S, self.z_of, self.s = mp, seed, chain, S, z_of, 0

    def begin_sweep(self):
        super().begin_sweep()
        self.s += 1
        self.var = M.oracle_variates(self.seed, self.chain, self.s, self.mp.N, self.S)
        self.step = dict(t_l=0, t_m=0, u_acc=0)
        self.hv = M.hyper_variates(self.seed, self.chain, self.s, self.mp.D, self.mp.K, self.mp.nu_n)

    def random(self, n, key):
        v = self.var["u_z"] if key == "u_z" else self.var["u_tau"][~self.z_of[self.s]]
        assert v.shape[0] == n
        return self._rec(key, v)

    def standard_exponential(self, n, key):
        v = self.var["e_alive"][self.z_of[self.s]]
        assert v.shape[0] == n
        return self._rec(key, v)

    def standard_t3(self, n, key):
        j = self.step[key]
        self.step[key] += 1
        return self._rec(key, self.var[key][j].astype(np.float64), append=True)

    def random_step(self, n, key):
        j = self.step[key]
        self.step[key] += 1
        return self._rec(key, np.exp2(self.var["log2_u"][j].astype(np.float64)), append=True)

    def standard_normal(self, n, key):
        return self._rec(key, self.var["eta_z"])

    def bartlett(self, dim, df):
        assert dim == self.mp.D and df == self.mp.nu_n
        self._rec("iw_normal", self.hv[0])
        self._rec("iw_chi2", self.hv[1])
        return self.hv[0], self.hv[1]

    def mvn_noise(self, cov):
        return self._rec("mvn_noise", np.linalg.cholesky(cov) @ self.hv[2])


@pytest.mark.parametrize("name", ["bi_k2", "tri_k3"] + list(M.EDGE_CASES))
def test_model_sweep_agrees_with_the_oracle_chain(name):
    """The edge cases run whole (385 / 257 customers): the oracle's chain passes through the capped tau
    exponents, tau = 700 / ml below t_x, T == t_x and states carried at the +-70 clip, and the model
    must follow it there to the same tolerances."""
    case = M.ALL_CASES[name]
    mp = M.ModelProblem(M.case_frame(case).iloc[:None if name in M.EDGE_CASES else 300], case["covs"], case["D"])
    seed, chain, S, T = case["seed"], 1, case["S"], 3
    free = {s: (r, l2) for s, r, l2 in M.model_chain(mp, seed, chain, T, S)}
    st = PhiloxStream(mp, seed, chain, S, {s: free[s][0]["z"] for s in free})
    hyper = orc.default_hyper(mp.K, mp.D)
    kw = dict(mcmc=1, burnin=10, thin=1, stream=st, trace=0, n_mh_steps=S, n_sweeps=T)  # nothing stored: no Q5 trip
    if mp.D == 2:
        orc.run_chain_bi(1, mp.x, mp.t_x, mp.T_cal, mp.X, hyper, **kw)
    else:
        orc.run_chain_tri(1, mp.x, mp.t_x, mp.T_cal, mp.log_s, mp.X, hyper, omega2=mp.omega2,
                          log_s_mean=mp.hyper["beta_0"][0, 2], **kw)
    lam, mu = mp.lam0, mp.mu0
    set_aside = 0
    for s in range(1, T + 1):
        t = st.tape[s - 1]
        beta, Sigma = (t["beta"], t["Sigma"]) if mp.D == 2 else (t["beta_in"], t["Sigma_in"])
        r = mp.level1(lam, mu, beta, Sigma, M.oracle_variates(seed, chain, s, mp.N, S))  # teacher forced
        clear = r["margin"] > M.RTOL
        set_aside += (~clear).sum()
        assert np.array_equal(r["z"][clear], t["z"][clear])
        np.testing.assert_allclose(r["tau"][clear], t["tau"][clear], rtol=M.RTOL, atol=0)
        np.testing.assert_allclose(r["lam"][clear], t["lam"][clear], rtol=M.RTOL, atol=0)
        np.testing.assert_allclose(r["mu"][clear], t["mu"][clear], rtol=M.RTOL, atol=0)
        np.testing.assert_allclose(r["lik"][clear], orc.lik_terms(mp.x, mp.T_cal, t["lam"], t["mu"], t["z"], t["tau"])[clear],
                                   rtol=M.RTOL, atol=0)
        if mp.D == 3:
            np.testing.assert_allclose(r["eta"][clear], t["eta"][clear], rtol=M.RTOL, atol=0)
            Y = np.log(np.column_stack([t["lam"], t["mu"], t["eta"]]))
        else:
            Y = np.log(np.column_stack([lam, mu]))
        l2 = mp.level2(seed, chain, s, Y)
        np.testing.assert_allclose(l2["beta"], t["beta"], rtol=M.L2_RTOL, atol=M.L2_ATOL)
        np.testing.assert_allclose(l2["Sigma"], t["Sigma"], rtol=M.L2_RTOL, atol=M.L2_ATOL)
        lam, mu = t["lam"], t["mu"]
    assert set_aside <= M.BORDERLINE_CAP * T * mp.N
    assert (mp.t_x == 0).any() and any((~free[s][0]["z"]).any() for s in free)


# ---------------------------------------------------------------------------------------------
class _FreeRuns(dict):
    """Every GPU case's chains run freely through the model with oracle.philox's variates (on first use)."""

    def __missing__(self, name):
        case = M.ALL_CASES[name]
        mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
        assert mp.N == case["data"][1]
        self[name] = (mp, {c: list(M.model_chain(mp, case["seed"], case["chain_first"] + c, M.n_sweeps_of(case), case["S"]))
                           for c in range(case["chains"])})
        return self[name]


@pytest.fixture(scope="module")
def free_runs():
    return _FreeRuns()


def coverage_of(mp, chains, edge=False):
    """Lanes of each coverage event (philox_sweep_ref.COVERAGE_EVENTS) over a case's free run;
    ``edge``: the events of EDGE_EVENTS too (counted for the edge cases only)."""
    n = dict.fromkeys(M.COVERAGE_EVENTS if edge else M.CDNOW_EVENTS, 0)
    for runs in chains.values():
        lam, mu = mp.lam0, mp.mu0
        for s, r, _ in runs:
            if edge:
                for k, v in M.edge_events(mp, lam, mu, r["z"], r["tau"], r["lam"], r["mu"]).items():
                    n[k] += int(v.sum())
                lam, mu = r["lam"], r["mu"]
            edges = M.near_edges(mp, r["z"], r["tau"])
            n["x0"] += int(((mp.x == 0) & (mp.t_x == 0)).sum())
            n["near_tx"] += int(edges[0].sum())
            n["near_T"] += int(edges[1].sum())
            n["clip"] += int(r["hit_clip"].sum())
            n["cap"] += int(r["hit_cap"].sum())
    return n


@pytest.mark.parametrize("name", list(M.ALL_CASES))
def test_borderline_share_is_within_the_cap(free_runs, name):
    """The cap is a condition on the model alone: no device involved."""
    mp, chains = free_runs[name]
    lanes = border = clip = cap = near_tx = near_T = 0
    for runs in chains.values():
        for s, r, _ in runs:
            lanes += mp.N
            border += (r["margin"] <= M.RTOL).sum()
            clip += r["hit_clip"].sum()
            cap += r["hit_cap"].sum()
            near_tx += M.near_edges(mp, r["z"], r["tau"])[0].sum()
            near_T += M.near_edges(mp, r["z"], r["tau"])[1].sum()
    share = border / lanes
    print(f"{name}: {lanes} lanes, borderline {border} ({100 * share:.4f}%), clip lanes {clip}, cap lanes {cap}, "
          f"churned tau near t_x {near_tx}, near T {near_T}, x = 0 customers {(mp.x == 0).sum()}")
    assert share <= M.BORDERLINE_CAP
    # the edge frame's churned draws sit at t_x (ml (T - t_x) is large): its own coverage table is
    # asserted by test_edge_coverage_table_is_what_the_model_produces
    assert (mp.x == 0).any() and near_tx > 0 and (near_T > 0 or name in M.EDGE_CASES)
    if name in M.EDGE_CASES:  # measured: no lane of 6,160 / 2,310 / 3,084 is borderline
        assert border == 0


@pytest.mark.parametrize("name", list(M.ALL_CASES))
def test_level2_tolerance_covers_the_measured_sensitivity(free_runs, name):
    """The hyper variates are pinned to <= 1e-12 relative (test_device_hyper_variates_match_oracle) and
    the device's Y is the log-scale state, within 2 ulp of log of the stored natural-scale one: the
    level-2 tolerance must cover ten times what those move beta and Sigma at this shape.  The edge cases
    (Sigma11 up to 1,200, Y from -70 to 19) measure 1.1e-12 (e_bi1), 2.4e-12 (e_bi2) and 3.1e-12
    (e_tri1) beyond the absolute term: ten times that is 3.1e-11, so L2_RTOL = 1e-10 holds for them too
    and they get no tolerance of their own."""
    mp, chains = free_runs[name]
    case = M.ALL_CASES[name]
    rng = np.random.default_rng(1)
    worst = raw = 0.0
    runs = chains[0]
    for s, r, l2 in runs[:3]:
        hs = s
        if mp.D == 2:
            prev = runs[s - 2][1] if s > 1 else None
            Y = np.log(np.column_stack([mp.lam0, mp.mu0])) if prev is None else np.column_stack([prev["ll"], prev["lm"]])
        else:
            Y = np.column_stack([r["ll"], r["lm"], r["leta"]])
        hv = M.hyper_variates(case["seed"], case["chain_first"], hs, mp.D, mp.K, mp.nu_n)
        base = M.level2_draw(mp.X, Y, mp.hyper, *hv)
        for _ in range(8):
            hv2 = [v * (1 + 1e-12 * rng.choice([-1, 1], v.shape)) for v in hv]
            Y2 = Y + 2 * np.spacing(Y) * rng.choice([-1, 1], Y.shape)
            got = M.level2_draw(mp.X, Y2, mp.hyper, *hv2)
            for k in ("beta", "Sigma"):
                worst = max(worst, M.l2_deviation(got[k], base[k]).max())
                raw = max(raw, (np.abs(got[k] - base[k]) / np.abs(base[k])).max())
    print(f"{name}: level-2 sensitivity {worst:.3e} beyond atol {M.L2_ATOL:.0e} (elementwise relative, no atol: "
          f"{raw:.3e}; tolerance {M.L2_RTOL:.1e})")
    assert 10 * worst <= M.L2_RTOL


@pytest.mark.parametrize("name", list(M.INSTANCE_CASES))
def test_instance_coverage_table_is_what_the_model_produces(free_runs, name):
    """philox_sweep_ref.INSTANCE_COVERAGE, which the GPU module asserts per case, is exactly the set of
    coverage events the model's free run of the case produces."""
    mp, chains = free_runs[name]
    n = coverage_of(mp, chains)
    print(f"{name}: N {mp.N}, coverage lanes " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert {k for k, v in n.items() if v > 0} == set(M.INSTANCE_COVERAGE[name])


@pytest.mark.parametrize("name", list(M.EDGE_CASES))
def test_edge_coverage_table_is_what_the_model_produces(free_runs, name):
    """philox_sweep_ref.EDGE_COVERAGE, which tests/test_gpu_edge_sweep.py asserts per case from the
    device's own state, is exactly the set of events the model's free run of the case produces, each
    on at least EDGE_MIN_LANES lanes (near_T aside: EDGE_UNASSERTED).  Measured, (chain, sweep,
    customer) lanes of e_bi1 (6,160) / e_bi2 (2,310) / e_tri1 (3,084): x0 784 / 294 / 396, near_tx
    2544 / 970 / 1263, near_T 0 / 0 / 5, clip 5600 / 1997 / 2587, cap 6133 / 2281 / 2987, cap_tx 320 /
    95 / 320, cap_T 1143 / 352 / 798, zz700 1078 / 339 / 734, span0 768 / 288 / 384, tau_lt_tx 320 /
    95 / 320, clip_state 3212 / 979 / 289; lambda ends in [5.4e-8, 1.5e8] / [0.11, 31] / [6.1e-9,
    2.5e10], mu in [e^-70, 141] / [e^-70, 134] / [e^-70, 126]; everything finite."""
    mp, chains = free_runs[name]
    n = coverage_of(mp, chains, edge=True)
    print(f"{name}: N {mp.N}, coverage lanes " + ", ".join(f"{k} {v}" for k, v in n.items()))
    for runs in chains.values():
        for s, r, _ in runs:
            assert all(np.isfinite(r[k]).all() for k in ("tau", "lam", "mu", "lik"))
    assert {k for k, v in n.items() if v > 0} - set(M.EDGE_UNASSERTED) == set(M.EDGE_COVERAGE[name])
    assert min(n[k] for k in M.EDGE_COVERAGE[name]) >= M.EDGE_MIN_LANES


@pytest.mark.parametrize("name", list(M.GRID_CASES) + list(M.SPLIT_GRID_CASES))
def test_loglik_mean_does_not_depend_on_the_summation_order(free_runs, name):
    """The stored log-likelihood is a mean over up to 153,345 terms, summed on the device per block, per
    unit and over the units.  numpy's pairwise mean of the model's terms, which the GPU module compares
    it with at RTOL, and the exactly rounded mean (math.fsum) differ by at most a tenth of RTOL."""
    mp, chains = free_runs[name]
    worst = 0.0
    for runs in chains.values():
        for s, r, _ in runs:
            exact = math.fsum(r["lik"]) / mp.N
            worst = max(worst, abs(r["lik"].mean() - exact) / abs(exact))
    print(f"{name}: {mp.N} terms, numpy mean against fsum mean {worst:.2e} relative (a tenth of RTOL: {0.1 * M.RTOL:.0e})")
    assert worst <= 0.1 * M.RTOL

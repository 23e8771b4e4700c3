"""Scoring customers outside the fit (csrc/score.hip, kernels.hip score_kernel) on the device, against
the float64 model of tests/score_ref.py, through the Python API and the debug ABI only.

Value by value (test_score_matches_model, the procedure of tests/test_gpu_production_sweep.py).  The
device is driven one record at a time — n_draws = 1, warmup = 0, init = the device's previous state,
sweep_first advancing — so a borderline flip cannot cascade (teacher forcing); the model runs from
the same state with the device's own variates (clv_debug_variates at the global customer indices).
z is compared exactly; lambda, mu, eta at philox_sweep_ref.RTOL = 1e-12; tau at RTOL plus
tau_atol(lambda, mu) of the state entering the recorded sweep; P, s00, s11 of the prepare kernel
(clv_debug_score_hyper) against inv_sigma_block at L2_RTOL / L2_ATOL — the project's figures, derived
in tests/test_gpu_production_sweep.py's header.  A lane whose model decision margin is <= RTOL at
any inner sweep of a call is set aside for that call; at most BORDERLINE_CAP = 0.1% of lanes per
case (tests/test_score_cpu.py asserts the model alone meets it at these shapes: none).  Each case
asserts the coverage events of score_ref.COVERAGE among its compared lanes: a mu-cap hit, a clip
hit, both z outcomes (bi1_s0 runs no MH step, so nothing is proposed there: z only).
Power: the same device outputs against the model with one thing wrong at a time — the next sweep's
variates, chain key + 1, the next record's (beta, Sigma) (not for S = 0 bivariate, where the record
does not enter a level-1 sweep at all), customer_offset off by one — each must fail more than half
the customers.

Whole-call identities, bit for bit, and the target distribution: see the tests' docstrings.

Measured on the MI355X: no lane set aside in any case; largest relative deviations lambda 4.2e-15, mu
5.4e-15, tau 4.0e-15, eta 1.9e-15; the prepare kernel's P, s00, s11 within the absolute term; every
power check fails every customer; distribution, largest |mean - quadrature| / MCSE: 2.4 / 2.3 / 2.7
(log lambda / log mu / P(alive), bivariate K = 2) and 3.5 / 2.3 / 2.6 (trivariate K = 3).  The module
takes about 5 s.
"""
import ctypes

import numpy as np
import pytest

from tests import philox_sweep_ref as M
from tests import score_ref as R
from tests.helpers import bits, cdnow, cdnow_tiled, with_covariates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _device_variates(L, seed, chain, sweep, first, n, S):
    """The kernels' own variates of one (chain, inner sweep) for customers first .. first + n - 1."""
    m = first + n
    tl, tm, ua, l2u = (np.zeros(max(m * S, 1), np.float32) for _ in range(4))
    uz, ut, ea, ez = (np.zeros(m) for _ in range(4))
    assert L.clv_debug_variates(seed, chain, sweep, m, S, _fp(tl), _fp(tm), _fp(ua), _dp(uz), _dp(ut), _dp(ea), _dp(ez),
                                _fp(l2u)) == 0
    sh = lambda a: a[: m * S].reshape(S, m)[:, first:]  # noqa: E731
    return dict(u_z=uz[first:], u_tau=ut[first:], e_alive=ea[first:], eta_z=ez[first:], t_l=sh(tl), t_m=sh(tm),
                log2_u=sh(l2u))


def _score(sp, level2, case, **kw):
    from mcmc_clv_model_amd import score_customers
    args = dict(inner_sweeps=case["R"], warmup=0, n_mh_steps=case["S"], seed=case["seed"], omega2=sp.omega2,
                customer_offset=case["offset"], chain_first=case["chain_first"])
    args.update(kw)
    return score_customers({"level_2": list(level2)}, sp.df, sp.covs, **args)


class Driven:
    """A case driven record by record on the device: the state entering every record, the recorded
    draws and the device's variates of every inner sweep."""

    def __init__(self, L, name):
        self.case = case = R.CASES[name]
        self.sp = sp = R.case_problem(case)
        self.l2 = l2 = R.case_level2(case)
        C, nd = case["chains"], case["records"]
        self.C, self.nd = C, nd
        lam, mu = R.default_init(l2, sp.X, sp.D, sp.K)
        self.enter, self.first_t = [], []
        self.l1 = np.empty((C, nd, sp.N, sp.D + 2))
        t = 1
        for d in range(nd):
            self.enter.append((lam, mu))
            self.first_t.append(t)
            out = _score(sp, l2[:, d:d + 1], case, init=(lam, mu), sweep_first=t)
            self.l1[:, d] = np.stack(out["level_1"])[:, 0]
            lam, mu = out["state"]["lam"], out["state"]["mu"]
            assert out["state"]["next_sweep"] == t + case["R"]
            t = out["state"]["next_sweep"]
        self.final = (lam, mu)
        self.n_sweeps = t - 1
        cf, off, S, n = case["chain_first"], case["offset"], case["S"], sp.N
        # one customer more on either side (the offset power check) and one sweep beyond the run
        lo = max(off - 1, 0)
        self.var_lo = lo
        self.var = {(c, s): _device_variates(L, case["seed"], cf + c, s, lo, off - lo + n + 1, S)
                    for c in range(C) for s in range(1, self.n_sweeps + 2)}
        self.var_next_key = {s: _device_variates(L, case["seed"], cf + 1, s, lo, off - lo + n + 1, S)
                             for s in range(1, self.n_sweeps + 1)}

    def variates(self, table, key, shift=0):
        """The variates of ``key`` for this case's customers, ``shift`` customers further on."""
        v = table[key]
        a = self.case["offset"] - self.var_lo + shift
        return {k: x[..., a:a + self.sp.N] for k, x in v.items()}


_DRIVEN = {}


def driven(L, name):
    if name not in _DRIVEN:
        _DRIVEN[name] = Driven(L, name)
    return _DRIVEN[name]


def _close(got, ref, atol=0.0):
    return np.abs(got - ref) <= M.RTOL * np.abs(ref) + atol


def compare(dev, chains, var_of=None, record_shift=0):
    """Model against device.  Returns dict(fail (chain, customer) mask, lanes, set_aside, the largest
    relative deviations, the coverage counts among the compared lanes)."""
    sp, case = dev.sp, dev.case
    var_of = var_of or (lambda c, s: dev.variates(dev.var, (c, s)))
    out = dict(fail=np.zeros((len(chains), sp.N), bool), lanes=0, set_aside=0, lam=0.0, mu=0.0, tau=0.0, eta=0.0,
               hit_cap=0, hit_clip=0, z0=0, z1=0)
    for ci, c in enumerate(chains):
        for d in range(dev.nd):
            rec = min(d + record_shift, dev.nd - 1) if record_shift else d
            if record_shift and rec == d:
                continue  # (the last record has no next one)
            lam, mu = dev.enter[d][0][c], dev.enter[d][1][c]
            r = R.run_chain(sp, dev.l2[c, rec:rec + 1], lam, mu, seed=case["seed"], chain=c, S=case["S"], inner=case["R"],
                            sweep_first=dev.first_t[d], variates=var_of)
            ref, got = r["level1"][0], dev.l1[c, d]
            clear = r["margin"] > M.RTOL
            out["lanes"] += sp.N
            out["set_aside"] += int((~clear).sum())
            assert np.isin(got[:, 3], (0.0, 1.0)).all()
            bad = got[:, 3] != ref[:, 3]
            bad |= ~_close(got[:, 0], ref[:, 0]) | ~_close(got[:, 1], ref[:, 1])
            bad |= ~_close(got[:, 2], ref[:, 2], M.tau_atol(r["lam_in"], r["mu_in"]))
            if sp.D == 3:
                bad |= ~_close(got[:, 4], ref[:, 4])
            nxt = dev.enter[d + 1] if d + 1 < dev.nd else dev.final  # the state written = the recorded draw
            bad |= (bits(nxt[0][c]) != bits(got[:, 0])) | (bits(nxt[1][c]) != bits(got[:, 1]))
            out["fail"][ci] |= bad & clear
            for k, col in (("lam", 0), ("mu", 1), ("tau", 2)) + ((("eta", 4),) if sp.D == 3 else ()):
                if clear.any():
                    out[k] = max(out[k], float((np.abs(got[:, col] - ref[:, col]) / np.abs(ref[:, col]))[clear].max()))
            for k in ("hit_cap", "hit_clip", "z0", "z1"):
                out[k] += int((clear & r[k]).sum())
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_score_matches_model(L, name):
    dev = driven(L, name)
    case, sp = dev.case, dev.sp
    r = compare(dev, range(dev.C))
    print(f"{name}: {dev.nd} records x {dev.C} chains x R = {case['R']}, {r['lanes']} lanes compared, {r['set_aside']} set "
          f"aside; largest relative deviation lambda {r['lam']:.2e} mu {r['mu']:.2e} tau {r['tau']:.2e} eta {r['eta']:.2e}; "
          f"cap lanes {r['hit_cap']}, clip lanes {r['hit_clip']}, churned {r['z0']}, alive {r['z1']}")
    assert r["lanes"] == dev.nd * dev.C * sp.N
    assert r["set_aside"] <= M.BORDERLINE_CAP * r["lanes"]
    assert not r["fail"].any(), f"{r['fail'].sum()} (chain, customer) lanes differ from the model"
    for ev in R.COVERAGE[name]:
        assert r[ev] > 0, ev

    # ---- the prepare kernel: P, s00, s11 (and the eta constants) of every record
    from mcmc_clv_model_amd import _lib
    recs = np.ascontiguousarray(dev.l2.reshape(-1, dev.l2.shape[-1]))
    H = np.empty((recs.shape[0], 64))
    _lib.check(L.clv_debug_score_hyper(-1, sp.D, sp.K, recs.shape[0], _dp(recs), sp.omega2 or 1.0, _dp(H)))
    worst = 0.0
    for row, h in zip(recs, H):
        beta, Sigma = M.l2_unpack(row, sp.D, sp.K)
        P = M.inv_sigma_block(Sigma)
        worst = max(worst, float(M.l2_deviation(h[36:39], [P[0, 0], P[0, 1], P[1, 1]]).max()))
        assert bits(h[39]) == bits(Sigma[0, 0]) and bits(h[40]) == bits(Sigma[1, 1])
        assert np.array_equal(bits(h[:sp.K * sp.D]), bits(beta.ravel()))
        if sp.D == 3:
            pv = 1.0 / (1.0 / sp.omega2 + 1.0 / Sigma[2, 2])
            worst = max(worst, float(M.l2_deviation(h[42:44], [pv, np.sqrt(pv)]).max()))
    print(f"{name}: prepare kernel, largest deviation beyond the absolute term {worst:.2e}")
    assert worst <= M.L2_RTOL

    # ---- power: one thing wrong at a time on the model's side, same device outputs, chain 0
    shares = dict(next_sweep=compare(dev, [0], var_of=lambda c, s: dev.variates(dev.var, (c, s + 1)))["fail"].mean(),
                  next_chain_key=compare(dev, [0], var_of=lambda c, s: dev.variates(dev.var_next_key, s))["fail"].mean(),
                  offset_plus_one=compare(dev, [0], var_of=lambda c, s: dev.variates(dev.var, (c, s), shift=1))["fail"].mean())
    if case["S"] > 0 or case["D"] == 3:
        shares["next_record"] = compare(dev, [0], record_shift=1)["fail"].mean()
    print(f"{name}: power, share of customers failing: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v > 0.5, (k, v)


# ---------------------------------------------------------------------------------------------
# whole-call identities, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bi2", "bi5", "tri3"])
def test_one_call_equals_record_by_record(L, name):
    """One call over all records = the record-by-record continuation of test_score_matches_model."""
    dev = driven(L, name)
    lam0, mu0 = dev.enter[0]
    out = _score(dev.sp, dev.l2, dev.case, init=(lam0, mu0), sweep_first=1)
    assert np.array_equal(bits(np.stack(out["level_1"])), bits(dev.l1))
    assert np.array_equal(bits(out["state"]["lam"]), bits(dev.final[0]))
    assert np.array_equal(bits(out["state"]["mu"]), bits(dev.final[1]))
    # the default start state is exp(x' beta_{c,0}) per customer; warm-up sweeps move the counter on
    from mcmc_clv_model_amd import analysis as A
    sp = dev.sp
    cov = np.ascontiguousarray(sp.X[:, 1:].T) if sp.K > 1 else None
    init = A.score_init(dev.l2, sp.D, sp.K, cov, sp.N, None)
    np.testing.assert_allclose(init[0], lam0, rtol=1e-14)
    np.testing.assert_allclose(init[1], mu0, rtol=1e-14)
    dflt, expl = _score(sp, dev.l2, dev.case), _score(sp, dev.l2, dev.case, init=init)
    assert np.array_equal(bits(np.stack(dflt["level_1"])), bits(np.stack(expl["level_1"])))
    warm = _score(dev.sp, dev.l2, dev.case, warmup=3)
    assert warm["state"]["next_sweep"] == out["state"]["next_sweep"] + 3
    assert not np.array_equal(bits(np.stack(warm["level_1"])), bits(dev.l1))
    wu = _score(dev.sp, dev.l2[:, :1], dev.case, inner_sweeps=3, warmup=0)      # 3 sweeps against record 0 ...
    cont = _score(dev.sp, dev.l2, dev.case, init=(wu["state"]["lam"], wu["state"]["mu"]), sweep_first=4)
    assert np.array_equal(bits(np.stack(cont["level_1"])), bits(np.stack(warm["level_1"])))  # ... are the warm-up


def test_customer_batches_do_not_matter(L):
    """N = 600 in one call = the halves with customer_offset 0 and 300."""
    dev = driven(L, "bi9")
    sp, case = dev.sp, dev.case
    whole = _score(sp, dev.l2, case, warmup=2)
    for lo in (0, 300):
        half = R.ScoreProblem(sp.df.iloc[lo:lo + 300].reset_index(drop=True), sp.covs, sp.D)
        part = _score(half, dev.l2, case, warmup=2, customer_offset=lo)
        assert np.array_equal(bits(np.stack(part["level_1"])), bits(np.stack(whole["level_1"])[:, :, lo:lo + 300]))
        assert np.array_equal(bits(part["state"]["mu"]), bits(whole["state"]["mu"][:, lo:lo + 300]))


def test_chains_do_not_matter(L):
    """Chains {0, 1, 2} in one call = three single-chain calls with chain_first 0, 1, 2."""
    dev = driven(L, "bi2")
    whole = _score(dev.sp, dev.l2, dev.case, warmup=2)
    for c in range(3):
        one = _score(dev.sp, dev.l2[c:c + 1], dev.case, warmup=2, chain_first=c)
        assert np.array_equal(bits(one["level_1"][0]), bits(whole["level_1"][c]))
        assert np.array_equal(bits(one["state"]["lam"][0]), bits(whole["state"]["lam"][c]))


@pytest.mark.parametrize("D,K", [(2, 2), (3, 3)])
def test_summary_sink_sums_the_full_sinks_draws(L, D, K):
    """sink="summary" = the sequential float64 sums, in record order, of what sink="full" records:
    N = 257, 2 chains, 50 records.  The log sums are the device's own log (clv_debug_log) of the
    recorded natural-scale draws."""
    from mcmc_clv_model_amd import _lib
    case = dict(R.CASES["tri3"], D=D, K=K, records=50, R=2, covs=[f"c{k}" for k in range(1, K)], seed=77)
    sp, l2 = R.case_problem(case), R.case_level2(case)
    full = _score(sp, l2, case, warmup=5)
    summ = _score(sp, l2, case, warmup=5, sink="summary")
    assert summ["level_1"] is None and summ["summary"]["n_draws"] == 50
    assert np.array_equal(bits(summ["state"]["lam"]), bits(full["state"]["lam"]))

    def dev_log(a):
        flat = np.ascontiguousarray(a, np.float64).ravel()
        out = np.empty_like(flat)
        _lib.check(L.clv_debug_log(_dp(flat), flat.size, _dp(out)))
        return out.reshape(a.shape)

    names = [s for s in R.SUM_STATS if D == 3 or "eta" not in s]
    assert sorted(summ["summary"]["sums"]) == sorted(names)
    for c in range(2):
        want = R.summary_sums(full["level_1"][c], log=dev_log)
        for k, s in enumerate(R.SUM_STATS):
            if s in names:
                assert np.array_equal(bits(summ["summary"]["sums"][s][c]), bits(want[k])), s
    pooled = np.stack(full["level_1"]).reshape(-1, sp.N, D + 2)
    means = summ["summary"]["means"]
    np.testing.assert_allclose(means["mean_lambda"], pooled[..., 0].mean(0), rtol=1e-13)
    np.testing.assert_allclose(means["mean_z"], pooled[..., 3].mean(0), rtol=1e-13)
    np.testing.assert_allclose(means["mean_mu_capped"], np.minimum(pooled[..., 1], 0.05).mean(0), rtol=1e-13)
    info = _lib.score_info()
    assert (info["block"], info["n_sum_stats"], info["D"], info["K"], info["sink"]) == (256, 11, D, K, _lib.SINK_SUMMARY)
    assert info["vgprs"] > 0 and info["scratch_bytes"] >= 0 and info["kernel_ns"] > 0


def test_sampler_route_equals_host_route(L):
    """HipSampler.score_customers (records in HBM) = score_customers on the records it returns: a
    300-customer, 12-sweep trivariate fit, the next 257 customers scored."""
    from mcmc_clv_model_amd import score_customers
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    covs = ["gender_F", "age_scaled"]
    df = cdnow("abe")
    new = df.iloc[300:557].reset_index(drop=True)
    p = build_problem(df.iloc[:300], covs, 3)
    kw = dict(inner_sweeps=2, warmup=4, seed=11, customer_offset=300)
    with HipSampler(p, mcmc=12, burnin=0, thin=1, chains=2, seed=5, draw_sink="summary", chain_first=1) as s:
        s.run(12)
        a = s.score_customers(new, covs, **kw)
        _, l2, _ = s.read_draws(level1=False)
    b = score_customers({"level_2": list(l2)}, new, covs, omega2=p.omega2, chain_first=1, **kw)
    assert np.array_equal(bits(np.stack(a["level_1"])), bits(np.stack(b["level_1"])))
    assert np.array_equal(bits(a["state"]["lam"]), bits(b["state"]["lam"]))
    assert np.array_equal(bits(np.stack(a["level_2"])), bits(l2)) and np.isfinite(np.stack(a["level_1"])).all()


def test_analysis_functions_take_the_scored_dict(L):
    """lifetime_value, draw_future_transactions and information_criteria on the scored dict = the same
    on a hand-built dict of the same arrays; level1_summary and level1_diagnostics run."""
    from mcmc_clv_model_amd import analysis as A
    case = dict(R.CASES["tri3"], records=8, R=1)     # 8 records per chain: the shortest series the diagnostics take
    sp = R.case_problem(case)
    scored = _score(sp, R.case_level2(case), case, warmup=2)
    cbs = sp.df
    hand = {"level_1": [np.array(a, copy=True) for a in scored["level_1"]]}
    lv, lv_h = A.lifetime_value(scored), A.lifetime_value(hand)
    for k in lv:
        if hasattr(lv[k], "to_numpy"):
            assert np.array_equal(bits(lv[k].to_numpy(float)), bits(lv_h[k].to_numpy(float))), k
    assert np.array_equal(A.draw_future_transactions(cbs, scored, seed=3), A.draw_future_transactions(cbs, hand, seed=3))
    ic, ic_h = A.information_criteria(scored, cbs), A.information_criteria(hand, cbs)
    assert np.array_equal(bits(ic["pointwise"].to_numpy()), bits(ic_h["pointwise"].to_numpy()))
    assert len(A.level1_summary(scored)) == sp.N and len(A.level1_diagnostics(scored)) == sp.N


def test_full_sink_too_large_names_the_summary_sink(L):
    """1,000,000 customers x 4 chains x 20,000 records x 4 doubles = 2.6 TB: refused before anything
    is allocated on the device, and the message names sink="summary"."""
    from mcmc_clv_model_amd import score_customers
    l2 = np.broadcast_to(R.synth_level2(2, 1, 1, 1, 1, plant=False), (4, 20000, 5))
    with pytest.raises(MemoryError, match='sink="summary"'):
        score_customers({"level_2": list(l2)}, cdnow_tiled(1_000_000), warmup=0, inner_sweeps=1)


# ---------------------------------------------------------------------------------------------
# the target distribution
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.DIST_MODELS))
def test_scored_draws_have_the_target_distribution(L, name):
    """Every record of every chain one constant (beta, Sigma): the scheme is exactly invariant, and the
    device's posterior means of log lambda, log mu and P(alive) (Rao-Blackwellised) of 64 customers
    must lie within 5 MCSE (diagnostics_ref.series_stats on the device's own draws) of the
    quadrature's — 192 comparisons at 5 standard errors with a fixed seed; the float64 model meets
    the same condition with the same seeds (tests/test_score_cpu.py)."""
    from mcmc_clv_model_amd import score_customers
    sp, rec = R.dist_problem(name), R.dist_record(name)
    D = R.DIST
    l2 = np.broadcast_to(rec, (D["chains"], D["records"], rec.shape[0]))
    out = score_customers({"level_2": list(l2)}, sp.df, sp.covs, inner_sweeps=D["R"], warmup=D["warmup"],
                          n_mh_steps=D["S"], seed=R.DIST_SEED, omega2=sp.omega2)
    diff, mcse = R.dist_check(R.dist_series(np.stack(out["level_1"]), sp), R.dist_quadrature(name))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(mcse > 0, diff / mcse, 0.0)
    print(f"{name}: largest |device mean - quadrature| / MCSE: log lambda {z[0].max():.2f}, log mu {z[1].max():.2f}, "
          f"P(alive) {z[2].max():.2f}; series that never move: {(mcse == 0).sum()}")
    assert R.dist_ok(diff, mcse).all(), np.argwhere(~R.dist_ok(diff, mcse))

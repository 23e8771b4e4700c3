"""GPU parity tests of the HIP path (through the C ABI), against the oracle and the reference's
recorded outputs (golden fixtures).  Tolerances are stated per test."""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

from oracle import philox as oph
from tests import summary_ref as SR
from tests.helpers import GOLDEN, bits, cdnow, golden, replay_case, with_covariates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def _u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---------------------------------------------------------------------------------------------
def test_device_philox_known_answers(L):
    """Bit-exact: device Philox4x32-10 vs Random123 KAT + 64 extra oracle vectors."""
    kat = json.load(open(os.path.join(GOLDEN, "philox_kat.json")))
    for k in kat["random123"]:
        ctr = np.array(k["ctr"], np.uint32)
        out = np.zeros(4, np.uint32)
        assert L.clv_debug_philox(k["key"][0], k["key"][1], _u32p(ctr), 1, _u32p(out)) == 0
        assert [f"{v:08x}" for v in out] == k["out"]
    e = kat["extra"]
    ctr = np.ascontiguousarray(np.array(e["ctr"], np.uint32))
    out = np.zeros_like(ctr)
    assert L.clv_debug_philox(e["key"][0], e["key"][1], _u32p(ctr), len(ctr), _u32p(out)) == 0
    assert np.array_equal(out, np.array(e["out"], np.uint32))


def test_device_variates_match_oracle(L):
    """u53 uniforms bit-exact; fp64 transforms <= 1e-13 rel; fp32 hardware-transcendental
    transforms (t3 noise) <= 2e-5 rel/abs (v_log/v_sin/v_cos/v_rsq are ~1-2 ulp fp32)."""
    n, S, seed, chain, sweep = 4096, 7, 987654321, 2, 77  # one full and one partial 4-step chunk
    tl, tm, ua, l2u = (np.zeros(n * S, np.float32) for _ in range(4))
    uz, ut, ea, ez = (np.zeros(n) for _ in range(4))
    assert L.clv_debug_variates(seed, chain, sweep, n, S, _fp(tl), _fp(tm), _fp(ua), _dp(uz), _dp(ut), _dp(ea),
                                _dp(ez), _fp(l2u)) == 0
    ref = oph.sweep_variates(seed, chain, sweep, n, S)
    assert np.array_equal(uz, ref["u_z"]) and np.array_equal(ut, ref["u_tau"])
    np.testing.assert_allclose(ea, ref["e_alive"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(ez, ref["eta_z"], rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(ua.reshape(S, n), ref["u_acc"])
    np.testing.assert_allclose(tl.reshape(S, n), ref["t_l"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(tm.reshape(S, n), ref["t_m"], rtol=2e-5, atol=2e-5)
    # the accept threshold's log2 U (v_log_f32 of the same fp32 uniform), to fp32 rounding
    np.testing.assert_allclose(l2u.reshape(S, n), np.log2(ref["u_acc"].astype(np.float64)), rtol=2**-22, atol=2**-24)


def test_accept_log2u_over_every_word(L):
    """Verdict r4 #4: the accept threshold's log2 U is v_log_f32 of uf32(w) (philox.h log2_f32),
    checked on the device against float64 log2 of the same fp32 uniform for ALL 2^32 Philox words
    (clv_debug_log2u_scan): within 1 fp32 ulp of the exact value everywhere — near U = 1 as well,
    where log2 U -> 0 (measured on MI355X: max 0.99975 ulp; absolute error <= 0.5 ulp of 33, 1.9e-6,
    at U ~ 2^-33).  In the accept test exp(lp' - lp) > U (bi:329-330), taken as lp' - lp >
    ln2 log2 U in fp64, an error e in log2 U scales the acceptance ratio by 2^e, |e| <= 2^-23 |log2 U|
    <= 4e-6: far below what test_shipped_mh_step_preserves_the_target resolves (2^0.02)."""
    out = np.zeros(4)
    assert L.clv_debug_log2u_scan(0, 1 << 32, _dp(out)) == 0
    max_ulp, max_abs, worst_word, max_ulp_far = out
    print(f"log2 U over 2^32 words: max {max_ulp:.5f} ulp (word {int(worst_word):#010x}), "
          f"max abs {max_abs:.3e}, max {max_ulp_far:.5f} ulp where U <= 1/2")
    assert max_ulp <= 1.0, out
    assert max_ulp_far <= 1.0 and max_abs <= 0.5 * 2.0 ** (5 - 23), out


def test_device_hyper_variates_match_oracle(L):
    """Marsaglia–Tsang chi-square and Box–Muller normals of the hyper stream (fp64): <= 1e-12 rel."""
    n, seed, chain, sweep = 64, 31337, 1, 5
    for df in (5.0, 23575.0, 1e7 + 3):
        chi, nor = np.zeros(n), np.zeros(n)
        assert L.clv_debug_hyper_variates(seed, chain, sweep, df, n, _dp(chi), _dp(nor)) == 0
        ref = np.array([oph.chi2_draw(seed, chain, sweep + i, 0, df) for i in range(n)])
        np.testing.assert_allclose(chi, ref, rtol=1e-12)
        refn = np.array([oph.hyper_normal(seed, chain, 0, sweep + i) for i in range(n)])
        np.testing.assert_allclose(nor, refn, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 9])
def test_device_level2_vs_reference(L, D, K):
    """Device level-2 draw from sufficient statistics vs the reference's _draw_level_2
    (bi:233-262) with the same Bartlett variates: Sigma <= 1e-11 rel; beta = B_hat +
    kron(chol Sigma, chol V) z (the device's factor of the same kron covariance) <= 1e-10."""
    from mcmc_clv_model_amd import _lib
    f = golden("formulas.npz")
    p = f"l2_D{D}_K{K}_"
    X, Y, B0 = f[p + "X"], f[p + "Y"], f[p + "B0"]
    A0 = np.eye(K) * 0.01
    S0 = float(f[p + "nu0"]) * np.eye(D)
    V = f[p + "V"]
    pr = _lib.ClvPrior()
    for i, v in enumerate(V.ravel()):
        pr.V[i] = v
    for i, v in enumerate(np.linalg.cholesky(V).ravel()):
        pr.chol_V[i] = v
    for i, v in enumerate((A0 @ B0).ravel()):
        pr.A0B0[i] = v
    for i, v in enumerate((S0 + B0.T @ A0 @ B0).ravel()):
        pr.S0_B0A0B0[i] = v
    xty = np.ascontiguousarray(X.T @ Y)
    yty = np.ascontiguousarray(Y.T @ Y)
    iwn = np.zeros(3)
    iwn[: D * (D - 1) // 2] = f[p + "iw_normal"]
    chi = np.ascontiguousarray(f[p + "iw_chi2"])
    z = np.ascontiguousarray(f[p + "mvn_z"])
    beta, sig = np.zeros(K * D), np.zeros(D * D)
    assert L.clv_debug_level2(D, K, ctypes.byref(pr), _dp(xty), _dp(yty), _dp(iwn), _dp(chi), _dp(z), _dp(beta),
                              _dp(sig)) == 0
    np.testing.assert_allclose(sig.reshape(D, D), f[p + "Sigma"], rtol=1e-11)
    Bh = f[p + "Bhat"]
    w = np.kron(np.linalg.cholesky(f[p + "Sigma"]), np.linalg.cholesky(V)) @ z
    np.testing.assert_allclose(beta.reshape(K, D), (Bh.ravel() + w).reshape(K, D), rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------
def _replay_run(name):
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    df, covs, f = replay_case(name)
    fn = mcmc_draw_parameters if str(f["kind"]) == "bi" else mcmc_draw_parameters_rfm_m
    d = fn(df, covs, mcmc=int(f["mcmc"]), burnin=0, thin=1, chains=int(f["chains"]), seed=int(f["seed"]), trace=0,
           n_mh_steps=int(f["S"]), rng="replay", replay_tape=f["tape"], replay_sweeps=int(f["n_tape_sweeps"]))
    return d, f


@pytest.mark.parametrize("name", ["bi_k1", "bi_k2", "tri_k3", "bi_k1_s0", "bi_k5", "tri_k9"])
def test_replay_trajectory_matches_reference(L, name):
    """G2: the HIP sampler consuming the reference's own variates reproduces the reference's
    trajectory (every sweep stored): lambda, mu, tau, eta and level-2 draws <= 1e-12 rel
    (1e-10 for the level-2 record, whose S_n is summed in a different order), z exact, and the
    marginal log-likelihood <= 1e-12 rel.  At most 0.5% of customers may differ (borderline
    accept flips from 1-ulp exp/log differences — none expected in 3 sweeps).
    bi_k5 / tri_k9 run the c4 / c5 kernel instances' covariate handling (X @ beta of bi:284,
    tri:403, tri:321 and X'Y): sweep_kernel_occ4<2,5> with the covariate row in registers and
    sweep_kernel<3,9> with it in LDS (Cust<3,9,CL=true>), on 384 customers (a half-filled block)."""
    d, f = _replay_run(name)
    l1 = np.stack(d["level_1"])
    ref = f["level_1"]
    assert l1.shape == ref.shape
    close = np.isclose(l1, ref, rtol=1e-12, atol=0).all(axis=(1, 3))  # (chains, N) over draws & columns
    assert close.mean() >= 0.995, f"{(~close).sum()} customers diverge"
    assert (l1[..., 3] == ref[..., 3]).mean() >= 0.995
    np.testing.assert_allclose(np.stack(d["level_2"]), f["level_2"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(d["log_likelihood"], float(f["log_likelihood"]), rtol=1e-12)


def test_replay_bitwise_fraction(L):
    """Informational: kernels follow numpy's operation order (no FMA contraction), but S_n is a
    different summation (block partials, bi:253-255 sums E'E directly) and exp/log are ocml, so
    trajectories agree to ~1e-15 rel rather than bit for bit; report the bit-identical share."""
    d, f = _replay_run("bi_k2")
    l1 = np.stack(d["level_1"])
    frac_bitwise = np.mean(bits(l1[..., :3]) == bits(f["level_1"][..., :3]))
    print(f"bit-identical fraction of lambda/mu/tau: {frac_bitwise:.4f}")
    assert frac_bitwise > 0.01


# ---------------------------------------------------------------------------------------------
def _bi(df, covs=(), **kw):
    from mcmc_clv_model_amd import mcmc_draw_parameters
    base = dict(mcmc=20, burnin=10, thin=2, chains=2, seed=123, trace=0)
    base.update(kw)
    return mcmc_draw_parameters(df, list(covs), **base)


def test_determinism_bitwise(L):
    df = cdnow("abe", 1000)
    a, b = _bi(df, ["first_sales_scaled"]), _bi(df, ["first_sales_scaled"])
    for x, y in zip(a["level_1"] + a["level_2"], b["level_1"] + b["level_2"]):
        assert np.array_equal(bits(x), bits(y))


def test_chain_batching_invariance(L):
    """Counter-based RNG: chain c's draws do not depend on how many chains share the launch."""
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", 700)
    p = build_problem(df, ["first_sales_scaled"], 2)
    kw = dict(mcmc=6, burnin=3, thin=1, seed=99)
    with HipSampler(p, chains=3, **kw) as s3:
        s3.run(9)
        a1, a2, _ = s3.read_draws()
    with HipSampler(p, chains=1, chain_first=2, **kw) as s1:
        s1.run(9)
        b1, b2, _ = s1.read_draws()
    assert np.array_equal(bits(a1[2]), bits(b1[0])) and np.array_equal(bits(a2[2]), bits(b2[0]))


def test_resume_from_state_is_exact(L):
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", 500)
    for D, covs in ((2, ["first_sales_scaled"]), (3, ["gender_F", "age_scaled"])):
        p = build_problem(df, covs, D)
        kw = dict(mcmc=10, burnin=0, thin=1, chains=8, seed=5, draw_sink="none")
        with HipSampler(p, **kw) as s:
            s.run(10)
            ref = s.get_state()
        # the hyper state set from (beta, Sigma) must carry the uninterrupted run's bits
        # (Philox mode finalises with rcp_nr / rsq_nr in the draw and in clv_set_state alike); several
        # split points x 8 chains, so an ulp mismatch of the finalisation cannot hide
        for k in (1, 4, 7, 9):
            with HipSampler(p, **kw) as s:
                s.run(k)
                st = s.get_state()
            with HipSampler(p, **kw) as s:
                s.set_state(*st, sweeps_done=k)
                s.run(10 - k)
                got = s.get_state()
            for x, y in zip(ref, got):
                assert np.array_equal(bits(x), bits(y)), (D, k)
        with HipSampler(p, **kw) as s:  # states exp() of a log-scale state can never take
            lam, mu = st[0].copy(), st[1].copy()
            for bad in (0.0, -1.0, np.inf, np.nan, 1e-310):
                lam[0, 3] = bad
                with pytest.raises(ValueError, match="positive, normal and finite"):
                    s.set_state(lam, mu, st[2], st[3], sweeps_done=4)


def test_storage_indexing_and_summary_sink(L):
    """burnin/thin storage (bi:402) and the on-device summary sink == means of the full draws: every
    stat against tests/summary_ref.py, the exact ones by their bits, the log ones within its bound."""
    df = cdnow("abe", 600)
    kw = dict(mcmc=23, burnin=7, thin=4, chains=2, seed=4242)
    full = _bi(df, **kw)
    summ = _bi(df, draw_sink="summary", **kw)
    nd = (23 - 1) // 4 + 1
    assert full["level_1"][0].shape == (nd, 600, 4) and full["level_2"][0].shape == (nd, 5)
    assert summ["level_1"] is None and summ["summary"]["n_draws"] == nd
    sm = summ["summary"]
    assert sorted(sm) == sorted(["n_draws"] + [nm for nm in SR.SUM_STATS if "eta" not in nm])
    for c in range(2):
        l1 = full["level_1"][c]
        ref = SR.sums_from_draws(l1) / nd
        for k, nm in enumerate(SR.SUM_STATS):
            if nm not in sm:
                continue
            if nm in SR.LOG_STATS:  # the division by nd rounds once on either side
                bound = SR.log_sum_bound(l1[:, :, SR.LOG_COLUMN[nm]]) / nd + SR.U * (np.abs(sm[nm][c]) + np.abs(ref[k]))
                assert np.all(np.abs(sm[nm][c] - ref[k]) <= bound), (c, nm)
            else:
                assert np.array_equal(bits(sm[nm][c]), bits(ref[k])), (c, nm)
        assert np.array_equal(bits(summ["level_2"][c]), bits(full["level_2"][c]))


@pytest.mark.parametrize("persistent", ["1", "0"])
def test_streamed_draws_bitwise_equal_read_after_run(L, monkeypatch, persistent):
    """Verdict r4 #3: level-1 draws streamed into the host buffer while the sampler runs
    (clv_stream_draws: the stored sweeps in sub-runs, each sub-run's draws copied by the host pool
    while the next runs) equal, bit for bit, the draws of the same run read after it — through a run
    cut into uneven calls (one call spans the burn-in boundary and several sub-runs) that stops one
    sweep short of the last stored draw (its slot is zeros in both), persistent kernel and
    launch-per-sweep kernel alike; level-2 records and log-likelihood too."""
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    monkeypatch.setenv("CLV_PERSISTENT", persistent)
    p = build_problem(cdnow("abe"), ["first_sales_scaled"], 2)
    kw = dict(mcmc=600, burnin=300, thin=1, chains=3, seed=11, draw_sink="full")
    calls = (100, 450, 349)
    with HipSampler(p, **kw) as s:
        assert s.launch_info()["persistent"] == (persistent == "1")
        s.run(sum(calls))
        ref = s.read_draws()
    with HipSampler(p, **kw) as s:
        buf = s.level1_buffer()
        buf.fill(np.nan)
        s.stream_draws(buf)
        for n in calls:
            s.run(n)
        got = s.read_draws(out=buf)
    assert got[0] is buf
    assert not ref[0][:, -1].any()  # the draw never stored: zeros
    for a, b in zip(ref, got):
        assert np.array_equal(bits(a), bits(b))


def test_stream_draws_arguments(L):
    """clv_stream_draws needs the full sink; the end-to-end drop-in (which streams) returns the same
    draws as the sampler read after its run."""
    from mcmc_clv_model_amd import mcmc_draw_parameters
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", 700)
    p = build_problem(df, [], 2)
    with HipSampler(p, mcmc=8, burnin=2, thin=2, chains=2, seed=5, draw_sink="summary") as s:
        with pytest.raises(Exception, match="CLV_SINK_FULL"):
            s.stream_draws(np.empty((2, 4, 700, 4)))
    with HipSampler(p, mcmc=8, burnin=2, thin=2, chains=2, seed=5) as s:
        with pytest.raises(ValueError):
            s.stream_draws(np.empty((2, 4, 700, 3)))
        ro = s.level1_buffer()
        ro.flags.writeable = False
        with pytest.raises(ValueError):
            s.stream_draws(ro)
        s.run(10)
        l1, l2, ll = s.read_draws()
    d = mcmc_draw_parameters(df, mcmc=8, burnin=2, thin=2, chains=2, seed=5, trace=0)
    for c in range(2):
        assert np.array_equal(bits(d["level_1"][c]), bits(l1[c])) and np.array_equal(bits(d["level_2"][c]), bits(l2[c]))


def test_clock_record_persistent_and_launch_per_sweep(L):
    """clv_clock_ghz: the shader clock over a run of the persistent kernel, from chain 0's level-2
    workgroup's (s_memtime, s_memrealtime) between publishes (per-CU intervals: s_memtime counts per
    XCD); 0 for a one-sweep run and for the launch-per-sweep kernel, which keeps no record.  MI355X's
    engine clock is at most 2.4 GHz.  clv_clock_probe (a 50 us probe kernel behind the run) reads
    it for either kernel and agrees with the persistent kernel's record."""
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from mcmc_clv_model_amd.data import synthetic_cbs
    cases = [(build_problem(cdnow("full"), ["first_sales_scaled"], 2), 4, True),
             (build_problem(synthetic_cbs(150_000, 5, seed=3), [f"c{k}" for k in range(1, 5)], 2), 2, False)]
    for p, chains, persistent in cases:
        with HipSampler(p, mcmc=1000, burnin=1000, thin=10, chains=chains, seed=9, draw_sink="summary") as s:
            assert s.launch_info()["persistent"] == persistent
            s.run(1)
            assert s.clock_ghz() == 0.0
            s.run(200)
            ghz = s.clock_ghz()
            probe = s.clock_probe(50.0)  # verdict r5 #6: every leg's clock, the probe kernel behind the run
            print(f"persistent={persistent}: record {ghz:.3f} GHz, probe {probe:.3f} GHz")
            assert 0.5 < probe < 2.6
            if not persistent:
                assert ghz == 0.0
                continue
            assert 0.5 < ghz < 2.6
            # the two readings of one clock, the probe a moment after the run and under a lighter load
            # (measured 2.17 record vs 2.35 probe on one box, 2.38-2.41 vs 2.34-2.35 on others)
            assert abs(probe / ghz - 1) < 0.2
            s.run(1500)  # longer than the record (the last 1024 sweeps)
            assert 0.5 < s.clock_ghz() < 2.6


@pytest.mark.parametrize("val", ["inf", "nan", "0x10", "5 ms"])
def test_wait_timeout_env_rejected(L, monkeypatch, val):
    """a CLV_WAIT_TIMEOUT_MS that is not a finite decimal number fails clv_create (EINVAL)
    instead of reaching (uint64_t)(ms * 1e5); a finite one is clamped to [1 ms, 1 h]."""
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    p = build_problem(cdnow("abe", 600), [], 2)
    monkeypatch.setenv("CLV_WAIT_TIMEOUT_MS", val)
    with pytest.raises(ValueError, match="CLV_WAIT_TIMEOUT_MS"):
        HipSampler(p, mcmc=2, burnin=0, thin=1, chains=1, seed=1)
    monkeypatch.setenv("CLV_WAIT_TIMEOUT_MS", "1e12")
    with HipSampler(p, mcmc=2, burnin=0, thin=1, chains=1, seed=1) as s:
        assert s.launch_info()["persistent"]
        s.run(2)


def test_edge_cases(L):
    """Single customer, zero-MH-step sweeps, all-zero repeat customers, maximum K=9/D=3."""
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    df = cdnow("abe")
    one = df[df["x"] > 0].iloc[:1].copy()
    d = mcmc_draw_parameters(one, mcmc=5, burnin=2, thin=1, chains=1, seed=1, trace=0)
    assert np.isfinite(d["level_1"][0]).all()
    # all-zero x: lam_init = 0 and math.log(0) raises in the reference's setup (bi:373) too
    with pytest.raises(ValueError, match="math domain error"):
        mcmc_draw_parameters(df[df["x"] == 0].iloc[:5], mcmc=2, burnin=0, thin=1, chains=1, seed=1, trace=0)
    d = mcmc_draw_parameters(df.iloc[:300], mcmc=3, burnin=0, thin=1, chains=1, seed=1, trace=0, n_mh_steps=0)
    assert np.isfinite(d["level_2"][0]).all()
    zero = pd.concat([df[df["x"] == 0].iloc[:390], df[df["x"] > 0].iloc[:10]])  # mostly x = t_x = 0
    d = mcmc_draw_parameters(zero, mcmc=5, burnin=5, thin=1, chains=1, seed=2, trace=0)
    assert np.isfinite(d["level_1"][0]).all()
    rng = np.random.default_rng(0)
    big = df.iloc[:800].copy()
    covs = []
    for k in range(8):
        big[f"c{k}"] = rng.uniform(-1, 1, len(big))
        covs.append(f"c{k}")
    d = mcmc_draw_parameters_rfm_m(big, covs, mcmc=4, burnin=2, thin=1, chains=2, seed=3, trace=0)
    assert d["level_2"][0].shape == (4, 3 * 9 + 6) and np.isfinite(d["level_2"][0]).all()
    assert isinstance(d["log_likelihood"], float)


def test_validation_errors_match_reference(L):
    from mcmc_clv_model_amd import mcmc_draw_parameters
    df = cdnow("abe", 10)
    with pytest.raises(ValueError, match="cal_cbs missing required column 't_x'"):
        mcmc_draw_parameters(df.drop(columns=["t_x"]))
    with pytest.raises(ValueError, match="some covariate columns not in cal_cbs"):
        mcmc_draw_parameters(df, ["nope"])


def test_trace_lines(L, capsys):
    df = cdnow("abe", 100)
    _bi(df, mcmc=4, burnin=4, thin=1, chains=2, trace=4)
    out = capsys.readouterr().out.splitlines()
    # the reference's order: its chains run one after another (bi:383-384, bi:484)
    assert out == ["chain 1 | step 4/8", "chain 1 | step 8/8", "chain 2 | step 4/8", "chain 2 | step 8/8"]


@pytest.mark.parametrize("D,covs,n", [(2, ["first_sales_scaled"], 23570), (3, ["gender_F", "age_scaled"], 2357),
                                      (2, [], 150_000)])
def test_sharded_path_bitwise_equals_unsharded(L, D, covs, n):
    """Row (e): W shards on one GPU through the sharded C path (sweep + group kernels, exchange of
    unit partials, standalone hyper kernel on the gathered buffer) reproduce the unsharded fused
    run bit for bit — the fixed-order reduction makes results independent of the GPU count."""
    import torch
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem, make_prior
    from mcmc_clv_model_amd.data import synthetic_cbs
    df = cdnow("full") if n == 23570 else (cdnow("abe") if n == 2357 else synthetic_cbs(n, 1, 2, seed=5))
    p = build_problem(df, covs, D)
    kw = dict(mcmc=6, burnin=3, thin=2, chains=2, seed=77, draw_sink="summary")
    sweeps = 9
    with HipSampler(p, **kw) as s:
        s.run(sweeps)
        ref = s.get_state()
        ref_sums, _ = s.read_summary()
        _, ref_l2, ref_ll = s.read_draws(level1=False)
    for world in (2, 3):
        plan = Dm.plan(p.N, world)
        prior = make_prior(p, p.N)
        shards = []
        for r in range(world):
            b, e = plan.shard(r)
            shards.append(HipSampler(Dm.slice_problem(p, b, e), n_global=p.N, shard_begin=r * plan.blocks_per_rank * 256,
                                     world_size=world, rank=r, blocks_per_rank=plan.blocks_per_rank,
                                     blocks_per_unit=plan.blocks_per_unit, prior=prior, **kw))
        nd = shards[0].partials()[1]
        gathered = torch.zeros(nd * world, dtype=torch.float64, device="cuda")

        def exchange():
            for r, sh in enumerate(shards):
                sh.copy_partials(gathered.data_ptr() + r * nd * 8)
                sh.synchronize()
            for sh in shards:
                sh.hyper(gathered.data_ptr())

        if D == 2:
            exchange()  # bivariate: initial draw from the initial state
        for _ in range(sweeps):
            for sh in shards:
                sh.sweep()
            exchange()
        for sh in shards:
            sh.synchronize()
        for r, sh in enumerate(shards):
            b, e = plan.shard(r)
            lam, mu, beta, sigma = sh.get_state()
            assert np.array_equal(bits(lam), bits(ref[0][:, b:e])) and np.array_equal(bits(mu), bits(ref[1][:, b:e]))
            assert np.array_equal(bits(beta), bits(ref[2])) and np.array_equal(bits(sigma), bits(ref[3]))
            sums, _ = sh.read_summary()
            assert np.array_equal(bits(sums), bits(ref_sums[:, :, b:e]))
            _, l2, ll = sh.read_draws(level1=False)
            assert np.array_equal(bits(l2), bits(ref_l2)) and np.array_equal(bits(ll), bits(ref_ll))
        for sh in shards:
            sh.close()


@pytest.mark.parametrize("cfg", ["c4", "c5"])
def test_full_size_eight_shards_bitwise(L, cfg):
    """Maximum sizes: c5 — the whole 10M-customer trivariate K=9 problem — and c4 —
    1M bivariate customers, K=5 — on one GPU, and the same problem as the driver's 8-GPU layout
    (8 shards of 1.25M / 125k customers through the sharded C path on one card) agree bit for bit
    after 3 sweeps (state, summary sums, level-2 draws, log-likelihood): size-independent parity
    at the full sizes (64-bit indexing, 39,063 / 3,907 blocks, 512-unit exchange); plus the
    posterior moments' sanity (finite, P(alive) in [0, 1])."""
    import torch
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.data import synthetic_cbs
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem, make_prior
    if cfg == "c5":
        p = build_problem(synthetic_cbs(10_000_000, 9, 3, seed=20250719), [f"c{k}" for k in range(1, 9)], 3)
    else:
        p = build_problem(synthetic_cbs(1_000_000, 5, 2, seed=20250718), [f"c{k}" for k in range(1, 5)], 2)
    kw = dict(mcmc=2, burnin=1, thin=1, chains=1, seed=20250719, draw_sink="summary")
    sweeps = 3
    with HipSampler(p, **kw) as s:
        s.run(sweeps)
        ref = s.get_state()
        ref_sums, k_ref = s.read_summary()
        _, ref_l2, ref_ll = s.read_draws(level1=False)
    assert k_ref == 2 and np.isfinite(ref_l2).all() and np.isfinite(ref_ll).all()
    assert np.isfinite(ref_sums).all() and (ref_sums[:, 2] >= 0).all() and (ref_sums[:, 2] <= k_ref).all()
    world = 8
    plan = Dm.plan(p.N, world)
    prior = make_prior(p, p.N)
    shards = []
    for r in range(world):
        b, e = plan.shard(r)
        shards.append(HipSampler(Dm.slice_problem(p, b, e), n_global=p.N, shard_begin=r * plan.blocks_per_rank * 256,
                                 world_size=world, rank=r, blocks_per_rank=plan.blocks_per_rank,
                                 blocks_per_unit=plan.blocks_per_unit, prior=prior, **kw))
    nd = shards[0].partials()[1]
    gathered = torch.zeros(nd * world, dtype=torch.float64, device="cuda")

    def exchange_and_hyper():
        for r, sh in enumerate(shards):
            sh.copy_partials(gathered.data_ptr() + r * nd * 8)
            sh.synchronize()
        for sh in shards:
            sh.hyper(gathered.data_ptr())

    try:
        if p.D == 2:  # bivariate: the initial draw from the initial state (bi:393 at step 1)
            exchange_and_hyper()
        for _ in range(sweeps):  # the level-2 draw closes each sweep
            for sh in shards:
                sh.sweep()
            exchange_and_hyper()
        for r, sh in enumerate(shards):
            sh.synchronize()
            b, e = plan.shard(r)
            lam, mu, beta, sigma = sh.get_state()
            assert np.array_equal(bits(lam), bits(ref[0][:, b:e])) and np.array_equal(bits(mu), bits(ref[1][:, b:e]))
            assert np.array_equal(bits(beta), bits(ref[2])) and np.array_equal(bits(sigma), bits(ref[3]))
            sums, _ = sh.read_summary()
            assert np.array_equal(bits(sums), bits(ref_sums[:, :, b:e]))
            _, l2, ll = sh.read_draws(level1=False)
            assert np.array_equal(bits(l2), bits(ref_l2)) and np.array_equal(bits(ll), bits(ref_ll))
    finally:
        for sh in shards:
            sh.close()


@pytest.mark.parametrize("graph_chunk", [0, 4])
def test_sharded_sampler_rccl_matches_fused(L, graph_chunk):
    """Row (e) through the production class: ShardedSampler at world size 1 over a real
    torch.distributed "nccl" (= RCCL) process group — sweep + group kernels, partial copy,
    all_gather_into_tensor, standalone hyper kernel — eager and torch.cuda-graph-captured
    (chunks of 4 sweeps incl. the all-gather, plus eager remainder) equals the fused run bit for bit."""
    import socket
    import torch
    import torch.distributed as dist
    from mcmc_clv_model_amd.distributed import ShardedSampler
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    p = build_problem(cdnow("full"), ["first_sales_scaled"], 2)
    kw = dict(mcmc=6, burnin=3, thin=2, chains=2, seed=91, draw_sink="summary")
    sweeps = 9
    with HipSampler(p, **kw) as s:
        s.run(sweeps)
        ref = s.get_state()
        ref_sums, _ = s.read_summary()
        _, ref_l2, ref_ll = s.read_draws(level1=False)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    store = dist.TCPStore("127.0.0.1", port, 1, True)
    dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        ss = ShardedSampler(p, rank=0, world=1, graph_chunk=graph_chunk, device=0, **kw)
        ss.step(sweeps)
        ss.synchronize()
        lam, mu, beta, sigma = ss.s.get_state()
        sums, _ = ss.s.read_summary()
        _, l2, ll = ss.s.read_draws(level1=False)
        assert ss.s.sweeps_done == sweeps
        ss.close()
    finally:
        dist.destroy_process_group()
    assert np.array_equal(bits(lam), bits(ref[0])) and np.array_equal(bits(mu), bits(ref[1]))
    assert np.array_equal(bits(beta), bits(ref[2])) and np.array_equal(bits(sigma), bits(ref[3]))
    assert np.array_equal(bits(sums), bits(ref_sums))
    assert np.array_equal(bits(l2), bits(ref_l2)) and np.array_equal(bits(ll), bits(ref_ll))


def test_device_fast_exp_accuracy(L):
    """exp_fast (csrc/fastmath.h), used by the Philox-mode MH step on arguments clipped to
    [-70, 70] (bi:323): <= 2 ulp from the correctly rounded exp (numpy's exp is within 1 ulp of
    it, so the test allows 3 ulp against numpy) over the whole range and near 0.  The same bound over
    the range fastmath.h claims, |x| <= 700, which draw_z, draw_tau (exponents capped at 700, bi:223)
    and the eta draw call it on, with the caps and the clip themselves and their neighbours."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-70, 70, 200_000), rng.uniform(-1e-3, 1e-3, 20_000),
                        np.array([-70.0, 70.0, 0.0, -0.0, 1e-300, np.log(2) / 128, -np.log(2) / 128])])
    out = np.zeros_like(x)
    assert L.clv_debug_exp(_dp(x), x.size, _dp(out)) == 0
    ref = np.exp(x)
    ulp = np.abs(out - ref) / np.spacing(ref)
    assert ulp.max() <= 3.0, ulp.max()
    assert np.mean(out == ref) > 0.6
    e = 70.0 + 2.0 ** -40
    xw = np.concatenate([np.random.default_rng(4).uniform(-700, 700, 200_000),
                         np.array([-700.0, 700.0, -70.0, 70.0, -e, e])])
    outw = np.zeros_like(xw)
    assert L.clv_debug_exp(_dp(xw), xw.size, _dp(outw)) == 0
    refw = np.exp(xw)
    ulpw = np.abs(outw - refw) / np.spacing(refw)
    print(f"exp_fast on [-700, 700]: largest deviation {ulpw.max():.2f} ulp, at the listed points {ulpw[-6:]}")
    assert np.isfinite(outw).all() and ulpw.max() <= 3.0, (ulpw.max(), xw[ulpw.argmax()])


@pytest.mark.parametrize("packed", [0, 1])
def test_t3_proposal_symmetric_over_every_angle(L, packed):
    """Verdict r3: the random-walk proposal of the production MH step is symmetric, so the MH
    acceptance of bi:316-330 (which omits the proposal ratio) stays exact.  t3 = R cos(2 pi V) with
    V on the 2^16-point angle lattice (philox.h t3_f32 / t3_pair, hardware v_cos_f32): for fixed
    radius words, every angle of both 16-bit halves is run through the device transform, and the
    multiset of the 65,536 values must equal its negation exactly (R >= 0 is independent of V, so
    this is the proposal's symmetry).  Also pinned: the packed pair equals the scalar form bit for
    bit, and the stronger pairwise identity t(k + 2^15) == -t(k) for every angle k."""
    k = np.arange(65536, dtype=np.uint32)
    radius = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x12345678, 0x9E3779B9, 0x00C0FFEE]
    n = len(k)
    for rw in radius:
        w = np.empty((n, 3), np.uint32)
        w[:, 0] = rw
        w[:, 1] = rw
        w[:, 2] = (k << 16) | k
        outs = {}
        for pk in (0, packed):
            tl, tm = np.empty(n, np.float32), np.empty(n, np.float32)
            assert L.clv_debug_t3(_u32p(np.ascontiguousarray(w)), n, pk, _fp(tl), _fp(tm)) == 0
            outs[pk] = (tl, tm)
        tl, tm = outs[packed]
        assert np.array_equal(bits(tl), bits(outs[0][0])) and np.array_equal(bits(tm), bits(outs[0][1]))
        assert np.array_equal(tl, tm)  # the same angle in either half gives the same variate
        assert np.isfinite(tl).all() and (np.abs(tl).max() > 0 or rw == 0xFFFFFFFF)
        assert np.array_equal(np.sort(tl), np.sort(-tl)), f"radius word {rw:#x}: t3 multiset not symmetric"
        assert np.array_equal(tl, -np.roll(tl, -32768)), f"radius word {rw:#x}: t(k + 2^15) != -t(k)"


def test_device_fast_log_accuracy(L):
    """log_fast (csrc/fastmath.h), the Philox-mode logs of the z/tau draw (bi:200-225: log lambda,
    log mu, the dropout time's uniform / truncated-exponential argument) and eta's normal:
    <= 1 ulp from the correctly rounded log (tools/gen_log_table.py; 2 ulp allowed against numpy)
    over the normal range, across every table bin and the binade edges, and exact at 1."""
    rng = np.random.default_rng(4)
    x = np.concatenate([np.exp(rng.uniform(-705, 705, 200_000)), rng.uniform(0.5, 2.0, 100_000),
                        1.0 + rng.uniform(-2e-3, 2e-3, 50_000), rng.random(50_000) + 2.0 ** -53,
                        np.array([1.0, 2.0, 0.5, 4.0, 1 - 2.0 ** -53, 1 + 2.0 ** -52, 2.0 ** -53, 2.0 ** -1022,
                                  np.finfo(np.float64).max, 0.6865234375, 1.373046875])])
    out = np.zeros_like(x)
    assert L.clv_debug_log(_dp(x), x.size, _dp(out)) == 0
    ref = np.log(x)
    ulp = np.abs(out - ref) / np.spacing(np.abs(ref))
    nz = ref != 0
    assert ulp[nz].max() <= 2.0, (ulp[nz].max(), x[nz][np.argmax(ulp[nz])])
    assert np.all(out[~nz] == 0.0)
    assert np.mean(out == ref) > 0.6


def _run_mode(p, persistent, sweeps, chunks, **kw):
    """Run `sweeps` sweeps in clv_run calls of `chunks` sizes with the persistent kernel on/off
    (off: one launch per sweep)."""
    from mcmc_clv_model_amd.sampler import HipSampler
    env = {"CLV_PERSISTENT": "1" if persistent else "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = HipSampler(p, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    with s:
        info = s.launch_info()
        for n in chunks:
            s.run(n)
        assert s.sweeps_done == sweeps
        st = s.get_state()
        l1, l2, ll = s.read_draws(level1=kw.get("draw_sink", "full") == "full")
        sums = s.read_summary()[0] if kw.get("draw_sink") in ("summary", "summary+pct") else None
    return info, st, l1, l2, ll, sums


@pytest.mark.parametrize("D,covs,n,sink,S", [(2, ["first_sales_scaled"], 23570, "full", 20),
                                             (3, ["gender_F", "age_scaled"], 23570, "summary", 20),
                                             (2, [], 1000, "full", 20), (3, ["gender_F"], 300, "full", 20),
                                             (2, ["first_sales_scaled"], 2357, "full", 7),
                                             (3, ["gender_F"], 2357, "summary", 23),
                                             (2, [f"c{k}" for k in range(1, 5)], 3000, "summary", 20),
                                             (3, [f"c{k}" for k in range(1, 9)], 2357, "full", 20)])
def test_persistent_kernel_bitwise_equals_launch_per_sweep(L, monkeypatch, D, covs, n, sink, S):
    """World size 1: the persistent kernel (one launch for all of a clv_run's sweeps, sentinel-slot
    hand-off to a level-2 workgroup per chain) is chosen by default where the grid fits at once,
    and reproduces the launch-per-sweep path (fused level-2 tail) bit for bit — state, draws,
    level-2 records, log-likelihood, summaries — across clv_run calls of uneven length (the
    carried state at each launch boundary), burn-in and thinning; S = 7 (a partial last chunk of
    drawn-ahead variates) and S = 23 (more steps than the drawn-ahead registers hold: variates
    drawn within the sweep).  K = 5 (bivariate) and K = 9 (trivariate) compare the persistent
    kernel's register-resident covariate rows with the c4 / c5 launch-per-sweep instances
    (sweep_kernel_occ4<2,5>; sweep_kernel<3,9> with the covariate rows in LDS)."""
    df = cdnow("full", n) if n > 2357 else cdnow("abe", n)
    if covs and covs[0] == "c1":
        df = with_covariates(df, len(covs))
    from mcmc_clv_model_amd.sampler import build_problem
    p = build_problem(df, covs, D)
    kw = dict(mcmc=25, burnin=6, thin=3, chains=3, seed=2024, draw_sink=sink, n_mh_steps=S)
    chunks = (1, 7, 2, 20, 1)
    a = _run_mode(p, True, 31, chunks, **kw)
    b = _run_mode(p, False, 31, chunks, **kw)
    assert a[0]["persistent"] and not b[0]["persistent"], (a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(bits(x), bits(y))
    for x, y in zip(a[2:], b[2:]):
        if x is not None:
            assert np.array_equal(bits(x), bits(y))


def test_c4_eight_rank_shard_persistent_bitwise(L):
    """The instance one GPU runs in c4's 8-rank run at its full size (rank 0's shard of the 1M-customer
    K = 5 problem: 126,976 customers, 496 blocks; bench.py's c4_shard8 leg) at world size 1: the
    persistent kernel — level-2 workgroup alone on a CU (>= 256 blocks), coalesced slot resets by
    wavefronts 1-3 during the draw (round 6) — against one launch per sweep, bit for bit over uneven
    clv_run calls through burn-in and stored sweeps (state, running sums, level-2 records,
    log-likelihood)."""
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.data import synthetic_cbs
    from mcmc_clv_model_amd.sampler import build_problem
    full = build_problem(synthetic_cbs(1_000_000, 5, 2, seed=20250718), [f"c{k}" for k in range(1, 5)], 2)
    plan = Dm.plan(full.N, 8)
    b, e = plan.shard(0)
    p = Dm.slice_problem(full, b, e)
    assert p.N == 126_976
    del full
    kw = dict(mcmc=25, burnin=6, thin=3, chains=1, seed=2024, draw_sink="summary", n_mh_steps=20)
    chunks = (1, 7, 2, 20, 1)
    a = _run_mode(p, True, 31, chunks, **kw)
    c = _run_mode(p, False, 31, chunks, **kw)
    assert a[0]["persistent"] and not c[0]["persistent"], (a[0], c[0])
    for x, y in zip(a[1], c[1]):
        assert np.array_equal(bits(x), bits(y))
    for x, y in zip(a[2:], c[2:]):
        if x is not None:
            assert np.array_equal(bits(x), bits(y))
    assert np.isfinite(a[5]).all()  # the running sums


def _run_ops(p, env, ops, **kw):
    """A sampler created under `env`, driven by `ops` ("run", n) / ("state",) / ("rollback",);
    returns the states taken at ("state",) ops, the final state and the draws."""
    from mcmc_clv_model_amd.sampler import HipSampler
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = HipSampler(p, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    mid = []
    with s:
        info = s.launch_info()
        for op in ops:
            if op[0] == "run":
                s.run(op[1])
            elif op[0] == "state":
                mid.append(s.get_state())
            else:
                s.rollback()
        st = s.get_state()
        l1, l2, ll = s.read_draws(level1=kw.get("draw_sink", "full") == "full")
        sums = s.read_summary()[0] if kw.get("draw_sink") in ("summary", "summary+pct") else None
    return info, mid, st, l1, l2, ll, sums


def _same_bits(a, b):
    for x, y in zip(a, b):
        if isinstance(x, (list, tuple)):
            _same_bits(x, y)
        elif x is not None:
            assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("D,covs,sink", [(2, ["first_sales_scaled"], "full"), (3, ["gender_F", "age_scaled"], "summary")])
def test_deferred_level2_draw_bitwise(L, D, covs, sink):
    """Verdict r3 #1: a persistent launch leaves the level-2 draw after its last sweep to the next
    launch (drawn first, while the customer workgroups load) or to a flush before anything reads
    the hyper state or the level-2 records.  Bit for bit the same run as without deferral
    (CLV_DEFER=0) and as the launch-per-sweep path, over uneven clv_run calls including 1-sweep
    calls, with get_state between calls (a flush mid-run), and through clv_rollback at world size 1
    (undo a completed call and redo it; also after a flush)."""
    from mcmc_clv_model_amd.sampler import build_problem
    p = build_problem(cdnow("full", 23570), covs, D)
    kw = dict(mcmc=22, burnin=5, thin=2, chains=2, seed=77, draw_sink=sink)
    ops = [("run", 1), ("run", 1), ("run", 6), ("state",), ("run", 3), ("run", 1), ("state",), ("run", 15)]
    ref = _run_ops(p, {"CLV_PERSISTENT": "0"}, ops, **kw)
    nodef = _run_ops(p, {"CLV_PERSISTENT": "1", "CLV_DEFER": "0"}, ops, **kw)
    dfr = _run_ops(p, {"CLV_PERSISTENT": "1", "CLV_DEFER": "1"}, ops, **kw)
    assert not ref[0]["persistent"] and nodef[0]["persistent"] and dfr[0]["persistent"]
    _same_bits(ref[1:], nodef[1:])
    _same_bits(ref[1:], dfr[1:])
    # rollback of a deferred call (pending draw in, pending draw out), and after a flush
    rb = [("run", 4), ("run", 5), ("rollback",), ("run", 5), ("run", 3), ("state",), ("rollback",), ("run", 3),
          ("run", 15)]
    straight = [("run", 4), ("run", 5), ("run", 3), ("state",), ("run", 15)]
    a = _run_ops(p, {"CLV_PERSISTENT": "1", "CLV_DEFER": "1"}, rb, **kw)
    b = _run_ops(p, {"CLV_PERSISTENT": "1", "CLV_DEFER": "1"}, straight, **kw)
    _same_bits(a[1:], b[1:])


def _mh_step_device(L, f, t3, log_u, cur_pt=None):
    """clv_debug_mh_step over formulas.npz's log-posterior inputs (G1, bi:291-310); log_u is log2 U."""
    n = f["lp_ll"].size
    S = f["lp_S"]
    P = np.linalg.inv(S)
    x = np.ascontiguousarray(f["lp_x"], dtype=np.int32)
    z = np.ascontiguousarray(f["lp_z"], dtype=np.uint8)
    T = np.ascontiguousarray(f["lp_T"], dtype=np.float64)
    tau = np.ascontiguousarray(f["lp_tau"], dtype=np.float64)
    m = np.ascontiguousarray(f["lp_mv"], dtype=np.float64)
    prec = np.array([P[0, 0], P[0, 1], P[1, 1]])
    cur = np.ascontiguousarray(np.column_stack([f["lp_ll"], f["lp_lm"]]) if cur_pt is None else cur_pt)
    scale = np.array([S[0, 0], S[1, 1]])
    out = np.zeros((n, 7))
    rc = L.clv_debug_mh_step(n, x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                             z.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _dp(T), _dp(tau), _dp(m), _dp(prec),
                             _dp(cur), _fp(np.ascontiguousarray(t3, dtype=np.float32)), _dp(scale),
                             _fp(np.ascontiguousarray(log_u, dtype=np.float32)), _dp(out))
    assert rc == 0
    return out


def test_device_mh_step_matches_reference_log_posterior(L):
    """The SHIPPED Philox-mode MH step (log_post_fast, fma + clip proposal, accept iff pm <= 5 and
    plp > cur + log U) on formulas.npz's log-posterior inputs, which include the reference's edge
    cases: lm > 5 -> lp = -inf (quirk Q3, bi:309) and -inf - -inf = NaN (never accepted, bi:329-330).
    Checked against the reference's log posterior (the oracle, bitwise = bi:291-310):
      * lp differences plp - cur equal the reference's within 1e-12 of the terms' magnitude;
      * current points with lm > 5 have cur = -inf; proposals with pm > 5 are never accepted;
      * accept decisions equal the reference's exp(lp' - lp) > U (U = exp(log U)) wherever the
        margin |lp' - lp - log U| exceeds the arithmetic tolerance (about half the lanes are placed
        close to their margin on purpose);
      * every accepted lane carries exactly (pl, pm, plp), every rejected lane exactly its input;
      * a padded step (log U = +inf) never accepts, also from a cur = -inf point."""
    from oracle import ref_cpu as orc
    f = golden("formulas.npz")
    n = f["lp_ll"].size
    rng = np.random.default_rng(2024)
    t3 = rng.standard_t(3, (n, 2)).astype(np.float32)
    P = np.linalg.inv(f["lp_S"])
    args = (f["lp_x"], f["lp_z"], f["lp_T"], f["lp_tau"], f["lp_mv"], P)
    # first pass only to get the device's proposals; log U chosen after from the reference's deltas
    out0 = _mh_step_device(L, f, t3, np.full(n, np.inf, np.float32))
    pl, pm = out0[:, 2], out0[:, 3]
    assert np.array_equal(out0[:, 4], f["lp_ll"]) and np.array_equal(out0[:, 5], f["lp_lm"])  # +inf: no accept
    ref_pl = np.clip(f["lp_ll"] + f["lp_S"][0, 0] * t3[:, 0].astype(np.float64), -70.0, 70.0)
    np.testing.assert_allclose(pl, ref_pl, rtol=1e-15, atol=1e-13)  # fma vs two roundings
    with np.errstate(over="ignore", invalid="ignore"):
        lp_cur = orc.log_posterior(f["lp_ll"], f["lp_lm"], *args)
        lp_prop = orc.log_posterior(pl, pm, *args)
        d_ref = lp_prop - lp_cur
    assert np.array_equal(bits(lp_cur), bits(f["lp_out"]))  # the oracle is the reference here
    # log U: half the lanes near the margin (d_ref + small offset), half uniform log U
    lu = np.log(rng.random(n)).astype(np.float32)
    near = (rng.random(n) < 0.5) & np.isfinite(d_ref) & (np.abs(d_ref) < 50)
    lu[near] = (np.minimum(d_ref[near], 0.0) + rng.choice([-1, 1], near.sum()) * 10.0 ** rng.uniform(-6, -1, near.sum())
                ).astype(np.float32)
    lu = np.minimum(lu, np.float32(-1e-30))  # log U < 0 (U < 1)
    # the step takes log2 U (fp32) and forms cur + ln2 log2 U in fp64: the reference sees that log U
    lu2 = (lu.astype(np.float64) / np.log(2.0)).astype(np.float32)
    lu = lu2.astype(np.float64) * np.log(2.0)
    out = _mh_step_device(L, f, t3, lu2)
    cur, plp = out[:, 0], out[:, 1]
    # Q3 on the current point
    assert np.all(np.isneginf(cur[f["lp_lm"] > 5.0])) and np.all(np.isfinite(cur[f["lp_lm"] <= 5.0]))
    # lp differences
    ll, lm = f["lp_ll"], f["lp_lm"]
    w = np.where(f["lp_z"], f["lp_T"], f["lp_tau"])
    mv = f["lp_mv"]
    quad = lambda a, b: (np.abs(a - mv[:, 0]) + np.abs(b - mv[:, 1])) ** 2 * np.abs(P).max()  # noqa: E731
    mag = (np.abs(f["lp_x"] * ll) + np.abs(f["lp_x"] * pl) + np.abs(lm) + np.abs(pm)
           + w * (np.exp(np.minimum(ll, 700)) + np.exp(np.minimum(lm, 700)) + np.exp(pl) + np.exp(pm))
           + quad(ll, lm) + quad(pl, pm) + np.abs(mv).sum(1) ** 2 * np.abs(P).max() + 1.0)
    fin = (lm <= 5.0) & (pm <= 5.0)
    d_dev = plp - cur
    err = np.abs(d_dev[fin] - d_ref[fin])
    assert np.all(err <= 1e-12 * mag[fin]), (err / mag[fin]).max()
    # accept decisions
    with np.errstate(over="ignore", invalid="ignore"):
        acc_ref = np.exp(d_ref) > np.exp(lu.astype(np.float64))
    acc_dev = (out[:, 4] == pl) & (out[:, 5] == pm) & (out[:, 6] == plp)
    rej_dev = (out[:, 4] == ll) & (out[:, 5] == lm) & (bits(out[:, 6]) == bits(cur))
    assert np.all(acc_dev | rej_dev)
    margin = np.abs(d_ref - lu.astype(np.float64))
    clear = ~(np.isfinite(margin) & (margin <= 1e-12 * mag))
    assert clear.sum() > 0.95 * n
    assert np.array_equal(acc_dev[clear & ~(acc_dev & rej_dev)], acc_ref[clear & ~(acc_dev & rej_dev)])
    assert not np.any(acc_dev & (pm > 5.0) & ~rej_dev)                 # capped proposals never taken
    both_inf = (lm > 5.0) & (pm > 5.0)                                # reference: NaN ratio -> reject
    assert both_inf.sum() > 0 and not np.any(acc_ref[both_inf]) and np.all(rej_dev[both_inf])
    from_inf = (lm > 5.0) & (pm <= 5.0)                               # reference: +inf ratio -> accept
    assert from_inf.sum() > 0 and np.all(acc_ref[from_inf]) and np.all(acc_dev[from_inf])
    assert 0.05 * n < acc_dev.sum() < 0.95 * n
    # padded steps from cur = -inf points: thr = -inf + inf = NaN, never accepted
    out2 = _mh_step_device(L, f, t3, np.full(n, np.inf, np.float32))
    assert np.array_equal(out2[:, 4], ll) and np.array_equal(out2[:, 5], lm)

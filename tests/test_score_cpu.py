"""Scoring customers outside the fit, without a device: the C ABI's declarations and argument checks,
the validation of the Python layer, and the float64 model (tests/score_ref.py) on its own — its
variates against oracle.philox, its borderline count and coverage events at exactly the shapes
tests/test_gpu_score.py compares, the quadrature's grid doubling and the model-alone run of the
distribution test, whose bound (5 MCSE, 192 comparisons, fixed seed) is thereby known to hold
before a GPU is involved.

Measured (model alone, the distribution test's seeds): largest |mean - quadrature| / MCSE 2.4 / 2.3
(log lambda / log mu, bivariate K = 2) and 3.8 / 2.3 (trivariate K = 3); doubling the 401 x 401 grid
moves no mean by more than 6e-11.
"""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from tests import philox_sweep_ref as M
from tests import score_ref as R

NEW_SYMBOLS = ("clv_score_customers", "clv_score_customers_sampler", "clv_score_info", "clv_debug_score_hyper")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")


def test_header_declares_and_library_exports_the_new_symbols():
    from mcmc_clv_model_amd import _lib
    import mcmc_clv_model_amd as pkg
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    with open(HDR) as f:
        text = f.read()
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert "score_customers" in pkg.__all__ and callable(pkg.score_customers)
    for cite in ("bi:193-227", "bi:268-339", "tri:306-333"):
        assert cite in text[text.index("Scoring customers outside the fit"):text.index("int clv_score_info")]


def test_info_reports_the_block_and_the_sum_stats():
    from mcmc_clv_model_amd import _lib
    info = _lib.score_info()
    assert info["block"] == 256 == _lib.BLOCK and info["n_sum_stats"] == _lib.N_SUM_STATS == len(R.SUM_STATS)
    assert _lib.SUM_STATS == R.SUM_STATS and _lib.SUMMARY_MU_CAP == R.MU_CAP_SUMMARY
    inst = [info[k] for k in ("D", "K", "sink", "vgprs", "scratch_bytes", "kernel_ns")]
    # no scoring call on this thread yet (-1 throughout), or the instance the last one launched
    assert all(v == -1 for v in inst) or (info["D"] in (2, 3) and 1 <= info["K"] <= 9 and info["vgprs"] > 0)
    assert _lib.lib().clv_score_info(None) == -1


# ---- the C ABI's argument checks: -1 before any device call ---------------------------------------
ORDER = ("device", "D", "K", "n_chains", "n_draws", "level2", "n", "x", "t_x", "T_cal", "cov", "log_s", "omega2",
         "n_mh_steps", "warmup", "inner_sweeps", "seed", "chain_first", "customer_offset", "sweep_first", "init_lam",
         "init_mu", "sink", "level1_out", "sums_out", "state_lam_out", "state_mu_out")


def _c_args(D=3, K=2, C=2, nd=3, n=4):
    from mcmc_clv_model_amd._lib import dptr
    rng = np.random.default_rng(1)
    a = dict(level2=np.ascontiguousarray(R.synth_level2(D, K, C, nd, 3)), x=np.arange(n, dtype=np.int32),
             t_x=np.linspace(0.0, 30.0, n), T_cal=np.full(n, 39.0), cov=rng.uniform(-1, 1, (K - 1, n)),
             log_s=rng.normal(3.0, 0.5, n), init_lam=np.full((C, n), 0.05), init_mu=np.full((C, n), 0.02),
             level1_out=np.empty((C, nd, n, D + 2)), sums_out=np.empty((C, 11, n)), state_lam_out=np.empty((C, n)),
             state_mu_out=np.empty((C, n)))
    ptr = {k: (v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if k == "x" else dptr(v)) for k, v in a.items()}
    ptr.update(device=0, D=D, K=K, n_chains=C, n_draws=nd, n=n, omega2=0.3, n_mh_steps=20, warmup=2, inner_sweeps=2,
               seed=7, chain_first=0, customer_offset=0, sweep_first=1, sink=0)
    return a, ptr


def _poke(name, index, value):
    def f(arrays):
        arrays[name].flat[index] = value
    return f


BAD = [dict(level2=None), dict(x=None), dict(t_x=None), dict(T_cal=None), dict(init_lam=None), dict(init_mu=None),
       dict(state_lam_out=None), dict(state_mu_out=None), dict(n=0), dict(n=-3), dict(n_chains=0), dict(n_draws=0),
       dict(D=1), dict(D=4), dict(K=0), dict(K=10),
       dict(cov=None),                                       # K = 2 without covariates
       dict(K=1),                                            # covariates given for K = 1
       dict(log_s=None),                                     # D = 3 without log_s
       dict(D=2),                                            # log_s given for D = 2
       dict(omega2=0.0), dict(omega2=-1.0), dict(omega2=float("nan")), dict(omega2=float("inf")),
       dict(inner_sweeps=0), dict(inner_sweeps=-1), dict(warmup=-1), dict(n_mh_steps=-1), dict(chain_first=-1),
       dict(sink=2), dict(sink=3), dict(sink=-1),
       dict(level1_out=None),                                # the full sink with nowhere to put it
       dict(sink=1, sums_out=None),
       dict(customer_offset=-1), dict(customer_offset=(1 << 32) - 3),          # offset + n beyond 32 bits
       dict(sweep_first=0), dict(sweep_first=1 << 32), dict(sweep_first=(1 << 32) - 7),  # 2 + 2 * 3 sweeps: the last would be 2^32
       dict(n_draws=1 << 31, inner_sweeps=2),                                   # (checked before the records are read)
       dict(poke=_poke("init_lam", 1, 0.0)), dict(poke=_poke("init_mu", 2, -1.0)), dict(poke=_poke("init_lam", 0, np.nan)),
       dict(poke=_poke("init_mu", 3, np.inf)), dict(poke=_poke("init_lam", 0, 1e-320)),
       dict(poke=_poke("t_x", 1, 40.0)),                     # t_x > T_cal
       dict(poke=_poke("t_x", 0, -1.0)), dict(poke=_poke("x", 2, -1)), dict(poke=_poke("T_cal", 0, np.nan)),
       dict(poke=_poke("t_x", 3, np.inf)), dict(poke=_poke("cov", 0, np.nan)), dict(poke=_poke("log_s", 1, np.inf)),
       dict(poke=_poke("level2", 4, np.nan)),
       dict(poke=_poke("level2", 6, -0.5))]                  # Sigma_00 of record 0 (D K = 6 betas come first)


def _bad_id(b):
    return "-".join(f"{k}={'poke' if callable(v) else v}" for k, v in b.items())


@pytest.mark.parametrize("bad", BAD, ids=_bad_id)
def test_c_abi_rejects_bad_arguments(bad):
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    arrays, a = _c_args()
    for k, v in bad.items():
        if k == "poke":
            v(arrays)
        else:
            a[k] = v
    assert L.clv_score_customers(*[a[k] for k in ORDER]) == -1
    assert L.clv_last_error()


def test_c_abi_accepts_the_good_call_up_to_the_device():
    """The unmodified arguments pass every check: without a device the call fails with a HIP error,
    not an argument error (so the rejections above are the arguments')."""
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    _, a = _c_args()
    rc = L.clv_score_customers(*[a[k] for k in ORDER])
    assert rc == 0 if _lib.device_count() >= 1 else rc == -2


def test_c_abi_rejects_the_rest():
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    _, a = _c_args()
    tail = [a[k] for k in ORDER[ORDER.index("n"):] if k not in ("omega2", "chain_first")]
    assert L.clv_score_customers_sampler(None, *tail) == -1
    out = np.empty(64)
    assert L.clv_debug_score_hyper(0, 2, 1, 1, None, 1.0, _lib.dptr(out)) == -1
    assert L.clv_debug_score_hyper(0, 3, 1, 1, _lib.dptr(out), 0.0, _lib.dptr(out)) == -1
    assert L.clv_debug_score_hyper(0, 2, 1, 0, _lib.dptr(out), 1.0, _lib.dptr(out)) == -1


# ---- the Python layer ------------------------------------------------------------------------------
def _py_case(D=2, K=2, n=5):
    df = pd.DataFrame(dict(x=np.arange(n), t_x=np.linspace(0, 30, n), T_cal=np.full(n, 39.0), c1=np.linspace(-1, 1, n),
                           log_s=np.linspace(2, 4, n)))
    return {"level_2": list(R.synth_level2(D, K, 2, 3, 5))}, df, ["c1"][:K - 1]


@pytest.mark.parametrize("kw", [
    dict(inner_sweeps=0), dict(warmup=-1), dict(n_mh_steps=-1), dict(sink="none"), dict(sink="summary+pct"),
    dict(customer_offset=-1), dict(customer_offset=1 << 32), dict(sweep_first=0), dict(sweep_first=1 << 32),
    dict(chain_first=-1), dict(omega2=0.3),                              # omega2 with a bivariate fit
    dict(init=(np.ones((2, 4)), np.ones((2, 4)))),                       # init of the wrong shape
    dict(init=(np.zeros((2, 5)), np.ones((2, 5)))), dict(init=(np.ones((2, 5)), np.full((2, 5), np.nan))),
    dict(covariates=[]),                                                 # width 7 is no model with K = 1
    dict(covariates=["c1", "nope"]),
])
def test_score_customers_rejects_bad_arguments_without_a_device(kw):
    from mcmc_clv_model_amd import score_customers
    draws, df, covs = _py_case()
    args = dict(covariates=covs)
    args.update(kw)
    with pytest.raises(ValueError):
        score_customers(draws, df, **args)


def test_score_customers_rejects_bad_inputs_without_a_device():
    from mcmc_clv_model_amd import score_customers
    draws, df, covs = _py_case()
    with pytest.raises(ValueError):
        score_customers({"level_2": None}, df, covs)
    with pytest.raises(ValueError):
        score_customers({"level_2": [np.zeros((3, 7)), np.zeros((2, 7))]}, df, covs)      # chains of unequal length
    with pytest.raises(ValueError):
        score_customers(draws, df.drop(columns="t_x"), covs)
    with pytest.raises(ValueError):
        score_customers(draws, df.iloc[:0], covs)
    with pytest.raises(ValueError):
        score_customers(draws, df.assign(x=-df["x"] - 1), covs)
    tri, df3, covs3 = _py_case(D=3)
    with pytest.raises(ValueError):
        score_customers(tri, df3.drop(columns="log_s"), covs3)
    for w2 in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            score_customers(tri, df3, covs3, omega2=w2)
    with pytest.raises(ValueError):
        score_customers(tri, df3.iloc[:1], covs3)                                        # no default omega2 from one customer


def test_python_default_init_is_the_models():
    from mcmc_clv_model_amd import analysis as A
    case = R.CASES["tri3"]
    sp, l2 = R.case_problem(case), R.case_level2(case)
    D, K, x, t_x, T_cal, cov, log_s = A.score_problem(sp.df, sp.covs, l2.shape[-1])
    assert (D, K) == (3, 3) and np.array_equal(cov.T, sp.X[:, 1:]) and np.array_equal(log_s, sp.log_s)
    lam, mu = A.score_init(l2, D, K, cov, sp.N, None)
    ref = R.default_init(l2, sp.X, D, K)
    np.testing.assert_allclose(lam, ref[0], rtol=1e-14)
    np.testing.assert_allclose(mu, ref[1], rtol=1e-14)
    # per customer: a customer's start does not depend on who else is in the batch
    sub = A.score_init(l2, D, K, np.ascontiguousarray(cov[:, 100:110]), 10, None)
    np.testing.assert_allclose(sub[0], lam[:, 100:110], rtol=1e-14)


# ---- the model on its own ---------------------------------------------------------------------------
def test_model_variates_are_the_oracles():
    a = R.variates_at(5, 1, 3, 10 + np.arange(7), 6)
    b = M.oracle_variates(5, 1, 3, 17, 6)
    for k in a:
        assert np.array_equal(a[k], b[k][..., 10:]), k
    blk = R._variates_block(5, 1, [3, 4], 10 + np.arange(7), 6)
    c = R.variates_at(5, 1, 4, 10 + np.arange(7), 6)
    for k in a:
        assert np.array_equal(blk[k][0], a[k]) and np.array_equal(blk[k][1], c[k]), k


def test_synthetic_records_carry_the_planted_ones():
    for D, K in ((2, 1), (3, 4)):
        l2 = R.synth_level2(D, K, 2, 4, 9)
        assert l2.shape == (2, 4, D * K + D * (D + 1) // 2)
        for c in range(2):
            _, big = M.l2_unpack(l2[c, 1], D, K)
            _, corr = M.l2_unpack(l2[c, 2], D, K)
            assert abs(big[1, 1] - 40.0) < 1e-9
            assert abs(corr[0, 1] / np.sqrt(corr[0, 0] * corr[1, 1]) - 0.99) < 1e-12
            beta, Sigma = M.l2_unpack(l2[c, 0], D, K)
            assert np.array_equal(M.l2_record(beta, Sigma), l2[c, 0]) and np.linalg.eigvalsh(Sigma).min() > 0
            assert abs(beta[0, 0] - np.log(0.05)) < 0.6


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_borderline_count_and_coverage_at_the_gpu_shapes(name):
    """The model run freely at exactly the GPU cases' shapes, one call per record as the GPU module
    drives the device: lanes within RTOL of a decision (expected: none; at most BORDERLINE_CAP) and
    the coverage events of score_ref.COVERAGE among the clear lanes."""
    case = R.CASES[name]
    sp, l2 = R.case_problem(case), R.case_level2(case)
    assert (sp.N, sp.K, sp.D, l2.shape[:2]) == (case["N"], case["K"], case["D"], (case["chains"], case["records"]))
    lam0, mu0 = R.default_init(l2, sp.X, sp.D, sp.K)
    lanes = aside = 0
    ev = dict.fromkeys(("hit_cap", "hit_clip", "z0", "z1"), 0)
    for c in range(case["chains"]):
        lam, mu, t = lam0[c], mu0[c], 1
        for d in range(case["records"]):
            r = R.run_chain(sp, l2[c, d:d + 1], lam, mu, seed=case["seed"], chain=case["chain_first"] + c, S=case["S"],
                            inner=case["R"], sweep_first=t, offset=case["offset"])
            lam, mu, t = r["lam"], r["mu"], r["next_sweep"]
            clear = r["margin"] > M.RTOL
            lanes += sp.N
            aside += int((~clear).sum())
            for k in ev:
                ev[k] += int((clear & r[k]).sum())
            assert np.isfinite(r["level1"]).all() and (r["level1"][..., 1] <= np.exp(M.MU_CAP)).all()
    print(f"{name}: {lanes} lanes, {aside} borderline; {ev}")
    assert t == 1 + case["records"] * case["R"]
    assert aside <= M.BORDERLINE_CAP * lanes
    for k in R.COVERAGE[name]:
        assert ev[k] > 0, k
    assert case["offset"] + case["N"] > 65536 or name != "bi5"


def test_one_call_is_the_record_by_record_continuation_in_the_model():
    case = R.CASES["tri3"]
    sp, l2 = R.case_problem(case), R.case_level2(case)
    lam0, mu0 = R.default_init(l2, sp.X, sp.D, sp.K)
    kw = dict(seed=case["seed"], chain=0, S=case["S"], inner=case["R"])
    whole = R.run_chain(sp, l2[0], lam0[0], mu0[0], warmup=2, **kw)
    wu = R.run_chain(sp, l2[0, :1], lam0[0], mu0[0], **dict(kw, inner=2))
    cont = R.run_chain(sp, l2[0], wu["lam"], wu["mu"], sweep_first=3, **kw)
    assert np.array_equal(whole["level1"], cont["level1"]) and whole["next_sweep"] == cont["next_sweep"]
    sums = R.summary_sums(whole["level1"])
    assert sums.shape == (11, sp.N) and np.allclose(sums[0], whole["level1"][..., 0].sum(0), rtol=1e-13)


def test_quadrature_is_converged():
    """Doubling the grid moves each posterior mean by less than 1e-6."""
    for name in R.DIST_MODELS:
        a, b = R.dist_quadrature(name, 401), R.dist_quadrature(name, 801)
        move = np.abs(a - b)[:, :3].max(axis=0)
        print(f"{name}: grid 401 -> 801 moves E log lambda, E log mu, E P(alive) by at most {move}")
        assert (move < 1e-6).all()
        assert (a[:, 2] > 0).all() and (a[:, 2] <= 1).all() and (a[:, 3:] > 0).all()


@pytest.mark.parametrize("name", list(R.DIST_MODELS))
def test_model_alone_meets_the_distribution_bound(name):
    """The float64 model with the distribution test's seeds: every customer's mean of log lambda, log
    mu and P(alive) within 5 MCSE of the quadrature (the GPU module asserts the same of the device)."""
    sp, rec, l1 = R.model_dist_run(name)
    assert l1.shape == (4, 2000, 64, sp.D + 2) and np.isfinite(l1).all()
    diff, mcse = R.dist_check(R.dist_series(l1, sp), R.dist_quadrature(name))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(mcse > 0, diff / mcse, 0.0)
    print(f"{name}: model alone, largest |mean - quadrature| / MCSE: log lambda {z[0].max():.2f}, log mu {z[1].max():.2f}, "
          f"P(alive) {z[2].max():.2f}; series that never move: {(mcse == 0).sum()}")
    assert R.dist_ok(diff, mcse).all(), np.argwhere(~R.dist_ok(diff, mcse))

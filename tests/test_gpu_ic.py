"""WAIC and PSIS-LOO on the GPU (csrc/ic.hip) against 40-digit mpmath (tests/ic_ref.py mp_*) and
the float64 model of the same file.

Tolerances (tests/test_ic_cpu.py measures E_L = 7e-16 and E_STAT = 8e-16, the model's deviation from
mpmath on its 64 x 100 fixtures): the device may deviate from mpmath by 4 E_L relative in the
pointwise log-likelihood, with a floor of 4 ulp of the largest term where the terms cancel
(ic_ref.loglik_scale), and by 4 E_STAT in the statistics — relative for lppd, p_waic and elpd_loo,
absolute for pareto_k, and for the two differences elpd_waic = lppd - p_waic and p_loo = lppd -
elpd_loo relative to the sum of their operands' magnitudes.  The factor covers an equally accurate
but different exp / log and nothing more.

What is held to mpmath: every log-likelihood value of every case but N = 600 x S = 100, where it is
draws 0 .. 7 (they hold every extreme row) and every 4th draw after them, the remaining values being
held to the model at 3 E_L (which implies 4 E_L against mpmath where the model is within E_L of it);
every row of the statistics at S <= 100, and at S = 1000 the planted series, their neighbours and
every 8th customer (mpmath takes 0.15 s per row there).  The S = 1000 rows left over are compared
with the model at 8 E_STAT: a guard against a gross error on those rows, not the issue's bound (the
model's own pareto_k is up to 1.9 E_STAT from mpmath on these matrices).  tail_len, the customers
with pareto_k = +inf and the NaN rows are equal exactly on every row.

Measured on an MI355X, as a fraction of the 4 x bound: the log-likelihood at most 0.26; lppd 0.36,
p_waic 0.11, elpd_waic 0.36, elpd_loo 0.28, p_loo 0.16, pareto_k 0.49."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from tests import ic_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu

E_L, E_STAT, ULP = R.E_L, R.E_STAT, R.ULP
MP_ENTRIES = 30000          # log-likelihood values one case evaluates in mpmath in full
TIED, CONST, DOMINANT, INF_ROW = R.TIED, R.CONST, R.DOMINANT, 7


def mp_rows(S):
    if S <= 100:
        return tuple(range(257))
    return tuple(sorted({TIED, CONST, DOMINANT, INF_ROW - 1, INF_ROW + 1} | set(range(0, 257, 8))))


COL = {c: j for j, c in enumerate(R.STATS)}


def _draws(l1):
    return {"level_1": [l1]}


# ---- the pointwise log-likelihood ------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 5])
@pytest.mark.parametrize("S", [8, 100])
@pytest.mark.parametrize("N", [1, 255, 257, 600])
def test_loglik_kernel_against_the_model(N, S, width):
    from mcmc_clv_model_amd.analysis import pointwise_log_likelihood
    spend = width == 5
    l1, d = R.synth_case(S, N, width, seed=100 + N, extremes=True)
    w2 = 0.37 if spend else None
    kw = dict(spend=True, omega2=w2) if spend else {}
    dev = pointwise_log_likelihood(_draws(l1), pd.DataFrame(d), **kw)
    ref = R.loglik(l1, d, spend, w2)
    scale = R.loglik_scale(l1, d, spend, w2)
    assert dev.shape == (S, N) and np.isfinite(dev).all() and np.isfinite(ref).all()
    draws = list(range(S)) if N * S <= MP_ENTRIES else list(range(8)) + list(range(8, S, 4))
    mp = R.mp_loglik_matrix(l1[draws], d, spend, w2)
    worst = 0.0
    for r, s in enumerate(draws):
        for i in range(N):
            err, want = R.abs_dev(dev[s, i], mp[r, i]), abs(float(mp[r, i]))
            bound = max(4 * E_L * want, 4 * ULP * scale[s, i])
            worst = max(worst, err / bound)
    rest = np.setdiff1d(np.arange(S), draws)
    vs_model = np.abs(dev - ref) / np.maximum(3 * E_L * np.abs(ref), 3 * ULP * scale)
    print(f"N={N} S={S} width={width}: largest deviation from mpmath / its bound {worst:.3g} over {len(draws)} draws; "
          f"from the model / its bound {vs_model[rest].max() if len(rest) else 0.0:.3g} over the other {len(rest)}")
    assert worst <= 1.0
    assert np.all(vs_model[rest] <= 1.0)
    if spend:   # spend=False on the trivariate draws: the bivariate kernel path on the same columns
        tx = pointwise_log_likelihood(_draws(l1), pd.DataFrame(d))
        tx4 = pointwise_log_likelihood(_draws(np.ascontiguousarray(l1[..., :4])), pd.DataFrame(d))
        assert np.array_equal(bits(tx), bits(tx4))


# ---- clv_psis_loo from the model's own matrix ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def psis_case(S):
    """(matrix with the planted series, the same with the +inf row, model, mpmath on mp_rows(S))."""
    ll = R.planted_matrix(S, 257, seed=40 + S)
    bad = ll.copy()
    bad[S // 2, INF_ROW] = np.inf
    ll.setflags(write=False)
    bad.setflags(write=False)
    model = R.model(ll)
    mp = {i: R.mp_stats(ll[:, i]) for i in mp_rows(S)}
    return ll, bad, model, mp


def stat_tolerance(ref, factor):
    """[N][7] absolute tolerance of each column from the reference values (see the module docstring)."""
    a = np.abs(ref)
    tol = factor * E_STAT * a
    tol[:, COL["elpd_waic"]] = factor * E_STAT * (a[:, COL["lppd"]] + a[:, COL["p_waic"]])
    tol[:, COL["p_loo"]] = factor * E_STAT * (a[:, COL["lppd"]] + a[:, COL["elpd_loo"]])
    tol[:, COL["pareto_k"]] = factor * E_STAT
    tol[:, COL["tail_len"]] = 0.0
    return tol


def assert_stats(dev, model, mp):
    """dev against mpmath (mp: row -> ic_ref.mp_stats) at 4 E_STAT on the rows mp holds, against the
    model at 8 E_STAT on the others (a guard, see the module docstring); the exact columns on all."""
    fin = np.isfinite(model[:, COL["pareto_k"]])
    assert np.array_equal(dev[:, COL["tail_len"]], model[:, COL["tail_len"]])
    assert np.array_equal(np.isposinf(dev[:, COL["pareto_k"]]), ~fin) and not np.isnan(dev).any()
    worst = dict.fromkeys(R.STATS[:6], 0.0)
    for i, r in mp.items():
        want = dict(lppd=r["lppd"], p_waic=r["p_waic"], elpd_waic=r["lppd"] - r["p_waic"], elpd_loo=r["elpd_loo"],
                    p_loo=r["lppd"] - r["elpd_loo"], pareto_k=r["pareto_k"])
        t = stat_tolerance(np.array([[float(want[c]) for c in R.STATS[:6]] + [r["tail_len"]]]), 4)[0]
        assert dev[i, COL["tail_len"]] == r["tail_len"] and (r["pareto_k"] == np.inf) == (not fin[i])
        for c in R.STATS[:6]:
            if c == "pareto_k" and not fin[i]:
                continue
            err = R.abs_dev(dev[i, COL[c]], want[c])
            if t[COL[c]] > 0:
                worst[c] = max(worst[c], err / t[COL[c]])
            else:
                assert err == 0.0, (i, c)
    print("  largest deviation from mpmath / (4 E_STAT x scale) over", len(mp), "rows:",
          {c: f"{v:.3g}" for c, v in worst.items()})
    rest = np.setdiff1d(np.arange(len(model)), list(mp))
    if len(rest):
        tol = stat_tolerance(model, 8)
        err = np.abs(dev - model)
        err[~fin, COL["pareto_k"]] = 0.0
        assert np.all(err[rest] <= tol[rest])
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("S", [8, 20, 25, 100, 1000])
def test_psis_loo_from_the_models_matrix(S):
    from mcmc_clv_model_amd.analysis import psis_loo
    ll, bad, model, mp = psis_case(S)
    out = psis_loo(ll)
    dev = out["pointwise"].to_numpy()
    assert list(out["pointwise"].columns) == list(R.STATS) and dev.shape == (257, 7)
    M = R.tail_max(S)
    # what the planted series are there for
    assert model[TIED, COL["tail_len"]] == max(M - 2, 0) and model[CONST, COL["tail_len"]] == 0
    assert model[CONST, COL["pareto_k"]] == np.inf and dev[CONST, COL["p_waic"]] == 0.0
    if M < R.MIN_FIT:
        assert np.isposinf(model[:, COL["pareto_k"]]).all()
    else:
        assert np.isfinite(np.delete(model[:, COL["pareto_k"]], [TIED, CONST])).all()
    if S >= 100:
        assert model[DOMINANT, COL["pareto_k"]] > 0.7 and dev[DOMINANT, COL["pareto_k"]] > 0.7
    assert_stats(dev, model, mp)
    loo = out["loo"].iloc[0]
    assert loo["n_samples"] == S and loo["n_data_points"] == 257
    assert loo["n_bad_k"] == np.count_nonzero(model[:, COL["pareto_k"]] > R.bad_k_threshold(S))
    # a series holding +inf: its row is NaN, its neighbours are untouched
    devb = psis_loo(bad)["pointwise"].to_numpy()
    assert np.isnan(devb[INF_ROW]).all()
    keep = np.arange(257) != INF_ROW
    assert np.array_equal(bits(devb[keep]), bits(dev[keep]))
    assert np.isnan(psis_loo(bad)["loo"].iloc[0]["elpd"])


def test_reff_sets_the_tail():
    from mcmc_clv_model_amd.analysis import psis_loo
    ll = psis_case(1000)[0]
    for reff in (0.25, 4.0):
        dev = psis_loo(ll, reff=reff)["pointwise"].to_numpy()
        assert dev[0, COL["tail_len"]] == R.tail_max(1000, reff)
        assert_stats(dev, R.model(ll, reff), {i: R.mp_stats(ll[:, i], reff) for i in (0, DOMINANT, 64, 128)})


# ---- the fused entry, batching and geometry --------------------------------------------------------
def _c_call(name, l1, d, spend, w2, reff=1.0, extra=()):
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import check, dptr
    S, N, w = l1.shape
    out = np.empty((N, 7), np.float64)
    x = np.ascontiguousarray(d["x"], np.int32)
    check(getattr(_lib.lib(), name)(-1, dptr(l1), S, N, w, x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    dptr(d["t_x"]), dptr(d["T_cal"]), dptr(d["log_s"]) if spend else None,
                                    w2 if spend else 0.0, reff, *extra, dptr(out)))
    return out


@pytest.mark.parametrize("width", [4, 5])
def test_fused_entry_equals_the_two_steps(width):
    from mcmc_clv_model_amd import analysis as A
    spend = width == 5
    l1, d = R.synth_case(100, 257, width, seed=9)
    cbs = pd.DataFrame(d)
    kw = dict(spend=True, omega2=0.37) if spend else {}
    ll = A.pointwise_log_likelihood(_draws(l1), cbs, **kw)
    two = A.psis_loo(ll)
    one = A.information_criteria(_draws(l1), cbs, **kw)
    for k in ("pointwise", "waic", "loo"):
        assert list(one[k].columns) == list(two[k].columns)
        assert np.array_equal(bits(one[k].to_numpy(dtype=np.float64)), bits(two[k].to_numpy(dtype=np.float64))), k
    assert np.array_equal(bits(_c_call("clv_information_criteria", l1, d, spend, 0.37)), bits(one["pointwise"].to_numpy()))
    assert_stats(one["pointwise"].to_numpy(), R.model(ll), {i: R.mp_stats(ll[:, i]) for i in range(0, 257, 16)})


def test_batching_and_geometry():
    S, N = 100, 600
    l1, d = R.synth_case(S, N, 5, seed=21)
    base = _c_call("clv_information_criteria", l1, d, True, 0.37)
    assert np.isfinite(base[:, :5]).all()
    one_block = 256 * S                                   # keys of one 256-customer block: 3 batches
    for batch_keys, grid in ((one_block, 0), (1, 0), (2 * one_block, 0), (0, 1), (0, 2), (one_block, 1)):
        out = _c_call("clv_debug_information_criteria", l1, d, True, 0.37, extra=(batch_keys, grid))
        assert np.array_equal(bits(out), bits(base)), (batch_keys, grid)


# ---- the sampler path and the drop-ins -------------------------------------------------------------
RUN = dict(mcmc=100, burnin=20, thin=2, chains=2, seed=5)


def frames_equal(a, b):
    for k in ("pointwise", "waic", "loo"):
        assert list(a[k].columns) == list(b[k].columns)
        assert np.array_equal(bits(a[k].to_numpy(dtype=np.float64)), bits(b[k].to_numpy(dtype=np.float64))), k


@functools.lru_cache(maxsize=None)
def fitted(D, covs):
    """(the drop-in's output with information_criteria, the CBS) of CDNOW's first 300 customers."""
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    df = cdnow("abe", n=300)
    fn = mcmc_draw_parameters_rfm_m if D == 3 else mcmc_draw_parameters
    kw = dict(spend=True) if D == 3 else True
    return fn(df, list(covs), trace=0, information_criteria=kw, **RUN), df


@pytest.mark.parametrize("D,covs", [(2, ("first_sales_scaled",)), (3, ("first_sales_scaled", "gender_F"))])
def test_sampler_path_and_drop_in(D, covs):
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    out, df = fitted(D, covs)
    kw = dict(spend=True) if D == 3 else {}
    p = build_problem(df, list(covs), D=D)
    assert p.K == D
    with HipSampler(p, n_mh_steps=20, **RUN) as s:
        with pytest.raises(_lib.ClvError, match="-3"):       # CLV_ESTATE: the run has not stored its draws
            s.information_criteria()
        s.run(120)
        dev = s.information_criteria(**kw)
        if D == 3:
            tx = s.information_criteria()
        l1, l2, _ = s.read_draws()
    draws = dict(level_1=list(l1), level_2=list(l2))
    host = A.information_criteria(draws, df, **kw)
    frames_equal(dev, host)
    assert dev["pointwise"].shape == (300, 7) and dev["loo"].iloc[0]["n_samples"] == 100
    assert np.isfinite(dev["pointwise"].to_numpy()[:, :5]).all()
    assert np.array_equal(bits(np.stack(out["level_1"])), bits(l1))
    frames_equal(out["information_criteria"], host)
    if D == 3:   # the default omega2 is the sampler's; the transaction part alone differs
        frames_equal(host, A.information_criteria(draws, df, spend=True, omega2=float(np.var(df["log_s"].to_numpy(), ddof=1))))
        frames_equal(tx, A.information_criteria(draws, df))
        assert tx["loo"].iloc[0]["elpd"] != dev["loo"].iloc[0]["elpd"]
    with HipSampler(p, n_mh_steps=20, draw_sink="summary", **RUN) as s:
        s.run(120)
        with pytest.raises(_lib.ClvError, match="-3"):
            s.information_criteria()


def test_drop_in_keyword_routes():
    from mcmc_clv_model_amd import mcmc_draw_parameters
    out, df = fitted(2, ("first_sales_scaled",))
    covs = ["first_sales_scaled"]
    assert "information_criteria" not in mcmc_draw_parameters(df, covs, trace=0, **RUN)
    multi = mcmc_draw_parameters(df, covs, trace=0, information_criteria=True, devices=[0, 0], shard="chains", **RUN)
    frames_equal(multi["information_criteria"], out["information_criteria"])
    with pytest.raises(ValueError):
        mcmc_draw_parameters(df, covs, trace=0, draw_sink="summary", information_criteria=True, **RUN)
    with pytest.raises(ValueError):
        mcmc_draw_parameters(df, covs, trace=0, information_criteria=dict(spend=True), **RUN)


def test_end_to_end_comparison():
    from mcmc_clv_model_amd import mcmc_draw_parameters
    from mcmc_clv_model_amd import analysis as A
    m2, df = fitted(2, ("first_sales_scaled",))
    m1 = mcmc_draw_parameters(df, [], trace=0, information_criteria=True, **RUN)
    ics = {"M1": m1["information_criteria"], "M2": m2["information_criteria"]}
    for crit in ("loo", "waic"):
        cmp = A.compare_models(ics, criterion=crit)
        assert sorted(cmp.index) == ["M1", "M2"] and cmp["elpd_diff"].iloc[0] == 0.0 and cmp["dse"].iloc[0] == 0.0
        assert np.isfinite(cmp[["elpd", "elpd_diff", "dse", "se", "p"]].to_numpy()).all()
        assert cmp["elpd_diff"].iloc[1] >= 0.0 and cmp["dse"].iloc[1] > 0.0
    # the totals against the model on the same draws
    d = dict(x=df["x"].to_numpy(np.int32), t_x=df["t_x"].to_numpy(float), T_cal=df["T_cal"].to_numpy(float))
    for fit in (m1, m2):
        model = R.model(R.loglik(np.concatenate(fit["level_1"]), d))
        ic = fit["information_criteria"]
        n = len(model)
        tol = n * stat_tolerance(model, 4).max(axis=0)
        for name, ecol, pcol in (("waic", "elpd_waic", "p_waic"), ("loo", "elpd_loo", "p_loo")):
            row = ic[name].iloc[0]
            assert abs(row["elpd"] - model[:, COL[ecol]].sum()) <= tol[COL[ecol]], (name, "elpd")
            assert abs(row["p"] - model[:, COL[pcol]].sum()) <= tol[COL[pcol]], (name, "p")
            se = np.sqrt(n * model[:, COL[ecol]].var())
            assert abs(row["se"] - se) <= tol[COL[ecol]], (name, "se")
            assert row["n_samples"] == 100 and row["n_data_points"] == 300

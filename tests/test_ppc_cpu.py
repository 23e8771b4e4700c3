"""Posterior predictive checks (csrc/ppc.hip, analysis.posterior_predictive_check): what needs no
GPU — the ABI, the float64 model of the replicate (tests/ppc_ref.py) against theory, its power to see a
wrong counter layout, the frame builders and the argument checks."""
import ctypes
import functools
import os

import numpy as np
import pandas as pd
import pytest
from scipy import integrate, stats

from tests import ppc_ref as R

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")
NEW_SYMBOLS = ("clv_ppc", "clv_ppc_sampler", "clv_ppc_info", "clv_debug_ppc")


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    import mcmc_clv_model_amd as pkg
    from mcmc_clv_model_amd import _lib, analysis
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    with open(HDR) as f:
        text = " ".join(f.read().split())
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2   # additions only: no bump
    for fn in ("posterior_predictive_check", "ppc_pit"):
        assert fn in analysis.__all__ and fn in pkg.__all__ and callable(getattr(pkg, fn))
    want = ["CLV_PPC_" + c.upper() for c in _lib.PPC_STATS] + ["CLV_N_PPC_STATS"]
    assert "enum { " + want[0] + " = 0, " + ", ".join(want[1:]) + " }" in text
    want = ["CLV_PPC_DRAW_" + c.upper() for c in _lib.PPC_DRAW_INTS] + ["CLV_N_PPC_DRAW_INTS"]
    assert "enum { " + want[0] + " = 0, " + ", ".join(want[1:]) + " }" in text
    assert _lib.PPC_STATS == R.STATS and _lib.PPC_DRAW_INTS == R.DRAW_INTS and _lib.PPC_MAX_K == R.MAX_K
    info = (ctypes.c_int64 * 6)()
    assert L.clv_ppc_info(info) == 0
    assert (info[0], info[1], info[2]) == (_lib.PPC_BLOCK, _lib.PPC_MAX_K, _lib.PPC_BATCH_DOUBLES)
    assert L.clv_ppc_info(None) == -1


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    n, nd = 3, 2
    l1 = np.ones((nd, n, 4))
    l2 = np.ones((nd, 5))
    x = np.zeros(n, np.int32)
    tx, T = np.zeros(n), np.ones(n)
    cu, di, df = np.empty((n, 7)), np.empty((nd, 13), np.int64), np.empty((nd, 1))
    i32 = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    i64 = di.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def call(level=0, l1p=dptr(l1), width=4, l2p=None, D=2, K=1, cov=None, nd_=nd, n_=n, xp=i32, k_hist=8, off=0,
             cup=dptr(cu)):
        return L.clv_ppc(0, level, l1p, width, l2p, D, K, cov, nd_, n_, xp, dptr(tx), dptr(T), k_hist, 1, off, cup,
                         i64, dptr(df), None, None)
    for bad in (dict(level=2), dict(l1p=None), dict(width=3), dict(nd_=0), dict(n_=0), dict(xp=None), dict(k_hist=0),
                dict(k_hist=4097), dict(off=-1), dict(off=(1 << 32) - 2), dict(cup=None),
                dict(level=1, l2p=None), dict(level=1, l2p=dptr(l2), D=4), dict(level=1, l2p=dptr(l2), K=0),
                dict(level=1, l2p=dptr(l2), K=10), dict(level=1, l2p=dptr(l2), K=2)):
        assert call(**bad) == -1, bad
        assert L.clv_last_error()
    assert L.clv_ppc_sampler(None, 0, 8, 1, dptr(cu), i64, dptr(df), None, None) == -1
    head = (0, 0, dptr(l1), 4, None, 2, 1, None, nd, n, i32, dptr(tx), dptr(T), 8, 1, 0, dptr(cu), i64, dptr(df), None,
            None)
    assert L.clv_debug_ppc(*head, -1, 0) == -1 and L.clv_debug_ppc(*head, 0, -1) == -1


# ---- the model alone: borderline cap on the GPU cases ---------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_cases():
    return R.gpu_cases()


@pytest.mark.parametrize("name", ["customer_w4", "customer_w5", "population_21", "population_23", "population_32", "long",
                                  "edge"])
def test_model_borderline_share_on_every_gpu_case(name):
    case = gpu_cases()[name]
    for seed in R.SEEDS:
        m = R.model(case, seed)
        share = float(np.mean(m["margin"] <= R.RTOL))
        print(name, hex(seed), "borderline share", share)
        assert share <= R.BORDERLINE_CAP
        assert (m["t_x_rep"] <= m["L"]).all() or name == "edge"
        assert (m["t_x_rep"][m["x_rep"] > 0] <= np.broadcast_to(case["T_cal"], m["L"].shape)[m["x_rep"] > 0]).all()


# ---- the model against theory ----------------------------------------------------------------------
LAM, MU, T0 = 0.11, 0.035, 39.0
N_TH, D_TH = 4000, 10


@functools.lru_cache(maxsize=None)
def theory_run(seed):
    l1 = np.zeros((D_TH, N_TH, 4))
    l1[..., 0], l1[..., 1] = LAM, MU
    return R.replicate(0, seed, np.zeros(N_TH), np.full(N_TH, T0), level1=l1)


def pmf_theory(k):
    alive = np.exp(-MU * T0) * stats.poisson.pmf(k, LAM * T0)
    dead = integrate.quad(lambda s: MU * np.exp(-MU * s) * stats.poisson.pmf(k, LAM * s), 0.0, T0, epsabs=1e-13)[0]
    return alive + dead


@pytest.mark.parametrize("seed", R.SEEDS)
def test_model_count_frequencies_against_the_closed_form(seed):
    x = theory_run(seed)["x_rep"].ravel()
    top = 12                                           # expected count of the pooled tail is > 5
    p = np.array([pmf_theory(k) for k in range(top)])
    p = np.append(p, 1.0 - p.sum())
    obs = np.bincount(np.minimum(x, top), minlength=top + 1)
    exp = p * x.size
    assert exp.min() > 5.0
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    bound = stats.chi2.ppf(1.0 - 1e-6, top)            # the 1 - 1e-6 quantile, top degrees of freedom
    print("chi2", chi2, "bound", bound)
    assert chi2 < bound


@pytest.mark.parametrize("seed", R.SEEDS)
def test_model_recency_is_the_largest_of_x_uniforms(seed):
    m = theory_run(seed)
    on = m["x_rep"] > 0
    u = (m["t_x_rep"][on] / m["L"][on]) ** m["x_rep"][on]
    ks = stats.kstest(u, "uniform").statistic
    bound = np.sqrt(-0.5 * np.log(1e-6 / 2.0) / u.size)   # Kolmogorov's 1 - 1e-6 quantile (DKW)
    print("ks", ks, "bound", bound, "n", u.size)
    assert ks < bound
    assert (m["t_x_rep"] <= m["L"]).all() and (m["L"] <= T0).all() and (m["t_x_rep"][~on] == 0.0).all()


@pytest.mark.parametrize("seed", R.SEEDS)
def test_model_p_alive(seed):
    a = theory_run(seed)["alive"]
    p = np.exp(-MU * T0)
    se = np.sqrt(p * (1.0 - p) / a.size)
    print("p_alive", a.mean(), "theory", p, "se", se)
    assert abs(a.mean() - p) < 5.0 * se                 # 5 standard errors: two-sided 5.7e-7


@pytest.mark.parametrize("seed", R.SEEDS)
def test_model_population_moments(seed):
    n, nd = 5000, 4
    beta = np.array([[-2.3, -3.4]])
    Sigma = np.array([[0.9, -0.35], [-0.35, 1.4]])
    l2 = np.tile(R.l2_record(beta, Sigma), (nd, 1))
    m = R.replicate(1, seed, np.zeros(n), np.full(n, T0), level2=l2, D=2, K=1)
    y = np.stack([np.log(m["lam"]).ravel(), np.log(m["mu"]).ravel()])
    N = y.shape[1]
    mean, cov = y.mean(axis=1), np.cov(y, ddof=0)
    for j in range(2):                                  # 5 standard errors: two-sided 5.7e-7
        assert abs(mean[j] - beta[0, j]) < 5.0 * np.sqrt(Sigma[j, j] / N)
        for k in range(2):
            se = np.sqrt((Sigma[j, j] * Sigma[k, k] + Sigma[j, k] ** 2) / N)
            assert abs(cov[j, k] - Sigma[j, k]) < 5.0 * se


# ---- power: a wrong layout disagrees with the model on most lanes ------------------------------
@pytest.mark.parametrize("wrong", [dict(swap_counter=True), dict(stream=2), dict(recency_half=0)],
                         ids=["swapped_counter", "stream_2", "recency_from_xy"])
def test_a_wrong_layout_disagrees_on_most_lanes(wrong):
    n, nd = 64, 6
    l1 = np.zeros((nd, n, 4))
    l1[..., 0], l1[..., 1] = 8.0 / 32.0, 0.5 / 32.0
    T = np.full(n, 32.0)
    for seed in R.SEEDS:
        a = R.replicate(0, seed, np.zeros(n), T, level1=l1)
        b = R.replicate(0, seed, np.zeros(n), T, level1=l1, **wrong)
        differ = (a["x_rep"] != b["x_rep"]) | (np.abs(a["t_x_rep"] - b["t_x_rep"]) > R.RTOL * np.abs(a["t_x_rep"]))
        print(wrong, hex(seed), "lanes that differ", differ.mean())
        assert differ.mean() > 0.8


# ---- frames ----------------------------------------------------------------------------------------
def _hand_made():
    # 4 customers, 3 replicated data sets, k_hist = 2
    x = np.array([0, 1, 3, 0])
    t_x = np.array([0.0, 4.0, 9.0, 0.0])
    x_rep = np.array([[0, 1, 3, 0], [0, 0, 0, 0], [2, 1, 5, 1]], np.int64)
    tx_rep = np.array([[0.0, 2.0, 7.0, 0.0], [0.0, 0.0, 0.0, 0.0], [3.0, 5.0, 9.5, 1.0]])
    alive = np.array([[1, 0, 1, 1], [0, 0, 0, 1], [1, 1, 1, 1]], bool)
    return x, t_x, x_rep, tx_rep, R.aggregates(x_rep, tx_rep, alive, x, t_x, 2)


def test_frames_from_hand_made_outputs():
    from mcmc_clv_model_amd import analysis as A
    x, t_x, x_rep, tx_rep, ag = _hand_made()
    out = A.ppc_frames(ag["customers"], ag["draws_int"], ag["sum_tx"][:, None], x, t_x, 2, "customer", 7)
    assert out["level"] == "customer" and out["n_samples"] == 3 and out["seed"] == 7 and "x_rep" not in out
    f = out["frequency"]
    assert list(f.index) == [0, 1, "2+"] and list(f.columns) == ["observed", "rep_mean", "rep_p05", "rep_p50", "rep_p95"]
    assert list(f["observed"]) == [2, 1, 1]
    np.testing.assert_allclose(f["rep_mean"], [(2 + 4 + 0) / 3, (1 + 0 + 2) / 3, (1 + 0 + 2) / 3])
    np.testing.assert_allclose(f["rep_p50"], [2, 1, 1])
    np.testing.assert_allclose(f["rep_p05"], np.percentile([[2, 1, 1], [4, 0, 0], [0, 2, 2]], 5, axis=0))
    d = out["draws"]
    assert list(d["n_zero"]) == [2, 4, 0] and list(d["total_x"]) == [4, 0, 9] and list(d["max_x"]) == [3, 0, 5]
    assert list(d["n_alive"]) == [3, 1, 4]
    np.testing.assert_allclose(d["var_x"], [np.var([0, 1, 3, 0]), 0.0, np.var([2, 1, 5, 1])])
    assert np.isnan(d["mean_recency"][1])               # nobody repeats in the second data set
    np.testing.assert_allclose(d["mean_recency"][[0, 2]], [9.0 / 2, 18.5 / 4])
    s = out["statistics"]
    assert list(s.index) == ["share_zero", "total_x", "max_x", "var_x", "mean_recency"]
    # total_x: observed 4; replicates 4, 0, 9 -> P(>=) = 2/3, p_mid = 1/3 + 1/6
    assert s.loc["total_x", "observed"] == 4 and s.loc["total_x", "p_value"] == pytest.approx(2 / 3)
    assert s.loc["total_x", "p_mid"] == pytest.approx(0.5)
    assert s.loc["total_x", "rep_mean"] == pytest.approx(13 / 3) and s.loc["total_x", "rep_sd"] == pytest.approx(np.std([4, 0, 9], ddof=1))
    # share_zero: observed 0.5; replicates 0.5, 1, 0
    assert s.loc["share_zero", "p_value"] == pytest.approx(2 / 3) and s.loc["share_zero", "p_mid"] == pytest.approx(0.5)
    # mean_recency: observed 13 / 2; defined in two replicates: 4.5, 4.625 -> nobody reaches it
    assert s.loc["mean_recency", "observed"] == pytest.approx(6.5) and s.loc["mean_recency", "p_value"] == 0.0
    c = out["customers"]
    assert list(c.columns) == list(R.STATS)
    np.testing.assert_allclose(c["p_x_lt"], [0, 1 / 3, 1 / 3, 0])
    np.testing.assert_allclose(c["p_x_eq"], [2 / 3, 2 / 3, 1 / 3, 2 / 3])
    with_rep = A.ppc_frames(ag["customers"], ag["draws_int"], ag["sum_tx"][:, None], x, t_x, 2, "population", 7, x_rep,
                            tx_rep)
    assert with_rep["x_rep"] is x_rep and with_rep["t_x_rep"] is tx_rep and with_rep["level"] == "population"
    for bins in (1, 4, 10):
        pit = A.ppc_pit(out, bins=bins, seed=3)
        assert len(pit) == bins and int(pit.sum()) == 4
    assert A.ppc_pit(out, bins=2, seed=0).equals(A.ppc_pit(out, bins=2, seed=0))
    with pytest.raises(ValueError):
        A.ppc_pit(out, bins=0)


# ---- validation ------------------------------------------------------------------------------------
def _py_case(n=3, nd=4):
    cbs = pd.DataFrame(dict(x=[0, 2, 5][:n], t_x=[0.0, 3.0, 8.0][:n], T_cal=[10.0] * n, c1=[0.1, -0.2, 0.3][:n]))
    draws = dict(level_1=[np.ones((nd, n, 4))], level_2=[np.ones((nd, 5))])
    return draws, cbs


@pytest.mark.parametrize("kw, match", [
    (dict(level="both"), "level must be one of"),
    (dict(k_hist=0), "k_hist must be a whole number"),
    (dict(k_hist=4097), "k_hist must be a whole number"),
    (dict(k_hist=2.5), "k_hist must be a whole number"),
    (dict(customer_offset=(1 << 32) - 2), "customer_offset \\+ N must fit in 32 bits"),
    (dict(customer_offset=-1), "customer_offset \\+ N must fit in 32 bits"),
    (dict(level="population", covariates=["c1"]), "match neither the bivariate"),
    (dict(level="population", covariates=["nope"], l2w=7), "no column 'nope'"),
])
def test_python_rejects_bad_arguments(kw, match):
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case()
    kw = dict(kw)
    cov = kw.pop("covariates", None)
    if "l2w" in kw:
        draws["level_2"] = [np.ones((4, kw.pop("l2w")))]
    with pytest.raises(ValueError, match=match):
        A.posterior_predictive_check(draws, cbs, cov, **kw)


def test_python_rejects_bad_data():
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case()
    for level in ("customer", "population"):
        with pytest.raises(ValueError, match="no column 't_x'"):
            A.posterior_predictive_check(draws, cbs.drop(columns="t_x"), level=level)
        bad = cbs.copy()
        bad["x"] = [0.0, 2.5, 5.0]
        with pytest.raises(ValueError, match="non-negative integer counts"):
            A.posterior_predictive_check(draws, bad, level=level)
    with pytest.raises(ValueError, match="level-2 records are needed"):
        A.posterior_predictive_check(dict(level_1=draws["level_1"]), cbs, level="population")
    with pytest.raises(ValueError, match="level-1 draws are needed"):
        A.posterior_predictive_check(dict(level_1=None, level_2=draws["level_2"]), cbs)
    with pytest.raises(ValueError, match="disagree on the number of customers"):
        A.posterior_predictive_check(draws, pd.concat([cbs, cbs]))


def test_fit_keyword_is_validated_before_the_run():
    from mcmc_clv_model_amd import sampler as S
    assert S.ppc_kwargs(None, "full") is None and S.ppc_kwargs(True, "full") == {}
    assert S.ppc_kwargs(dict(level="population", k_hist=16), "full") == dict(level="population", k_hist=16)
    for bad, sink in ((dict(level="x"), "full"), (dict(k_hist=0), "full"), (dict(T_star=3), "full"), (True, "summary"),
                      (3, "full")):
        with pytest.raises(ValueError):
            S.ppc_kwargs(bad, sink)


def test_default_k_hist():
    from mcmc_clv_model_amd import analysis as A
    assert A.ppc_params(x=np.array([0, 3]))["k_hist"] == 8
    assert A.ppc_params(x=np.array([0, 40]))["k_hist"] == 41
    assert A.ppc_params(x=np.array([0, 4000]))["k_hist"] == 256

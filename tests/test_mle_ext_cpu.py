"""The classical baseline's extensions without a device: the C ABI's declarations and
argument checks, the host-side validation, the float64 models of tests/mle_ext_ref.py held to mpmath on a
sample of each fixture of tests/golden/mle_ext_*.npz, the bound on the models' own error, the step of the
central-difference Hessian, the chi-square survival function and the Wald algebra."""
import ctypes
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import mle_ext_ref as M
from tests.helpers import cdnow, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "clvmcmc.h")
NEW_SYMBOLS = ("clv_pnbd_set_covariates", "clv_pnbd_eval_cov", "clv_pnbd_customers_cov", "clv_pnbd_track_cov",
               "clv_pnbd_dert", "clv_dert_integral", "clv_gg_create", "clv_gg_destroy", "clv_gg_eval", "clv_gg_customers",
               "clv_digamma")
ULP = 2.0 ** -52
NEAR_OPT = (0.55, 10.58, 0.61, 11.67)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def same_error(measured, stored):
    """A model error measured here against the one the fixture stores: libm builds differ by an ulp or two per
    call, so the two agree to a factor, not to the bit."""
    return measured <= max(4.0 * float(stored), 64.0 * ULP)


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
    sec = text[text.index("Pareto/NBD with time-invariant covariates"):text.index("Many small fits in one launch")]
    for cite in ("Fader & Hardie (2007)", "equations (1) and (2)", "Fader, Hardie & Lee (2005)", "equation 14",
                 "Gamma-Gamma model", "equation (1a)"):
        assert cite in sec, cite
    for name in ("GammaGammaFitter", "classical_lifetime_value", "likelihood_ratio_test", "ParetoNBDFitter"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_c_abi_argument_checks_come_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    one, out = np.ones(1), np.empty(1)
    assert L.clv_pnbd_set_covariates(None, 0, None, 0, None) == -1
    assert L.clv_pnbd_eval_cov(None, dptr(one), dptr(out), None) == -1
    assert L.clv_pnbd_customers_cov(None, dptr(one), 1.0, dptr(out)) == -1
    assert L.clv_pnbd_dert(None, dptr(one), 0.1, 1.0, dptr(out)) == -1
    p = np.array(NEAR_OPT + (0.0,))
    z = np.zeros((9, 1))
    assert L.clv_pnbd_track_cov(-1, 1, dptr(one), dptr(one), 1, dptr(p), 9, dptr(z), 0, None, dptr(out)) == -1
    assert b"0..8" in L.clv_last_error()
    z[0, 0] = np.nan
    assert L.clv_pnbd_track_cov(-1, 1, dptr(one), dptr(one), 1, dptr(p), 1, dptr(z), 0, None, dptr(out)) == -1
    assert b"non-finite purchase covariate" in L.clv_last_error()
    p[4] = np.inf
    assert L.clv_pnbd_track_cov(-1, 1, dptr(one), dptr(one), 1, dptr(p), 1, dptr(np.zeros(1)), 0, None, dptr(out)) == -1
    assert b"coefficients must be finite" in L.clv_last_error()
    for s, B, d, H, msg in ((1.0, 10.0, 0.0, np.inf, b"infinite horizon"), (0.0, 10.0, 0.1, 1.0, b"positive"),
                            (1.0, 10.0, -1.0, 1.0, b"delta"), (1.0, 10.0, 0.1, 0.0, b"horizon")):
        a = [np.array([v]) for v in (s, B, d, H)]
        assert L.clv_dert_integral(-1, 1, *(dptr(v) for v in a), dptr(out)) == -1 and msg in L.clv_last_error()
    h = ctypes.c_void_p()
    n1 = (ctypes.c_int32 * 2)(1, 0)
    assert L.clv_gg_create(-1, 2, n1, dptr(np.ones(2)), None, ctypes.byref(h)) == -1 and b"frequency < 1" in L.clv_last_error()
    n1 = (ctypes.c_int32 * 2)(1, 3)
    assert L.clv_gg_create(-1, 2, n1, dptr(np.array([1.0, 0.0])), None, ctypes.byref(h)) == -1
    assert b"monetary value must be > 0" in L.clv_last_error() and not h
    assert L.clv_gg_create(-1, 0, n1, dptr(np.ones(2)), None, ctypes.byref(h)) == -1
    assert L.clv_gg_eval(None, dptr(one), dptr(out)) == -1 and L.clv_gg_customers(None, dptr(one), dptr(out)) == -1
    assert L.clv_digamma(-1, 1, dptr(np.array([-1.0])), dptr(out)) == -1 and b"positive" in L.clv_last_error()
    L.clv_gg_destroy(None)


def test_host_side_validation_raises_before_the_device():
    from mcmc_clv_model_amd.mle import (GammaGammaFitter, GgData, ParetoNBDFitter, PnbdData, classical_lifetime_value,
                                        covariate_matrix, pnbd_weekly_tracking)
    df = cdnow("abe", 50)
    a = (df["x"], df["t_x"], df["T_cal"])
    for kw, msg in ((dict(covariates=np.zeros((50, 9))), "at most 8"), (dict(covariates=np.zeros((49, 1))), "shape"),
                    (dict(covariates=np.zeros((50, 1, 1))), "shape"), (dict(covariates=np.full((50, 1), np.inf)), "finite"),
                    (dict(covariates=np.zeros((50, 1)), covariates_dropout=np.zeros((50, 9))), "at most 8"),
                    (dict(covariates=np.zeros((50, 1)), covariates_dropout=np.full((50, 1), np.nan)), "finite"),
                    (dict(covariates=np.zeros((50, 2)), covariate_names=["a"]), "names"),
                    (dict(covariates_dropout=np.zeros((50, 1))), "without covariates"),
                    (dict(covariates=np.zeros((50, 1)), initial_params=(1, 1, 1, 1, 0)), "initial_params"),
                    (dict(covariates=np.zeros((50, 1)), initial_params=(1, 1, 1, 1, 0, np.nan)), "initial_params")):
        with pytest.raises(ValueError, match=msg):
            ParetoNBDFitter().fit(*a, **kw)
        if "initial_params" not in kw and "covariate_names" not in kw:
            with pytest.raises(ValueError, match=msg):
                PnbdData(*a, **kw)
    z, names = covariate_matrix(df[["first_sales_scaled", "age_scaled"]], 50)
    assert z.shape == (2, 50) and z.flags.c_contiguous and names == ["first_sales_scaled", "age_scaled"]
    assert covariate_matrix(np.zeros((50, 0)), 50)[0].shape == (0, 50)
    f = ParetoNBDFitter()
    f.params_ = pd.Series(NEAR_OPT + (0.1, -0.1), index=["r", "alpha", "s", "beta", "purchase:z", "dropout:z"])
    f._k = (1, 1)
    good = df[["first_sales_scaled"]]
    for call in (lambda: f.conditional_probability_alive(*a), lambda: f.pointwise_log_likelihood(*a),
                 lambda: f.conditional_expected_number_of_purchases_up_to_time(39.0, *a),
                 lambda: f.information_criteria(*a), lambda: f.discounted_expected_transactions(*a),
                 lambda: f.expected_number_of_purchases_up_to_time(5.0), lambda: f.hessian(*a),
                 lambda: pnbd_weekly_tracking(f, [1.0] * 50, [2.0])):
        with pytest.raises(ValueError, match="fitted with covariates"):
            call()
    with pytest.raises(ValueError, match="1 purchase and 1 dropout"):
        f.conditional_probability_alive(*a, covariates=df[["first_sales_scaled", "age_scaled"]])
    with pytest.raises(ValueError, match="one row per customer"):
        f.conditional_probability_alive(*a, covariates=good.iloc[:40])
    with pytest.raises(ValueError, match="infinite horizon"):
        f.discounted_expected_transactions(*a, discount_rate=0.0, covariates=good)
    with pytest.raises(ValueError, match="horizon"):
        f.discounted_expected_transactions(*a, horizon=0.0, covariates=good)
    with pytest.raises(ValueError, match="theta"):
        f.hessian(*a, covariates=good, theta=np.zeros(5))
    per = f.expected_number_of_purchases_up_to_time(np.arange(4.0), covariates=good)      # host numpy
    al, be = M.customer_scales(f.params_.to_numpy(), good.to_numpy().T, good.to_numpy().T)
    assert per.shape == (50, 4) and per[7, 0] == 0.0
    assert np.allclose(per[:, 3], NEAR_OPT[0] * be / al * (-np.expm1(-(NEAR_OPT[2] - 1) * np.log1p(3.0 / be)) / (NEAR_OPT[2] - 1)),
                       rtol=1e-14)
    plain = ParetoNBDFitter()
    plain.params_ = pd.Series(NEAR_OPT, index=["r", "alpha", "s", "beta"])
    with pytest.raises(ValueError, match="without covariates"):
        plain.conditional_probability_alive(*a, covariates=good)
    with pytest.raises(ValueError, match="without covariates"):
        plain.expected_number_of_purchases_up_to_time(1.0, covariates=good)
    # Gamma-Gamma
    for n, m, msg in (([0, 1], [1.0, 1.0], "filter"), ([1, 2], [1.0, 0.0], "monetary_value"), ([1, 2], [1.0, -3.0], "monetary_value"),
                      ([1, 2], [np.nan, 1.0], "monetary_value"), ([1.5], [1.0], "integer"), ([1, 2], [1.0], "same length"),
                      ([-1], [1.0], "filter")):
        with pytest.raises(ValueError, match=msg):
            GgData(n, m)
        with pytest.raises(ValueError, match=msg):
            GammaGammaFitter().fit(n, m)
    with pytest.raises(ValueError, match="weights"):
        GgData([1, 2], [1.0, 2.0], [1.0])
    with pytest.raises(ValueError, match="initial_params"):
        GammaGammaFitter().fit([1], [1.0], initial_params=(1, 0, 1))
    gg = GammaGammaFitter()
    with pytest.raises(RuntimeError):
        gg.conditional_expected_average_profit()
    gg.params_ = pd.Series([6.25, 3.74, 15.44], index=["p", "q", "gamma"])
    with pytest.raises(ValueError, match="missing required column"):
        classical_lifetime_value(plain, gg, df.drop(columns="t_x"), monetary_frequency=[1] * 50, monetary_value=[1.0] * 50)
    with pytest.raises(ValueError, match="one entry per customer"):
        classical_lifetime_value(plain, gg, df, monetary_frequency=[1], monetary_value=[1.0])
    with pytest.raises(ValueError, match="infinite horizon"):
        classical_lifetime_value(plain, gg, df, monetary_frequency=[1] * 50, monetary_value=[1.0] * 50, discount_rate=0.0)


def test_plain_fit_path_is_untouched_by_the_new_keywords():
    """fit_objective on four parameters: the names, the log transform and the result's bits as before."""
    from mcmc_clv_model_amd.mle import ParetoNBDFitter
    def quad(t):
        return float(((t - 0.3) ** 2).sum()), 2.0 * (t - 0.3)
    f = ParetoNBDFitter().fit_objective(quad, (1.0, 2.0, 3.0, 4.0))
    assert list(f.params_.index) == ["r", "alpha", "s", "beta"] and f.converged_
    assert np.allclose(f.params_.to_numpy(), np.exp(0.3), rtol=1e-6)
    g = ParetoNBDFitter().fit_objective(quad, (1.0, 2.0, 3.0, 4.0, 0.5), names=["r", "alpha", "s", "beta", "purchase:z"])
    assert np.allclose(g.params_.to_numpy(), [np.exp(0.3)] * 4 + [0.3], rtol=1e-6)
    assert f._k is None


# ---------------------------------------------------------------------------------------------
# the float64 models against mpmath, on a sample of each fixture
# ---------------------------------------------------------------------------------------------
def test_covariate_model_against_mpmath_on_a_sample():
    g = golden("mle_ext_cov.npz")
    for k in (0, 1):
        p = g["params"][k]
        m = M.model_customers_cov(g["x"], g["t_x"], g["T"], p, g["z1"], g["z2"], float(g["t_star"]))
        assert np.array_equal(m["alpha"] < m["beta"], g["swap"][k]) and g["swap"][k].any() and not g["swap"][k].all()
        for key in ("logL", "p_alive", "ey"):
            assert same_error(rel(m[key], g[key][k]).max(), g["eref_" + key][k]), (k, key)
        err = (np.abs(m["scores"].sum(0) - g["grad_sum"][k]) / np.maximum(1.0, g["grad_abs"][k])).max()
        assert same_error(err, g["eref_grad"][k])
        assert m["scores"][:, 5].tolist() == [0.0] * 12 or not m["scores"][:, 5].any()    # the zero column
        for i in (1, 7):                                                                 # regenerated with mpmath
            v = M.exact_customer_cov(g["x"][i], g["t_x"][i], g["T"][i], p, g["z1"][:, i], g["z2"][:, i], float(g["t_star"]))
            assert [float(t) for t in v[:3]] == [g["logL"][k, i], g["p_alive"][k, i], g["ey"][k, i]]
            assert abs(float(v[3][4]) + g["z1"][0, i] * float(v[3][1])) <= 4 * ULP * abs(float(v[3][4]))    # the chain rule


def test_hessian_step_reproduces_the_stored_error():
    from mcmc_clv_model_amd import mle
    g = golden("mle_ext_hessian.npz")
    assert float(g["step"]) == mle.HESSIAN_STEP == M.HESSIAN_STEP
    grad = M.model_gradient_cov(g["x"], g["t_x"], g["T"], g["z1"], g["z2"])
    scale = np.maximum(1.0, g["hessian_abs"])
    H = mle.central_hessian(grad, g["theta"])
    assert np.array_equal(H, M.central_hessian(grad, g["theta"])) and np.array_equal(H, H.T)
    err = (np.abs(H - g["hessian"]) / scale).max()
    print(f"model central difference at 2^{np.log2(g['step']):.0f}: {err:.3g} (stored {float(g['eref']):.3g})")
    assert same_error(err, g["eref"])
    # the scan: truncation falls as h^2 above the chosen step, rounding rises as 1 / h below it, and both are two
    # orders of magnitude below the 1e-6 the standard errors are held to
    scan, steps = g["scan"], g["steps"]
    assert float(g["eref"]) <= scan.min() * 1.0000001 and float(g["eref"]) <= 1e-8
    assert scan[0] > 1e3 * scan.min() and scan[-1] > 1e2 * scan.min()
    k = int(np.flatnonzero(steps == g["step"])[0])
    assert scan[k] == float(g["eref"]) and scan[k - 3] > 10 * scan[k] and scan[k + 5] > 10 * scan[k]
    # one entry regenerated with mpmath (a 2 x 2 block of one customer's frame would not be the sum): the
    # exact Hessian is symmetric and agrees with a high-precision difference of the model-free gradient
    assert np.allclose(g["hessian"], g["hessian"].T, rtol=1e-13)
    eig = np.linalg.eigvalsh(-M.central_hessian(grad, g["indefinite_theta"]))
    assert eig.min() < -1.0 < 1.0 < eig.max()


def test_gamma_gamma_model_against_mpmath_and_its_error_bound():
    g = golden("mle_ext_gg.npz")
    heavy = g["heavy"]
    assert heavy.sum() == 4 and (g["n"][heavy] == 2000).all()
    for k, p in enumerate(g["params"]):
        c = M.model_gg_customers(g["n"], g["m"], p)
        eL, eG = rel(c["logL"], g["logL"][k]), rel(c["grad"], g["grad"][k]).max(1)
        assert same_error(eL.max(), g["eref_logL"][k]) and same_error(eG.max(), g["eref_grad"][k])
        assert same_error(rel(M.model_gg_mean(g["n"], g["m"], p), g["mean"][k]).max(), g["eref_mean"][k])
        # E_ref is itself bounded: the heavy buyers are no more than ten times worse than the easy rows
        for name in ("logL", "grad"):
            hv, ez = float(g[f"eref_{name}_heavy"][k]), float(g[f"eref_{name}_easy"][k])
            print(f"set {k} {name}: E_ref heavy {hv:.3g}, easy {ez:.3g}")
            assert hv <= 10.0 * ez, (k, name)
        for i in (3, 14):
            v = M.exact_gg_customer(g["n"][i], g["m"][i], p)
            assert float(v[0]) == g["logL"][k, i] and [float(t) for t in v[1]] == g["grad"][k, i].tolist()
            assert float(v[2]) == g["mean"][k, i]
    # what the rule is for: two lgamma calls lose the heavy buyers
    p = g["params"][2]
    bad = rel(M.model_gg_customers(g["n"], g["m"], p, stable=False)["logL"], g["logL"][2])
    assert bad[heavy].max() > 10.0 * float(g["eref_logL_easy"][2]) and bad[heavy].max() > 8.0 * float(g["eref_logL"][2])
    x = g["psi_x"]
    assert same_error(rel(M.model_digamma(x), g["psi"]).max(), g["eref_psi"])
    assert [float(M.exact_digamma(v)) for v in x[::9]] == g["psi"][::9].tolist()
    a = np.array([32.0, 1e3, 6e5, 1e6])
    for d in (0.5, 3.74, 200.0):
        want = np.array([float(M._mp().digamma(M._mp().mpf(float(v)) + M._mp().mpf(d)) - M._mp().digamma(M._mp().mpf(float(v)))) for v in a])
        assert rel(M.model_digamma_diff(a, d), want).max() <= 8 * ULP
        assert (np.abs(M.model_digamma_diff(a, d) / want - 1.0)).max() <= 64 * ULP      # relative: nothing cancels


def test_gamma_gamma_model_fit_is_the_golden_optimum():
    from mcmc_clv_model_amd.mle import GammaGammaFitter
    g = golden("mle_ext_fit.npz")
    df = cdnow("abe")
    n = df["x"].to_numpy() + 1
    m = df["sales"].to_numpy() / n
    n, m = n[m > 0], m[m > 0]
    f = GammaGammaFitter().fit_objective(M.model_gg_value_and_grad(n, m), [1, 1, 1])
    assert f.converged_ and np.allclose(f.params_.to_numpy(), g["gg_params"], rtol=1e-6)
    # the covariate optimum: the model's gradient vanishes there
    x, tx, T = df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy()
    z = df["first_sales_scaled"].to_numpy()[None, :]
    p = g["cov_params"]
    val, grad = M.model_value_and_grad_cov(x, tx, T, z, z)(np.concatenate([np.log(p[:4]), p[4:]]))
    assert np.abs(grad).max() <= 1e-7 and abs(-val * len(x) - float(g["cov_logL"])) <= 1e-8


def test_dert_model_against_mpmath_and_its_error_bound():
    g = golden("mle_ext_dert.npz")
    s, B, d, H = g["s"], g["B"], g["delta"], g["H"]
    assert sorted(set(s)) == [0.3, 0.606, 1 - 2.0 ** -30, 1.0, 1 + 2.0 ** -30, 2.0, 2.5, 7.0]
    assert sorted(set(np.round(d * B, 12))) == [1e-4, 0.0137, 0.14, 1.0, 30.0] and sorted(set(H)) == [1e-3, 52.0, 520.0, np.inf]
    mod = np.array([M.model_dert_integral(*v) for v in zip(s, B, d, H)])
    assert same_error(rel(mod, g["J"]).max(), g["eref"])
    print(f"E_ref at integer s {float(g['eref_integer']):.3g}, elsewhere {float(g['eref_easy']):.3g}")
    assert float(g["eref_integer"]) <= 10.0 * float(g["eref_easy"]) and g["integer"].sum() == 5 * 5 * 4
    for i in range(0, len(s), 23):
        assert float(M.exact_dert_integral(s[i], B[i], d[i], H[i])) == g["J"][i]
    # the closed form the integral rewrites: J(inf) = B e^z E_s(z), and the finite-horizon difference
    mp = M._mp()
    for i in np.flatnonzero(np.isinf(H))[::7]:
        z = mp.mpf(float(d[i])) * mp.mpf(float(B[i]))
        assert abs(float(mp.mpf(float(B[i])) * mp.exp(z) * mp.expint(mp.mpf(float(s[i])), z)) / g["J"][i] - 1.0) <= 4 * ULP
    # what the rule is for: the small-z series of E_s cancels next to an integer s
    i = int(np.flatnonzero((s == 1 + 2.0 ** -30) & np.isinf(H) & (np.abs(d * B - 0.14) < 1e-9))[0])
    naive = M.naive_dert_integral_inf(s[i], B[i], d[i])
    assert rel(naive, g["J"][i]) > 1e3 * max(8 * float(g["eref"]), 64 * ULP)
    # end to end on two edge customers
    k = 1
    p = g["cust_params"][k]
    _, md = M.model_dert_customers(g["x"], g["t_x"], g["T"], p[0], p[1], p[2], p[3], float(g["cust_delta"]), np.inf)
    assert same_error(rel(md, g["cust_dert"][k, 0]).max(), g["eref_cust"][k])
    for i in (0, 6):
        pa, de = M.exact_dert_customer(g["x"][i], g["t_x"][i], g["T"][i], p, float(g["cust_delta"]), 52.0)
        assert float(de) == g["cust_dert"][k, 1, i] and float(pa) == g["cust_p_alive"][k, i]


def test_gauss_legendre_header():
    x, w = M.gauss_legendre_header()
    nx, nw = np.polynomial.legendre.leggauss(16)
    assert len(x) == 16 and np.allclose(x, nx, rtol=0, atol=4 * ULP) and np.allclose(w, nw, rtol=1e-13, atol=0)
    for deg in range(0, 32):
        want = 0.0 if deg % 2 else 2.0 / (deg + 1)
        assert abs(math.fsum(w * x ** deg) - want) <= 4 * ULP
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_gauss_legendre.py"), "--check"])
    assert r.returncode == 0


# ---------------------------------------------------------------------------------------------
# chi-square, delta method, Wald interval
# ---------------------------------------------------------------------------------------------
def test_chi2_survival_function_against_mpmath():
    from mcmc_clv_model_amd.mle import chi2_sf, likelihood_ratio_test
    worst = 0.0
    for df in range(1, 17):
        for x in (1e-6, 0.1, 1.0, 3.84, float(df), 2.5 * df, 60.0, 200.0):
            want = float(M.exact_chi2_sf(x, df))
            worst = max(worst, abs(chi2_sf(x, df) / want - 1.0))
    print(f"chi2_sf, df 1..16: largest relative error {worst:.3g}")
    assert worst <= 1e-13           # erfc, exp and lgamma to a few ulp; up to eight positive terms; exponents to 100
    assert chi2_sf(0.0, 3) == 1.0 and chi2_sf(-1.0, 2) == 1.0 and math.isnan(chi2_sf(np.nan, 2))
    assert abs(chi2_sf(3.841458820694124, 1) - 0.05) <= 1e-15
    with pytest.raises(ValueError):
        chi2_sf(1.0, 0)
    from types import SimpleNamespace as NS
    r, f = NS(log_likelihood_=-100.0, params_=[0] * 4), NS(log_likelihood_=-97.0, params_=[0] * 6)
    t = likelihood_ratio_test(r, f)
    assert t == dict(statistic=6.0, df=2, p_value=chi2_sf(6.0, 2)) and abs(t["p_value"] - math.exp(-3.0)) <= 1e-16
    with pytest.raises(ValueError):
        likelihood_ratio_test(f, r)


def test_delta_method_and_wald_interval_on_a_hand_made_covariance():
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, delta_standard_errors, wald_summary
    theta = np.array([math.log(2.0), math.log(0.5), 0.3, -0.02])
    cov = np.diag([0.04, 0.01, 0.0025, 0.01])
    cov[0, 2] = cov[2, 0] = 0.001
    se = delta_standard_errors(theta, cov, 2)
    assert np.allclose(se, [2.0 * 0.2, 0.5 * 0.1, 0.05, 0.1], rtol=1e-15)
    t = wald_summary(theta, cov, ["a", "b", "g1", "g2"], 2)
    assert list(t.index) == ["a", "b", "g1", "g2"] and list(t.columns) == ["estimate", "se", "z", "p", "ci_lower", "ci_upper"]
    assert np.allclose(t["estimate"], [2.0, 0.5, 0.3, -0.02], rtol=1e-15) and np.allclose(t["se"], se)
    assert np.allclose(t["z"], [math.log(2.0) / 0.2, math.log(0.5) / 0.1, 6.0, -0.2], rtol=1e-14)
    assert np.allclose(t["p"], [math.erfc(abs(z) / math.sqrt(2)) for z in t["z"]], rtol=1e-15)
    q = 1.959963984540054
    assert np.allclose(t["ci_lower"], [2.0 * math.exp(-q * 0.2), 0.5 * math.exp(-q * 0.1), 0.3 - q * 0.05, -0.02 - q * 0.1], rtol=1e-14)
    assert np.allclose(t["ci_upper"], [2.0 * math.exp(q * 0.2), 0.5 * math.exp(q * 0.1), 0.3 + q * 0.05, -0.02 + q * 0.1], rtol=1e-14)
    assert abs(0.5 * math.erfc(q / math.sqrt(2.0)) - 0.025) <= 1e-15
    # through the fitter: covariance = (-H)^-1, the sandwich, and the indefinite case
    f = ParetoNBDFitter()
    f.params_ = pd.Series([2.0, 0.5, 1.0, 1.0, 0.3], index=["r", "alpha", "s", "beta", "purchase:z"])
    H = -np.diag([25.0, 100.0, 4.0, 1.0, 400.0])
    f._set_uncertainty(H)
    assert np.allclose(np.diag(f.covariance_), [0.04, 0.01, 0.25, 1.0, 0.0025]) and list(f.covariance_.index)[0] == "log r"
    assert np.allclose(f.standard_errors_, [0.4, 0.05, 0.5, 1.0, 0.05]) and list(f.standard_errors_.index) == list(f.params_.index)
    S = np.arange(15.0).reshape(3, 5)
    f._set_uncertainty(H, S)
    Hi = np.linalg.inv(H)
    assert np.allclose(f.covariance_, Hi @ S.T @ S @ Hi, rtol=1e-13)
    H[4, 4] = 1.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        f._set_uncertainty(H)
    assert len(rec) == 1 and issubclass(rec[0].category, RuntimeWarning) and "not negative definite" in str(rec[0].message)
    assert np.isnan(f.standard_errors_).all() and np.isnan(f.summary_[["se", "z", "p", "ci_lower", "ci_upper"]].to_numpy()).all()
    assert np.allclose(f.summary_["estimate"], f.params_)

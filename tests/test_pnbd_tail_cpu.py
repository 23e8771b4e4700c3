"""The quadrature evaluation of the Pareto/NBD integral without a device: the C ABI's
declaration and argument checks, the host-side validation, the float64 model of tests/pnbd_tail_ref.py held to
mpmath on a sample of tests/golden/pnbd_tail_exact.npz (regenerated here), the power of that fixture against the
two wrong variants the model carries, and the recorded full-CBS optimum."""
import os

import numpy as np
import pytest

from tests import pnbd_tail_ref as Q
from tests.helpers import cdnow, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "clvmcmc.h")
ULP = 2.0 ** -52


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def same_error(measured, stored):
    """A model error measured here against the one the fixture stores: libm builds differ by an ulp or two per
    call, so the two agree to a factor, not to the bit."""
    return measured <= max(4.0 * float(stored), 64.0 * ULP)


@pytest.fixture(scope="module")
def fx():
    e = golden("pnbd_tail_exact.npz")
    return {k: e[k] for k in e.files}


def test_header_declares_and_library_exports_the_new_symbol():
    from mcmc_clv_model_amd import _lib
    assert "clv_pnbd_set_integral" in _lib.exported_symbols(), "not declared in include/clvmcmc.h"
    assert hasattr(_lib.lib(), "clv_pnbd_set_integral"), "not exported by the library"
    with open(HDR) as f:
        text = f.read()
    for name, value in (("CLV_PNBD_INTEGRAL_SERIES", 0), ("CLV_PNBD_INTEGRAL_AUTO", 1), ("CLV_PNBD_INTEGRAL_QUADRATURE", 2)):
        assert f"{name} = {value}" in text
    from mcmc_clv_model_amd import mle
    assert mle.INTEGRAL_MODES == {"series": 0, "auto": 1, "quadrature": 2} and tuple(mle.INTEGRAL_MODES) == Q.MODES


def test_a_null_handle_or_a_bad_mode_fails_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 2):
        assert L.clv_pnbd_set_integral(None, mode) == -1 and b"null handle" in L.clv_last_error()
    for mode in (-1, 3, 2 ** 31 - 1):
        assert L.clv_pnbd_set_integral(None, mode) == -1 and b"integral mode" in L.clv_last_error()


def test_an_unknown_integral_raises_before_the_device_is_touched(monkeypatch):
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, PnbdData, integral_mode

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)
    df = cdnow("abe", 20)
    for bad in ("Series", "gauss", "", None, 1):
        with pytest.raises(ValueError, match="integral must be one of"):
            ParetoNBDFitter(integral=bad)
        with pytest.raises(ValueError, match="integral must be one of"):
            PnbdData(df["x"], df["t_x"], df["T_cal"], integral=bad)
        with pytest.raises(ValueError, match="integral must be one of"):
            integral_mode(bad)
    assert ParetoNBDFitter().integral == "series" and ParetoNBDFitter(0.1, integral="auto").integral == "auto"
    with pytest.raises(ValueError):
        Q.takes_quadrature("gauss", 0.0, 1.0, 1.0, 2.0)


def test_the_path_choice_of_the_three_modes(fx):
    tx, T = fx["t_x"], fx["T"]
    has = tx < T
    for k, p in enumerate(fx["params"]):
        z = Q.z_tx(tx, p[1], p[3])
        assert not Q.takes_quadrature("series", tx, T, p[1], p[3]).any()
        assert np.array_equal(Q.takes_quadrature("quadrature", tx, T, p[1], p[3]), has)
        auto = Q.takes_quadrature("auto", tx, T, p[1], p[3])
        assert np.array_equal(auto, has & (z > Q.Z_SWITCH)) and np.array_equal(auto, fx["auto_quadrature"][k])
    # the set at the switch: customers within 1e-12 of it on either side, and each on its own path
    k = int(fx["switch_set"])
    z = fx["z_tx"][k]
    near = has & (np.abs(z - Q.Z_SWITCH) <= 1e-12)
    assert (near & (z > Q.Z_SWITCH)).any() and (near & (z <= Q.Z_SWITCH)).any()
    assert np.array_equal(fx["auto_quadrature"][k][near], z[near] > Q.Z_SWITCH)
    # NEAR_OPT stays on the series throughout; at the sets with a tiny alpha or beta the early t_x leave it
    early = has & (tx <= 0.5)
    assert not fx["auto_quadrature"][5].any() and all(fx["auto_quadrature"][j][early].all() for j in (2, 3))
    assert early.sum() >= 6


ROWS = [(0, 7), (1, 0), (2, 14), (3, 6), (3, 12), (4, 13), (5, 15), (6, 0), (6, 4)]


@pytest.mark.parametrize("k,i", ROWS)
def test_model_against_mpmath_on_a_sample_of_the_fixture(fx, k, i):
    """The row regenerated: the exact values are the fixture's to 1e-15, and the model in both modes is within
    the stored E_ref (to the factor libm builds differ by)."""
    x, tx, T, p = fx["x"][i:i + 1], fx["t_x"][i:i + 1], fx["T"][i:i + 1], fx["params"][k]
    ll, g, pa, ey, lsi = Q.exact_customer(x[0], tx[0], T[0], p, float(fx["t_star"]))
    assert rel(float(lsi), fx["log_sI"][k, i]) <= 4 * ULP
    ex = dict(logL=float(ll), p_alive=float(pa), ey=float(ey))
    for key, v in ex.items():
        assert rel(v, fx[key][k, i]) <= 4 * ULP, key
    assert rel(np.array([float(v) for v in g]), fx["grad"][k, i]).max() <= 4 * ULP
    scale = np.maximum(1.0, fx["grad_abs"][k])
    for mode in ("auto", "quadrature"):
        m = Q.model_customers_tail(x, tx, T, *p, mode, float(fx["t_star"]))
        assert m["converged"].all()
        if mode == "quadrature":
            assert same_error(rel(m["log_sI"][0], float(lsi)), fx["eref_log_sI"][k])
        for key, v in ex.items():
            err = rel(m[key][0], v)
            print(f"set {k} row {i} {mode} {key}: measured {err:.3g}, stored E_ref {fx['eref_' + key][k]:.3g}")
            assert same_error(err, fx["eref_" + key][k]), (mode, key, err)
        err = (np.abs(m["grad"][0] - fx["grad"][k, i]) / scale).max()
        assert same_error(err, fx["eref_grad"][k]), (mode, err)


def test_the_fixture_keeps_the_model_far_inside_its_cap(fx):
    assert fx["eref_logL"].max() <= 1e-13 and fx["eref_log_sI"].max() <= 1e-13
    print("E_ref of log L per set", fx["eref_logL"], "panels (max per set)", fx["model_panels"].max(1))


def worst_row(fx, variant, mode="quadrature"):
    """(error of log L over 8 x E_ref, set, row) where the variant is furthest outside the fixture's bound."""
    worst = (0.0, -1, -1)
    for k, p in enumerate(fx["params"]):
        m = Q.model_customers_tail(fx["x"], fx["t_x"], fx["T"], *p, mode, variant=variant)
        err = rel(m["logL"], fx["logL"][k])
        err[~np.isfinite(err)] = np.inf
        bound = max(8.0 * fx["eref_logL"][k], 64.0 * ULP)
        i = int(np.argmax(err))
        if err[i] / bound > worst[0]:
            worst = (err[i] / bound, k, i)
    return worst


def test_the_width_as_a_difference_of_logs_is_caught_at_T_minus_1e_12(fx):
    """At T - t_x = 1e-12 s I is 1e-13 of the survivor term, so log L cannot show the width: the fixture's
    log(s I) does, at every parameter set."""
    i = int(fx["row_t_minus_1e12"])
    assert fx["T"][i] - fx["t_x"][i] == pytest.approx(1e-12, rel=1e-2)
    for k, p in enumerate(fx["params"]):
        row = (fx["x"][i:i + 1], fx["t_x"][i:i + 1], fx["T"][i:i + 1], *p, "quadrature")
        bad, good = Q.model_customers_tail(*row, variant="log_difference_width"), Q.model_customers_tail(*row)
        bound = max(8.0 * fx["eref_log_sI"][k], 64.0 * ULP)
        e_bad, e_good = rel(bad["log_sI"][0], fx["log_sI"][k, i]), rel(good["log_sI"][0], fx["log_sI"][k, i])
        print(f"set {k}: log(s I) with the log-difference width off by {e_bad:.3g}, the model by {e_good:.3g}, "
              f"bound {bound:.3g}")
        assert e_good <= bound < e_bad


def test_exchanged_exponents_are_caught(fx):
    ratio, k, i = worst_row(fx, "exchanged_exponents")
    print(f"p_m and p_M exchanged: {ratio:.3g} x the bound at set {k}, row {i}")
    assert ratio > 1.0
    # named row: x = 200 at a beta of 1e-8, where the two exponents differ by 200
    m = Q.model_customers_tail(fx["x"][7:8], fx["t_x"][7:8], fx["T"][7:8], *fx["params"][3], "quadrature",
                               variant="exchanged_exponents")
    assert rel(m["logL"][0], fx["logL"][3, 7]) > max(8.0 * fx["eref_logL"][3], 64.0 * ULP)


def test_the_abe_sample_holds_both_evaluations(fx):
    df = cdnow("abe")
    idx = fx["abe_rows"][::8]
    x, tx, T = (df[c].to_numpy()[idx] for c in ("x", "t_x", "T_cal"))
    assert 0.3 <= fx["abe_z_min"] and fx["abe_z_max"] <= 0.97
    for mode in ("series", "quadrature"):
        m = Q.model_customers_tail(x, tx, T, *fx["abe_params"], mode, float(fx["t_star"]))
        assert m["converged"].all() and m["quadrature"].all() == (mode == "quadrature")
        for key in ("logL", "p_alive", "ey", "grad"):
            err = rel(m[key], fx["abe_" + key][::8]).max()
            assert same_error(err, fx[f"abe_eref_{mode}_{key}"]), (mode, key, err)


def test_the_recorded_full_cbs_optimum_is_a_stationary_point_of_the_model(fx):
    """The pin of the device fit: converged, interior, above the wall, and the model's mean-NLL gradient there is
    below the fit's tol."""
    from tests.golden.make_pnbd_tail_goldens import full_cbs
    assert bool(fx["fit_converged"]) and float(fx["fit_grad_norm"]) <= float(fx["fit_tol"]) == 1e-7
    assert float(fx["fit_logL"]) > -95_304.36 and np.isfinite(fx["fit_se"]).all() and (fx["fit_se"] > 0.0).all()
    np.linalg.cholesky(fx["fit_covariance"])
    x, tx, T, z = full_cbs()
    p = fx["fit_params"]
    val, g = Q.model_value_and_grad_cov_tail(x, tx, T, z, z, "auto")(np.concatenate([np.log(p[:4]), p[4:]]))
    print(f"log L {-val * len(x):.4f} (recorded {float(fx['fit_logL']):.4f}), max |mean-NLL gradient| {np.abs(g).max():.3g}")
    assert np.abs(g).max() <= float(fx["fit_tol"])
    assert abs(-val * len(x) - float(fx["fit_logL"])) <= 1e-6
    assert int(fx["fit_n_quadrature"]) > 0 and int(fx["fit_n_z_above_cap"]) > 0

"""GPU: the quadrature evaluation of the Pareto/NBD integral (csrc/pnbd.hip pnbd_si_quadrature, the modes of
clv_pnbd_set_integral) against tests/golden/pnbd_tail_exact.npz (mpmath quadrature of the
integral, the float64 model's own error and the model's full-CBS covariate fit; made by
tests/golden/make_pnbd_tail_goldens.py).  Neither mpmath nor a host fit is needed here.

Bound for a device value against the exact one, relative to max(1, |value|): 8 x the fixture's recorded error of
the float64 model (E_ref), floor 64 ulp, as in tests/test_gpu_pnbd.py: the device's log, log1p, expm1, exp and
lgamma each differ from glibc's by a few ulp.  Gradient sums are scaled by sum |terms|."""
import numpy as np
import pytest

from tests import pnbd_ref as R
from tests import pnbd_tail_ref as Q
from tests.helpers import bits, cdnow, golden

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
NEAR_OPT = (0.55, 10.58, 0.61, 11.67)
WALL_LOGL = -95_304.36          # where the series-only covariate fit stops


def bound(e_ref):
    return max(8.0 * float(e_ref), 64.0 * ULP)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@pytest.fixture(scope="module")
def fx():
    e = golden("pnbd_tail_exact.npz")
    return {k: e[k] for k in e.files}


@pytest.fixture(scope="module")
def abe():
    df = cdnow("abe")
    return df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy()


# ---------------------------------------------------------------------------------------------
# the default is untouched
# ---------------------------------------------------------------------------------------------
def test_series_set_explicitly_is_the_handle_that_never_called_the_setter(abe):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T = (a[:257] for a in abe)
    with PnbdData(x, tx, T) as d:
        assert d.integral == "series"
        c0, (s0, u0) = d.customers(NEAR_OPT, 39.0), d.eval(NEAR_OPT)
    with PnbdData(x, tx, T, integral="series") as d:
        c1, (s1, u1) = d.customers(NEAR_OPT, 39.0), d.eval(NEAR_OPT)
        d.set_integral("quadrature")
        d.set_integral("series")            # and back: the mode is the handle's only state
        c2, (s2, u2) = d.customers(NEAR_OPT, 39.0), d.eval(NEAR_OPT)
    assert u0 == u1 == u2 == 0
    assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(s0), bits(s1))
    assert np.array_equal(bits(c0), bits(c2)) and np.array_equal(bits(s0), bits(s2))


def test_series_still_reports_the_customers_past_its_cap():
    from mcmc_clv_model_amd.mle import PnbdData
    e = golden("pnbd_edge.npz")
    p, nan = e["params"][5], e["model_nan"][5]
    assert nan.any()
    with PnbdData(e["x"], e["t_x"], e["T"], integral="series") as d:
        cust, (sums, n_unc) = d.customers(p, 39.0), d.eval(p)
        assert np.array_equal(np.isnan(cust[:, 0]), nan) and n_unc == int(nan.sum()) > 0 and np.isnan(sums[0])
        d.set_integral("auto")             # the same customers, reached
        cust, (sums, n_unc) = d.customers(p, 39.0), d.eval(p)
    assert np.isfinite(cust).all() and n_unc == 0 and np.isfinite(sums).all()
    # device and model run the same algorithm and differ by the few ulp between the device's and glibc's
    # log / log1p / expm1 / exp / lgamma in each of a term's ~10 summands: far below 1e-12
    m = Q.model_customers_tail(e["x"], e["t_x"], e["T"], *p, "auto", 39.0)
    assert m["quadrature"][nan].all()
    for col, key in enumerate(("logL", "p_alive", "ey")):
        err = rel(cust[:, col], m[key]).max()
        print(f"past the cap in auto, {key} against the model: measured {err:.3g}, bound 1e-12")
        assert err <= 1e-12


# ---------------------------------------------------------------------------------------------
# auto below the switch is the series
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2357])
def test_auto_below_the_switch_has_the_bits_of_series(abe, n):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T = (a[:n] for a in abe)
    assert not Q.takes_quadrature("auto", tx, T, NEAR_OPT[1], NEAR_OPT[3]).any()
    with PnbdData(x, tx, T) as d:
        c0, (s0, u0), r0 = d.customers(NEAR_OPT, 39.0), d.eval(NEAR_OPT), d.customers_cov(NEAR_OPT, 39.0)
        d.set_integral("auto")
        c1, (s1, u1), r1 = d.customers(NEAR_OPT, 39.0), d.eval(NEAR_OPT), d.customers_cov(NEAR_OPT, 39.0)
    assert u0 == u1 == 0
    assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(r0), bits(r1))


# ---------------------------------------------------------------------------------------------
# the fixture grid
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "quadrature"])
@pytest.mark.parametrize("k", range(7))
def test_grid_against_the_exact_values(fx, mode, k):
    from mcmc_clv_model_amd.mle import PnbdData
    p = fx["params"][k]
    with PnbdData(fx["x"], fx["t_x"], fx["T"], integral=mode) as d:
        cust = d.customers(p, float(fx["t_star"]))
        rows = d.customers_cov(p, float(fx["t_star"]))
        sums, n_unc = d.eval(p)
    assert np.isfinite(cust).all() and np.isfinite(rows).all() and np.isfinite(sums).all() and n_unc == 0
    assert np.array_equal(bits(rows[:, :3]), bits(cust)) and sums[5] == float(len(fx["x"]))
    for col, key in enumerate(("logL", "p_alive", "ey")):
        err = rel(cust[:, col], fx[key][k]).max()
        print(f"set {k} {mode} {key}: measured {err:.3g}, bound {bound(fx['eref_' + key][k]):.3g}")
        assert err <= bound(fx["eref_" + key][k]), (key, err, int(np.argmax(rel(cust[:, col], fx[key][k]))))
    assert bits(sums[0]) == bits(R.device_sum(cust[:, 0]))
    scale = np.maximum(1.0, fx["grad_abs"][k])
    err = (np.abs(sums[1:5] - fx["grad_sum"][k]) / scale).max()
    print(f"set {k} {mode} gradient sums: measured {err:.3g}, bound {bound(fx['eref_grad'][k]):.3g}")
    assert err <= bound(fx["eref_grad"][k]), err
    err = (np.abs(rows[:, 3:7] - fx["grad"][k]) / scale).max()     # each customer's score on the same scale
    assert err <= bound(fx["eref_grad"][k]), err


# ---------------------------------------------------------------------------------------------
# both paths in one launch, and the fixed-order sums
# ---------------------------------------------------------------------------------------------
def mixed_table(abe, n):
    """n customers and one covariate on both processes.  gamma = (1, -1): z = 8 moves alpha_i / beta_i by e^16
    (z(t_x) of 0.9999, the series would need 10^5 terms), z = 0 leaves NEAR_OPT.  Lanes 0..63 alternate, lanes
    64..255 and every lane of a block between the first and the last take the quadrature, the last customer,
    the only live lane of its block, takes it too at n = 257 and the series at n = 513."""
    live = np.flatnonzero(abe[1] < abe[2])[:n]       # t_x < T: a customer with t_x = T has no integral at all
    x, tx, T = (a[live] for a in abe)
    z = np.full(n, 8.0)
    z[:64:2] = 0.0
    if n > 257:
        z[-1] = 0.0
    return x, tx, T, z.reshape(1, n), np.array(NEAR_OPT + (1.0, -1.0))


@pytest.mark.parametrize("n", [257, 513])
def test_mixed_paths_and_the_fixed_order_sums(abe, n):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T, z, p = mixed_table(abe, n)
    assert n % 256 == 1
    m = Q.model_customers_cov_tail(x, tx, T, p, z, z, "auto", 39.0)
    quad = m["quadrature"]
    assert quad[1:64:2].all() and not quad[:64:2].any()              # both paths inside the first wavefront
    assert quad[64:n - 1].all() and quad[-1] == (n == 257)           # whole wavefronts (n = 513: a whole block)
    with PnbdData(x, tx, T, integral="auto") as d:
        d.set_covariates(z, z)
        cust = d.customers_cov(p, 39.0)
        s1, u1 = d.eval_cov(p)
        s2, u2 = d.eval_cov(p)
        cust2 = d.customers_cov(p, 39.0)
    assert u1 == u2 == 0 and np.isfinite(cust).all()
    assert np.array_equal(bits(s1), bits(s2)) and np.array_equal(bits(cust), bits(cust2))
    want = [R.device_sum(cust[:, 0])] + [R.device_sum(cust[:, 3 + j]) for j in range(4)] + [float(n)]
    want += [R.device_sum(cust[:, 4] * -z[0]), R.device_sum(cust[:, 6] * -z[0])]
    assert np.array_equal(bits(s1), bits(np.array(want)))
    # and each lane is on the path the model says: the series lanes have the bits of a series-only handle
    ser = np.flatnonzero(~quad)
    with PnbdData(x[ser], tx[ser], T[ser]) as d:
        d.set_covariates(z[:, ser], z[:, ser])
        assert np.array_equal(bits(d.customers_cov(p, 39.0)), bits(cust[ser]))
    err = rel(cust[:, 0], m["logL"]).max()
    print(f"n = {n}: {int(quad.sum())} customers on the quadrature, log L against the model {err:.3g}")
    assert err <= 1e-13


# ---------------------------------------------------------------------------------------------
# the two evaluations where both work
# ---------------------------------------------------------------------------------------------
def test_quadrature_against_series_where_both_work(fx, abe):
    """2,357 rows at z(t_x) in [0.49, 0.97].  On the 64 rows of the fixture's sample each mode is within its bound
    of the exact value; on every row the two modes agree within the sum of the two bounds."""
    from mcmc_clv_model_amd.mle import PnbdData
    p, idx = fx["abe_params"], fx["abe_rows"]
    z = Q.z_tx(abe[1], p[1], p[3])
    assert 0.3 <= z.min() and z.max() <= 0.97
    out = {}
    with PnbdData(*abe) as d:
        for mode in ("series", "quadrature"):
            d.set_integral(mode)
            out[mode] = d.customers_cov(p, float(fx["t_star"]))
            assert d.eval(p)[1] == 0 and np.isfinite(out[mode]).all()
    cols = (("logL", slice(0, 1)), ("p_alive", slice(1, 2)), ("ey", slice(2, 3)), ("grad", slice(3, 7)))
    for key, c in cols:
        both = 0.0
        for mode in ("series", "quadrature"):
            b = bound(fx[f"abe_eref_{mode}_{key}"])
            both += b
            exact = fx["abe_" + key].reshape(len(idx), -1)
            err = rel(out[mode][idx][:, c], exact).max()
            print(f"{key} {mode} against mpmath on the sample: measured {err:.3g}, bound {b:.3g}")
            assert err <= b, (key, mode, err)
        err = rel(out["quadrature"][:, c], out["series"][:, c]).max()
        print(f"{key} quadrature against series on {len(z)} rows: measured {err:.3g}, bound {both:.3g}")
        assert err <= both, (key, err)


def test_dert_takes_p_alive_from_the_same_point(abe):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T, z, p = mixed_table(abe, 513)
    with PnbdData(x, tx, T, integral="auto") as d:
        d.set_covariates(z, z)
        cust, dert = d.customers_cov(p, 39.0), d.dert(p, 0.0027, np.inf)
    assert np.isfinite(dert).all() and (dert[:, 1] > 0.0).all()
    assert np.array_equal(bits(dert[:, 0]), bits(cust[:, 1]))


# ---------------------------------------------------------------------------------------------
# the fit the series cannot finish
# ---------------------------------------------------------------------------------------------
def test_full_cbs_covariate_fit_in_auto_reaches_the_recorded_optimum(fx):
    from mcmc_clv_model_amd import ParetoNBDFitter
    df = cdnow("full")
    f = ParetoNBDFitter(integral="auto").fit(df["x"], df["t_x"], df["T_cal"], covariates=df[["first_sales_scaled"]],
                                             standard_errors=True)
    se = f.standard_errors_.to_numpy()
    print(f"params {f.params_.to_numpy()}\nse {se}\nlog L {f.log_likelihood_:.4f} (recorded {float(fx['fit_logL']):.4f}), "
          f"{f.n_eval_} evaluations, max |gradient| {f.grad_norm_:.3g}")
    assert f.converged_ and f.n_unconverged_ == 0 and f.grad_norm_ <= 1e-7
    assert np.isfinite(se).all() and (se > 0.0).all()
    dev = np.abs(f.params_.to_numpy() - fx["fit_params"]) / fx["fit_se"]
    print(f"distance from the record in recorded standard errors {dev}")
    assert dev.max() <= 0.01
    # both covariances are central differences, with the same step, of gradients that agree to 1e-12 of
    # sum |terms|, taken 0.01 se apart at the most
    assert np.abs(se / fx["fit_se"] - 1.0).max() <= 1e-3
    assert abs(f.log_likelihood_ - float(fx["fit_logL"])) <= 1e-3
    assert f.log_likelihood_ > WALL_LOGL
    # the fitter's mode reaches the calls after the fit
    pa = f.conditional_probability_alive(df["x"][:300], df["t_x"][:300], df["T_cal"][:300],
                                         covariates=df[["first_sales_scaled"]][:300])
    assert np.isfinite(pa).all()

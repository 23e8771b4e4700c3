"""The maximum-marginal-likelihood kernels on the GPU (csrc/mml.hip): l_i bit for
bit clv_marginal_loglik's, the moments against the float64 model tests/mml_ref.py evaluated at the
device's own centres, the 2K + 6 sums in the fixed order bit for bit, NaN handling, and the fits of
the CDNOW tables against tests/golden/mml_fit.npz.  Every figure is printed before it is asserted."""
import functools
import warnings

import numpy as np
import pytest

from tests import marginal_ref as M
from tests import mml_ref as R
from tests.helpers import bits, cdnow, golden
from tests.test_gpu_marginal import c_marginal

pytestmark = pytest.mark.gpu

N = 600
T_STAR = 39.0
# The device's moments against the model at the device's centres, in units of marginal_ref.unit_tol of
# the column's scale (scale_of: 1 for P(alive), sqrt E[da da] for E[da], ...).  The device's exp / log
# differ from numpy's by an ulp, which passes through the 1,024-term sums; for the heavy buyers of the
# edge archetypes (x = 20,000) an ulp of mu is 2e-12 in (lambda + mu) t and so in a node's weight.
# Measured on an MI355X over K = 1, 2, 9 and the orders 8 .. 32: the largest deviation is 109 units
# (E[db db], K = 2, order 24; l itself stays below 0.09), held to 4 times 110.  DESIGN.md section 4n.
MEASURED_UNITS = 110.0
MOMENT_UNITS = 4.0 * MEASURED_UNITS
# theta-hat of the device's fit against the float64 model's (mml_fit.npz).  Both are roots of the score
# to max |score| <= 1e-7 only, so to first order they are apart by at most |H^-1| (|score| + |score'| + rounding),
# H the Jacobian of the score (the fit's hessian_), |.| the largest absolute row sum: the bound the
# test computes.  Measured on an MI355X: 3.5e-14 (K = 1) and 1.3e-14 (K = 2), far inside it, because
# the two optimisers take the same path there; that figure is a property of the paths, not of the
# code, and is printed, not held.


@functools.lru_cache(maxsize=None)
def case(K):
    """(record, arrays) of a device case: the 600 case customers and one CDNOW-like record."""
    df, names = M.case_customers(N, K, 17)
    rec = M.case_records(1, 2, K, 300 + K)[0]
    return rec, M.case_arrays(df, names, False)


def handle(K, arrays=None, w=None, sel=None):
    from mcmc_clv_model_amd.mle import MmlData
    cov, x, tx, T, _ = arrays or case(K)[1]
    sel = slice(None) if sel is None else sel
    return MmlData(x[sel], tx[sel], T[sel], w, None if cov is None else cov[:, sel].T, check_finite=False)


def scale_of(rows):
    """The scale of each column of clv_mml_customers' rows (the units of the moment tolerance)."""
    sa, sb = np.sqrt(rows[:, 4]), np.sqrt(rows[:, 6])
    return np.stack([np.maximum(1.0, np.abs(rows[:, 0])), np.ones(len(sa)), sa, sb, rows[:, 4], sa * sb, rows[:, 6],
                     np.abs(rows[:, 7])], axis=1)


def test_abi_exports_and_a_closed_handle():
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    for name in ("clv_mml_create", "clv_mml_destroy", "clv_mml_eval", "clv_mml_customers", "clv_debug_mml_eval"):
        assert hasattr(L, name), name
    rec, _ = case(1)
    d = handle(1)
    d.close()
    sums = np.full(8, -7.0)
    assert L.clv_mml_eval(d._h, _lib.dptr(rec), 0, _lib.dptr(sums), None) == -1          # CLV_EINVAL
    assert L.clv_mml_customers(d._h, _lib.dptr(rec), 0, 0.0, _lib.dptr(np.empty((N, 8)))) == -1
    assert np.all(sums == -7.0)
    info = _lib.mml_info()
    print("mml_info", info)
    assert info["eval_scratch_bytes"] == 0 and info["customers_scratch_bytes"] == 0
    assert info["eval_vgprs"] > 0 and info["customers_vgprs"] > 0 and info["block"] == 2 * info["customers"] == 512


@pytest.mark.parametrize("K", [1, 2, 9])
def test_loglik_is_the_marginal_likelihoods_bits_at_every_order(K):
    rec, arrays = case(K)
    with handle(K) as d:
        for nodes in M.ORDERS:
            rows = d.customers(rec, nodes, T_STAR)
            want, _ = c_marginal(rec[None], 2, K, arrays, nodes=nodes)
            assert np.isfinite(rows).all()
            assert np.array_equal(bits(rows[:, 0]), bits(want[0])), (K, nodes)
        assert np.array_equal(bits(d.customers(rec, 0, T_STAR)), bits(rows))             # 0: the default order, 32


@pytest.mark.parametrize("K", [1, 2, 9])
def test_moments_and_holdout_expectation_against_the_model(K):
    rec, arrays = case(K)
    cov, x, tx, T, _ = arrays
    worst = 0.0
    with handle(K) as d:
        for nodes in M.ORDERS:
            rows = d.customers(rec, nodes, T_STAR)
            _, cen = c_marginal(rec[None], 2, K, arrays, nodes=nodes, centre=True)
            want = R.customers(rec, K, cov, x, tx, T, nodes, T_STAR, centres=cen[0])
            dev = np.abs(rows - want) / M.unit_tol(scale_of(want))
            print(f"K={K} nodes={nodes}: worst |device - model| per column in units "
                  f"{np.array2string(dev.max(axis=0), precision=3)}")
            worst = max(worst, dev.max())
            assert ((rows[:, 1] >= 0.0) & (rows[:, 1] <= 1.0)).all() and (rows[:, 7] >= 0.0).all()
    print(f"K={K}: worst deviation {worst:.3g} units (held to {MOMENT_UNITS})")
    assert worst <= MOMENT_UNITS


@pytest.mark.parametrize("K", [1, 2, 9])
def test_sums_are_the_fixed_order_sums_of_the_rows(K):
    rec, arrays = case(K)
    cov = arrays[0]
    with handle(K) as d:
        rows = d.customers(rec, 0, 0.0)
        sums, nn = d.eval(rec)
        again, _ = d.eval(rec)
        grids = [d.eval(rec, 0, grid)[0] for grid in (1, 2)]
    want, _ = R.sums_of_rows(rows, K, cov)
    assert nn == 0 and sums.shape == (2 * K + 6,) and sums[1] == float(N)
    assert np.array_equal(bits(sums), bits(want))
    assert np.array_equal(bits(sums), bits(again))
    for g in grids:
        assert np.array_equal(bits(sums), bits(g))


def test_a_weight_of_two_is_the_customer_listed_twice():
    K = 2
    rec, arrays = case(K)
    cov, x, tx, T, _ = arrays
    with handle(K, w=np.full(N, 2.0)) as d:
        sw, _ = d.eval(rec)
        rows = d.customers(rec)
    twice = (np.tile(cov, 2), np.tile(x, 2), np.tile(tx, 2), np.tile(T, 2), None)
    with handle(K, arrays=twice) as d:
        sd, _ = d.eval(rec)
    # two fixed-order sums of the same 2N terms in different orders: each is within depth * 2^-53 of
    # sum |terms| of the exact sum, depth = 8 (block tree) + 1 (lane's partials) + 8 (final tree) additions
    terms = np.abs(R.sums_of_rows(np.abs(rows), K, np.abs(cov), np.full(N, 2.0))[0])
    tol = 2.0 * 17.0 * 2.0 ** -53 * terms
    print("weights: |weighted - listed twice| / tolerance", np.array2string(np.abs(sw - sd) / np.maximum(tol, 1e-300), precision=3))
    assert sw[1] == 2.0 * N == sd[1] and sw[2] == 0.0 == sd[2]
    assert (np.abs(sw - sd) <= tol).all()


def test_an_indefinite_sigma_and_a_nan_covariate():
    K = 2
    rec, arrays = case(K)
    cov, x, tx, T, _ = arrays
    bad = rec.copy()
    bad[2 * K + 1] = 10.0                                           # Sigma_01^2 > Sigma_00 Sigma_11
    with handle(K) as d:
        sums, nn = d.eval(bad)
        assert nn == N and np.isnan(sums[[0, 3, 4, 5]]).all() and np.isnan(sums[6:]).all() and sums[1] == float(N)
        assert np.isnan(d.customers(bad)).all()
        good = d.customers(rec, 0, T_STAR)
    cov2 = cov.copy()
    cov2[0, 301] = np.nan
    with handle(K, arrays=(cov2, x, tx, T, None)) as d:
        sums, nn = d.eval(rec)
        rows = d.customers(rec, 0, T_STAR)
    assert nn == 1 and np.isnan(sums[0]) and sums[2] == 1.0
    assert np.isnan(rows[301]).all()
    keep = np.arange(N) != 301
    assert np.array_equal(bits(rows[keep]), bits(good[keep]))


@functools.lru_cache(maxsize=None)
def abe_fit(K):
    from mcmc_clv_model_amd import LogNormalParetoNBDFitter
    df = cdnow("abe")
    cov = df[["first_sales_scaled"]] if K > 1 else None
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fit = LogNormalParetoNBDFitter().fit(df["x"], df["t_x"], df["T_cal"], covariates=cov, standard_errors=True,
                                             robust=True)
    return fit, df, cov


@pytest.mark.parametrize("K", [1, 2])
def test_the_abe_fit_lands_on_the_models(K):
    from mcmc_clv_model_amd.mle import MmlData, mml_record
    fit, df, cov = abe_fit(K)
    f = golden("mml_fit.npz")
    theta, ll = f[f"abe_k{K}_theta"], float(f[f"abe_k{K}_loglik"])
    move = np.abs(fit.theta_ - theta).max()
    hinv = np.abs(np.linalg.inv(-fit.hessian_)).sum(axis=1).max()
    # the two scores at the roots, and the rounding by which the device's score may differ from the model's
    # (every customer's moments at their tolerance)
    rounding = len(df) * float(M.unit_tol(1.0)) * MOMENT_UNITS
    THETA_TOL = hinv * (fit.grad_norm_ + float(f[f"abe_k{K}_score"]) + rounding)
    print(f"K={K}: converged {fit.converged_} in {fit.n_eval_} evaluations, max |score| {fit.grad_norm_:.3g}, "
          f"log L {fit.log_likelihood_:.6f} (model {ll:.6f}), |theta - model's| {move:.3g} (held to {THETA_TOL})")
    assert fit.converged_ and fit.grad_norm_ <= 1e-7 and fit.n_nonfinite_ == 0
    assert move <= THETA_TOL
    with MmlData(df["x"], df["t_x"], df["T_cal"], None, cov) as d:             # the value at the model's own theta
        sums, _ = d.eval(mml_record(theta, K), 32)
        rows = d.customers(mml_record(theta, K), 32)
    bound = M.unit_tol(rows[:, 0]).sum()
    print(f"K={K}: log L at the model's theta differs by {abs(sums[0] - ll):.3g} (bound {bound:.3g})")
    assert abs(sums[0] - ll) <= bound
    assert abs(fit.log_likelihood_ - ll) <= bound + 1e-9        # the two roots: the value is flat to second order
    se = fit.standard_errors_.to_numpy()
    assert np.isfinite(se).all() and (se > 0.0).all() and fit.summary_.shape == (2 * K + 4, 6)
    c = fit.covariance_.to_numpy()
    assert np.array_equal(c, c.T) and np.linalg.eigvalsh(c).min() > 0.0           # the robust covariance
    cols = dict(covariates=cov) if K > 1 else {}
    ll_i = fit.pointwise_log_likelihood(df["x"], df["t_x"], df["T_cal"], **cols)
    from mcmc_clv_model_amd import marginal_log_likelihood
    lm = marginal_log_likelihood(fit.as_level2_record(), df, list(cov.columns) if K > 1 else None)
    assert np.array_equal(bits(lm[0]), bits(ll_i))
    ic = fit.information_criteria(df["x"], df["t_x"], df["T_cal"], **cols)
    assert ic["kind"] == "marginal" and ic["n_params"] == 2 * K + 3


def test_the_covariate_is_significant_and_the_customers_are_scored():
    from mcmc_clv_model_amd import likelihood_ratio_test
    (f1, df, _), (f2, _, cov) = abe_fit(1), abe_fit(2)
    lr = likelihood_ratio_test(f1, f2)
    print("likelihood ratio", lr)
    assert lr["df"] == 2 and abs(lr["statistic"] - 24.5) < 0.1 and lr["p_value"] < 1e-4
    pa = f2.conditional_probability_alive(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    ex = f2.conditional_expected_number_of_purchases_up_to_time(39.0, df["x"], df["t_x"], df["T_cal"], covariates=cov)
    pm = f2.posterior_means(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    assert ((pa > 0.0) & (pa <= 1.0)).all() and (ex >= 0.0).all() and np.isfinite(pm.to_numpy()).all()
    s = f2.scores(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    assert s.shape == (len(df), 7) and np.abs(s.sum(axis=0)).max() <= 1e-6        # the rows add up to the score


def test_the_full_cbs_slice_with_its_far_covariate_converges():
    """The first 4,096 rows of the full CBS with first_sales_scaled (it reaches 14 sd and more): the
    case the gamma-mixed covariate MLE cannot finish.  The float64 model converges on this slice
    (tests/golden/mml_fit.npz, full_k2)."""
    from mcmc_clv_model_amd import LogNormalParetoNBDFitter
    f = golden("mml_fit.npz")
    df = cdnow("full", int(f["full_rows"]))
    assert df["first_sales_scaled"].abs().max() > 14.0
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fit = LogNormalParetoNBDFitter().fit(df["x"], df["t_x"], df["T_cal"], covariates=df[["first_sales_scaled"]])
    print(f"full CBS slice: {fit.n_eval_} evaluations, max |score| {fit.grad_norm_:.3g}, log L {fit.log_likelihood_:.6f} "
          f"(model {float(f['full_k2_loglik']):.6f})")
    assert fit.converged_ and fit.n_nonfinite_ == 0
    ll_i = fit.pointwise_log_likelihood(df["x"], df["t_x"], df["T_cal"], covariates=df[["first_sales_scaled"]])
    # the rounding of the 4,096 terms, and 1e-9 for the two roots (the value is flat to second order there)
    assert abs(fit.log_likelihood_ - float(f["full_k2_loglik"])) <= M.unit_tol(ll_i).sum() + 1e-9

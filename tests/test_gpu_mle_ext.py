"""GPU: the classical baseline's extensions against the exact fixtures of
tests/golden/mle_ext_*.npz (mpmath; made by tests/golden/make_mle_ext_goldens.py): the Pareto/NBD with
time-invariant covariates, the Hessian and standard errors, the Gamma-Gamma model, DERT and the classical CLV.
Neither mpmath nor a host fit is needed here.

Bound for a device value against the exact one, relative to max(1, |value|): 8 x the fixture's recorded error
of the float64 numpy model (E_ref), floor 64 ulp — section 4e's rule.  Gradient sums and Hessian entries are
scaled by sum |terms|."""
import math
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import mle_ext_ref as M
from tests import pnbd_ref as R
from tests.helpers import bits, cdnow, golden

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
NEAR_OPT = (0.55, 10.58, 0.61, 11.67)


def bound(e_ref):
    return max(8.0 * float(e_ref), 64.0 * ULP)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def fsum_err(got, terms):
    """|got - fsum(terms)| / max(1, fsum |terms|) per column."""
    terms = terms.reshape(len(terms), -1)
    want = np.array([math.fsum(terms[:, j]) for j in range(terms.shape[1])])
    scale = np.maximum(1.0, [math.fsum(np.abs(terms[:, j])) for j in range(terms.shape[1])])
    return np.abs(np.asarray(got) - want) / scale


def grads(sums):
    return np.concatenate([sums[1:5], sums[6:]])


@pytest.fixture(scope="module")
def abe():
    df = cdnow("abe")
    return (df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy(),
            df[["first_sales_scaled", "age_scaled"]].to_numpy(np.float64))


@pytest.fixture(scope="module")
def fits():
    """The plain and the covariate fit of abe, the latter with robust standard errors: fitted once."""
    from mcmc_clv_model_amd import ParetoNBDFitter
    df = cdnow("abe")
    plain = ParetoNBDFitter().fit(df["x"], df["t_x"], df["T_cal"])
    cov = ParetoNBDFitter().fit(df["x"], df["t_x"], df["T_cal"], covariates=df[["first_sales_scaled"]],
                                standard_errors=True, robust=True)
    return df, plain, cov


# ---------------------------------------------------------------------------------------------
# 1. bit identity with the plain kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2357])
def test_bit_identity_with_the_plain_kernels(abe, n):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T, Z = (a[:n] for a in abe)
    with PnbdData(x, tx, T) as d:
        cust = d.customers(NEAR_OPT, 39.0)
        s, u = d.eval(NEAR_OPT)
    for z1, z2 in ((Z, Z[:, :1]), (np.empty((n, 0)), np.empty((n, 0)))):
        p = np.concatenate([NEAR_OPT, np.zeros(z1.shape[1] + z2.shape[1])])
        with PnbdData(x, tx, T, covariates=z1, covariates_dropout=z2) as d:
            cc = d.customers_cov(p, 39.0)
            sc, uc = d.eval_cov(p)
            sc2, _ = d.eval_cov(p)
        assert cc.shape == (n, 7) and sc.shape == (6 + z1.shape[1] + z2.shape[1],)
        assert np.array_equal(bits(cc[:, :3]), bits(cust))              # log L, P(alive), E[Y]
        assert np.array_equal(bits(sc[:6]), bits(s)) and uc == u == 0   # the six sums of clv_pnbd_eval
        assert np.array_equal(bits(sc), bits(sc2))                      # two calls: the same bits
        for j in range(4):                                              # the scores are what the sums add
            assert bits(sc[1 + j]) == bits(R.device_sum(cc[:, 3 + j]))
        for k in range(z1.shape[1]):
            assert bits(sc[6 + k]) == bits(R.device_sum(-z1[:, k] * cc[:, 4])), k
        for k in range(z2.shape[1]):
            assert bits(sc[6 + z1.shape[1] + k]) == bits(R.device_sum(-z2[:, k] * cc[:, 6])), k


def test_replacing_the_covariates_of_a_handle(abe):
    """clv_pnbd_set_covariates swaps the handle's two covariate matrices and its two reduction buffers for new
    ones: K1 = K2 = 8, then 1 (23 sums to 9), then 0 on one handle of 257 customers (two blocks, one live lane
    in the second) give what a fresh handle with the same covariates gives, and the last the plain kernel's sums."""
    from mcmc_clv_model_amd.mle import PnbdData
    n = 257
    x, tx, T, _ = (a[:n] for a in abe)
    rng = np.random.default_rng(13)
    Z1, Z2 = rng.uniform(-1.0, 1.0, (n, 8)), rng.uniform(-1.0, 1.0, (n, 8))
    with PnbdData(x, tx, T) as d:
        s_plain, _ = d.eval(NEAR_OPT)
        for k in (8, 1, 0):
            z1, z2 = Z1[:, :k], Z2[:, :k]
            p = np.concatenate([NEAR_OPT, np.linspace(-0.15, 0.15, 2 * k)])
            d.set_covariates(z1.T, z2.T)
            with PnbdData(x, tx, T, covariates=z1, covariates_dropout=z2) as fresh:
                want_s, want_u = fresh.eval_cov(p)
                want_c = fresh.customers_cov(p, 39.0)
            s, u = d.eval_cov(p)
            assert s.shape == (6 + 2 * k,) and u == want_u == 0
            assert np.array_equal(bits(s), bits(want_s)), k
            assert np.array_equal(bits(d.customers_cov(p, 39.0)), bits(want_c)), k
        assert np.array_equal(bits(s), bits(s_plain))


@pytest.mark.parametrize("n", [1, 257])
def test_dert_on_a_handle_with_an_empty_covariate_set(abe, n):
    """clv_pnbd_dert reads K1 = K2 = 0 from a handle that never had covariates and from one given none."""
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T, _ = (a[:n] for a in abe)
    delta = math.log1p(0.15) / 52.0
    with PnbdData(x, tx, T) as d:
        never = [d.dert(NEAR_OPT, delta, H) for H in (np.inf, 52.0)]
    with PnbdData(x, tx, T, covariates=np.empty((n, 0))) as d:
        assert d.k1 == d.k2 == 0
        empty = [d.dert(NEAR_OPT, delta, H) for H in (np.inf, 52.0)]
    assert never[0].shape == (n, 2) and np.isfinite(never[0]).all()
    assert np.array_equal(bits(never), bits(empty))


# clv_pnbd_track against clv_pnbd_track_cov with K1 = K2 = 0, bit for bit: the last assertion of
# test_tracking_with_covariates (700 births in three blocks, 78 times) calls both entries.


# ---------------------------------------------------------------------------------------------
# 2. covariate edge grid against the quadrature
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_covariate_edge_grid_against_the_quadrature(k):
    from mcmc_clv_model_amd.mle import PnbdData
    g = golden("mle_ext_cov.npz")
    p = g["params"][k]
    assert g["swap"][k].any() and not g["swap"][k].all()     # alpha_i crosses beta_i within the frame
    assert not g["z1"][1].any() and p[5] != 0.0              # a column of zeros with a non-zero coefficient
    with PnbdData(g["x"], g["t_x"], g["T"], covariates=g["z1"].T, covariates_dropout=g["z2"].T) as d:
        cc = d.customers_cov(p, float(g["t_star"]))
        s, u = d.eval_cov(p)
    assert u == 0 and s[5] == 12.0
    for col, key in enumerate(("logL", "p_alive", "ey")):
        err = rel(cc[:, col], g[key][k]).max()
        print(f"set {k} {key}: measured {err:.3g}, bound {bound(g['eref_' + key][k]):.3g}")
        assert err <= bound(g["eref_" + key][k]), (k, key, err)
    err = (np.abs(grads(s) - g["grad_sum"][k]) / np.maximum(1.0, g["grad_abs"][k])).max()
    print(f"set {k} gradient sums: measured {err:.3g}, bound {bound(g['eref_grad'][k]):.3g}")
    assert err <= bound(g["eref_grad"][k]), (k, err)
    assert s[7] == 0.0                                       # the zero column's coefficient: exactly no gradient
    assert np.array_equal(bits(grads(s)), bits([R.device_sum(c) for c in M.theta_scores(cc[:, 3:7], g["z1"], g["z2"]).T]))


# ---------------------------------------------------------------------------------------------
# 3. strides and the widest reduction
# ---------------------------------------------------------------------------------------------
def test_the_widest_reduction_23_sums(abe):
    from mcmc_clv_model_amd.mle import PnbdData
    n = 257
    x, tx, T, _ = (a[:n] for a in abe)
    rng = np.random.default_rng(5)
    z1, z2 = rng.uniform(-1.0, 1.0, (n, 8)), rng.uniform(-1.0, 1.0, (n, 8))
    p = np.concatenate([NEAR_OPT, rng.uniform(-0.15, 0.15, 16)])
    with PnbdData(x, tx, T, covariates=z1, covariates_dropout=z2) as d:
        s, u = d.eval_cov(p)
        s2, _ = d.eval_cov(p)
        cc = d.customers_cov(p, 39.0)
    m = M.model_customers_cov(x, tx, T, p, z1.T, z2.T)
    err = np.concatenate([fsum_err(s[:1], m["logL"]), fsum_err(grads(s), m["scores"])])
    print(f"23 sums at n = 257: largest error {err.max():.3g} of sum |terms|, bound 1e-12")
    assert u == 0 and s[5] == float(n) and s.shape == (22,) and err.max() <= 1e-12
    assert np.array_equal(bits(s), bits(s2))
    want = [R.device_sum(c) for c in M.theta_scores(cc[:, 3:7], z1.T, z2.T).T]     # the grouping is not in the bits
    assert np.array_equal(bits(grads(s)), bits(want)) and bits(s[0]) == bits(R.device_sum(cc[:, 0]))


@pytest.mark.parametrize("n", [65_537, 524_545])
def test_covariates_beyond_one_grid_and_one_reduction_pass(abe, n):
    """The abe table tiled as in tests/test_gpu_pnbd.py (257 block partials; 2,050 blocks > PNBD_MAX_GRID),
    K1 = K2 = 1: a strided customer reads its own covariates and weight."""
    from mcmc_clv_model_amd.mle import PnbdData
    n0 = len(abe[0])
    idx = np.arange(n) % n0
    x, tx, T, Z = (a[idx] for a in abe)
    z = Z[:, :1]
    p = np.array(NEAR_OPT + (0.1, -0.05))      # first_sales_scaled reaches 14: larger coefficients pass the term cap
    with PnbdData(x, tx, T, covariates=z) as d:
        cc = d.customers_cov(p, 39.0)
        s1, u1 = d.eval_cov(p)
        s2, _ = d.eval_cov(p)
    assert cc.shape == (n, 7) and not np.isnan(cc).any()
    assert np.array_equal(bits(cc), bits(cc[:n0][idx]))                    # the bits of the first copy
    assert u1 == 0 and np.array_equal(bits(s1), bits(s2)) and s1[5] == float(n)
    assert bits(s1[0]) == bits(R.device_sum(cc[:, 0]))
    assert np.array_equal(bits(grads(s1)), bits([R.device_sum(c) for c in M.theta_scores(cc[:, 3:7], z.T, z.T).T]))
    m = M.model_customers_cov(*abe[:3], p, abe[3][:, :1].T, abe[3][:, :1].T)
    err = fsum_err(grads(s1), m["scores"][idx])
    print(f"n = {n} covariate gradient sums: measured {err.max():.3g} of sum |terms|, bound 1e-12")
    assert err.max() <= 1e-12
    w = np.zeros(n)
    w[-300:] = 1.0
    with PnbdData(x, tx, T, w, covariates=z) as d:
        sw, uw = d.eval_cov(p)
    with PnbdData(x[-300:], tx[-300:], T[-300:], covariates=z[-300:]) as d:
        s300, _ = d.eval_cov(p)
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert sw[5] == 300.0 == s300[5] and uw == 0
    assert np.allclose(sw[keep], s300[keep], rtol=1e-13, atol=0)


def test_tracking_with_covariates(abe):
    from mcmc_clv_model_amd import ParetoNBDFitter, pnbd_weekly_tracking
    rng = np.random.default_rng(11)
    n = 700
    birth, times = rng.integers(1, 91, n), np.arange(1, 79)
    z = abe[3][:n, :1]
    f = ParetoNBDFitter()
    f.params_ = pd.Series(NEAR_OPT + (0.3, -0.2), index=["r", "alpha", "s", "beta", "purchase:z", "dropout:z"])
    f._k = (1, 1)
    cum = pnbd_weekly_tracking(f, birth, times, covariates=z)
    rel_t = np.clip(times[None, :] - birth[:, None], 0, None).astype(np.float64)
    per = f.expected_number_of_purchases_up_to_time(rel_t[0], covariates=z)
    assert per.shape == (n, 78)                                  # one row per customer
    a, b = M.customer_scales(f.params_.to_numpy(), z.T, z.T)
    part = NEAR_OPT[0] * b[:, None] / a[:, None] * R.phi(NEAR_OPT[2] - 1.0, np.log1p(rel_t / b[:, None]))
    assert np.allclose(cum, [R.device_sum(c) for c in part.T], rtol=1e-13, atol=0)
    assert (np.diff(cum) >= 0).all() and cum[-1] > 0
    f0 = ParetoNBDFitter()
    f0.params_ = pd.Series(NEAR_OPT, index=["r", "alpha", "s", "beta"])
    f._k, f.params_ = (0, 0), f0.params_                         # no column: the plain curve, bit for bit
    assert np.array_equal(bits(pnbd_weekly_tracking(f, birth, times, covariates=np.empty((n, 0)))),
                          bits(pnbd_weekly_tracking(f0, birth, times)))


# ---------------------------------------------------------------------------------------------
# 4. fit   5. Hessian and standard errors
# ---------------------------------------------------------------------------------------------
def test_covariate_fit_reaches_the_golden_optimum(fits):
    from mcmc_clv_model_amd import likelihood_ratio_test
    df, plain, f = fits
    g = golden("mle_ext_fit.npz")
    print(f.params_.to_dict(), f.log_likelihood_, f.n_iter_, f.n_eval_, f.grad_norm_)
    assert f.converged_ is True and f.grad_norm_ <= 1e-7 and f.n_unconverged_ == 0
    assert list(f.params_.index) == ["r", "alpha", "s", "beta", "purchase:first_sales_scaled", "dropout:first_sales_scaled"]
    assert abs(f.log_likelihood_ - float(g["cov_logL"])) <= 1e-6
    assert np.allclose(f.params_.to_numpy(), g["cov_params"], rtol=1e-4, atol=0)
    assert f.log_likelihood_ >= plain.log_likelihood_                 # nested models
    t = likelihood_ratio_test(plain, f)
    assert t["statistic"] == 2.0 * (f.log_likelihood_ - plain.log_likelihood_) and t["df"] == 2
    assert 0.0 <= t["p_value"] <= 1.0
    print("likelihood-ratio test of first_sales_scaled:", t)
    cov = df[["first_sales_scaled"]]
    ic = f.information_criteria(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    assert ic["n_params"] == 6 and ic["kind"] == "marginal"
    ll = f.pointwise_log_likelihood(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    assert abs(ll.sum() - f.log_likelihood_) <= 1e-9 * abs(f.log_likelihood_)
    assert abs(float(ic["pointwise"]["elpd_loo"].sum()) - (ll.sum() - 6.0)) <= 1e-8
    pa = f.conditional_probability_alive(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    ey = f.conditional_expected_number_of_purchases_up_to_time(39.0, df["x"], df["t_x"], df["T_cal"], covariates=cov)
    assert (pa > 0).all() and (pa <= 1).all() and (ey >= 0).all()


def test_hessian_against_mpmath():
    from mcmc_clv_model_amd import ParetoNBDFitter
    g = golden("mle_ext_hessian.npz")
    f = ParetoNBDFitter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # theta is no optimum: -H need not be definite
        H = f.hessian(g["x"], g["t_x"], g["T"], covariates=g["z1"].T, covariates_dropout=g["z2"].T, theta=g["theta"])
    assert H.shape == (6, 6) and np.array_equal(H, H.T)
    err = (np.abs(H - g["hessian"]) / np.maximum(1.0, g["hessian_abs"])).max()
    print(f"central-difference Hessian: measured {err:.3g}, bound {bound(g['eref']):.3g} (step 2^{np.log2(g['step']):.0f})")
    assert err <= bound(g["eref"])


def test_standard_errors_of_the_covariate_fit(fits):
    from mcmc_clv_model_amd import ParetoNBDFitter
    df, _, f = fits
    g = golden("mle_ext_fit.npz")
    cov = df[["first_sales_scaled"]]
    assert np.isfinite(f.standard_errors_.to_numpy()).all() and (f.standard_errors_ > 0).all()
    assert list(f.summary_.columns) == ["estimate", "se", "z", "p", "ci_lower", "ci_upper"]
    assert (f.summary_["ci_lower"] < f.summary_["estimate"]).all() and (f.summary_["estimate"] < f.summary_["ci_upper"]).all()
    # robust: the numpy sandwich of the returned scores
    S = f.scores(df["x"], df["t_x"], df["T_cal"], covariates=cov)
    Hi = np.linalg.inv(f.hessian_)
    want = Hi @ (S.T @ S) @ Hi
    assert S.shape == (len(df), 6)
    assert np.abs(f.covariance_.to_numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the model's standard errors at the same theta and the same step
    p = g["cov_params"]
    h = ParetoNBDFitter()
    h.hessian(df["x"], df["t_x"], df["T_cal"], covariates=cov, theta=np.concatenate([np.log(p[:4]), p[4:]]))
    err = np.abs(h.standard_errors_.to_numpy() / g["cov_se"] - 1.0).max()
    print(f"standard errors against the model's: largest relative deviation {err:.3g}, bound 1e-6")
    print(h.summary_)
    assert err <= 1e-6
    assert np.allclose(h.covariance_.to_numpy(), np.linalg.inv(-h.hessian_), rtol=1e-12, atol=0)


def test_an_indefinite_hessian_gives_nan_and_one_warning():
    from mcmc_clv_model_amd import ParetoNBDFitter
    g = golden("mle_ext_hessian.npz")
    f = ParetoNBDFitter()
    theta = np.array(g["indefinite_theta"])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        H = f.hessian(g["x"], g["t_x"], g["T"], covariates=g["z1"].T, covariates_dropout=g["z2"].T, theta=theta)
    assert np.isfinite(H).all() and np.linalg.eigvalsh(-H).min() < 0.0
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert np.isnan(f.standard_errors_.to_numpy()).all() and np.isnan(f.covariance_.to_numpy()).all()
    assert np.isnan(f.summary_["se"].to_numpy()).all()


# ---------------------------------------------------------------------------------------------
# 6. Gamma-Gamma
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_gamma_gamma_edge_grid_against_mpmath(k):
    from mcmc_clv_model_amd.mle import GammaGammaFitter, GgData
    g = golden("mle_ext_gg.npz")
    p = g["params"][k]
    with GgData(g["n"], g["m"]) as d:
        c = d.customers(p)
    f = GammaGammaFitter()
    f.params_ = pd.Series(p, index=["p", "q", "gamma"])
    mean = f.conditional_expected_average_profit(g["n"], g["m"])
    for name, got, want in (("logL", c[:, 0], g["logL"][k]), ("grad", c[:, 1:], g["grad"][k]), ("mean", mean, g["mean"][k])):
        err = rel(got, want).max()
        print(f"set {k} {name}: measured {err:.3g}, bound {bound(g['eref_' + name][k]):.3g}")
        assert err <= bound(g["eref_" + name][k]), (k, name, err)


def test_device_digamma_against_mpmath():
    from mcmc_clv_model_amd.mle import device_digamma
    g = golden("mle_ext_gg.npz")
    x = g["psi_x"]
    assert x.min() < 1e-100 and x.max() == 1e6
    err = rel(device_digamma(x), g["psi"]).max()
    print(f"digamma on [{x.min():.3g}, {x.max():.3g}]: measured {err:.3g}, bound {bound(g['eref_psi']):.3g}")
    assert err <= bound(g["eref_psi"])


def gg_rows(df):
    n = df["x"].to_numpy() + 1
    m = df["sales"].to_numpy() / n
    return n[m > 0], m[m > 0]


@pytest.mark.parametrize("n", [1, 256, 257])
def test_gamma_gamma_block_edges_fixed_order_sums(n):
    from mcmc_clv_model_amd.mle import GgData
    nn, m = (a[:n] for a in gg_rows(cdnow("abe")))
    p = (6.25, 3.74, 15.44)
    with GgData(nn, m) as d:
        c = d.customers(p)
        s1, s2 = d.eval(p), d.eval(p)
    assert np.array_equal(bits(s1), bits(s2)) and s1[4] == float(n)
    assert np.array_equal(bits(s1[:4]), bits([R.device_sum(c[:, j]) for j in range(4)]))
    mod = M.model_gg_customers(nn, m, p)
    assert fsum_err(s1[1:4], mod["grad"]).max() <= 1e-12 and fsum_err(s1[:1], mod["logL"]).max() <= 1e-12
    with GgData(nn, m, np.full(n, 2.0)) as d:
        sw = d.eval(p)
    assert sw[4] == 2.0 * n and np.allclose(sw, 2.0 * s1, rtol=1e-13, atol=0)


def test_gamma_gamma_fit_reaches_the_golden_optimum():
    from mcmc_clv_model_amd import GammaGammaFitter
    g = golden("mle_ext_fit.npz")
    nn, m = gg_rows(cdnow("abe"))
    assert len(nn) == int(g["gg_n"])
    f = GammaGammaFitter()
    assert f.fit(nn, m, standard_errors=True) is f
    print(f.params_.to_dict(), f.log_likelihood_, f.n_iter_, f.n_eval_, f.grad_norm_)
    print(f.summary_)
    assert f.converged_ is True and f.grad_norm_ <= 1e-7 and list(f.params_.index) == ["p", "q", "gamma"]
    assert abs(f.log_likelihood_ - float(g["gg_logL"])) <= 1e-6
    assert np.allclose(f.params_.to_numpy(), g["gg_params"], rtol=1e-4, atol=0)
    assert (f.standard_errors_ > 0).all() and np.isfinite(f.summary_.to_numpy()).all()
    ll = f.pointwise_log_likelihood(nn, m)
    assert abs(ll.sum() - f.log_likelihood_) <= 1e-9 * abs(f.log_likelihood_)
    # the population mean and the n = 0 path
    p, q, gam = f.params_.to_numpy()
    pop = f.conditional_expected_average_profit()
    assert pop.shape == (1,) and pop[0] == p * gam / (q - 1.0)
    mixed = f.conditional_expected_average_profit([0, 3, 0], [0.0, 20.0, np.nan])
    assert mixed[0] == mixed[2] == pop[0] and mixed[1] == p * (gam + 60.0) / (3 * p + q - 1.0)
    f.params_ = pd.Series([p, 0.9, gam], index=["p", "q", "gamma"])
    assert np.isnan(f.conditional_expected_average_profit()[0])         # q <= 1: no population mean


# ---------------------------------------------------------------------------------------------
# 7. DERT
# ---------------------------------------------------------------------------------------------
def test_dert_integral_grid_against_the_quadrature():
    from mcmc_clv_model_amd.mle import device_dert_integral
    g = golden("mle_ext_dert.npz")
    assert len(g["J"]) == 8 * 5 * 4
    J = device_dert_integral(g["s"], g["B"], g["delta"], g["H"])
    err = rel(J, g["J"])
    print(f"DERT integral on s x z x H: measured {err.max():.3g} (integer s {err[g['integer']].max():.3g}), "
          f"bound {bound(g['eref']):.3g}")
    assert err.max() <= bound(g["eref"])
    ok = np.abs(J / g["J"] - 1.0)                     # a horizon of 1e-3 is still known to its own size
    assert ok.max() <= 64 * ULP + 8 * float(g["eref"]), ok.max()


@pytest.mark.parametrize("k", [0, 1])
def test_dert_per_customer_against_mpmath(k):
    from mcmc_clv_model_amd import ParetoNBDFitter
    g = golden("mle_ext_dert.npz")
    f = ParetoNBDFitter()
    f.params_ = pd.Series(g["cust_params"][k], index=["r", "alpha", "s", "beta"])
    x, tx, T = g["x"], g["t_x"], g["T"]
    assert abs(float(g["cust_delta"]) - math.log1p(0.15) / 52.0) == 0.0
    inf = f.discounted_expected_transactions(x, tx, T)
    h52 = f.discounted_expected_transactions(x, tx, T, horizon=52.0)
    for name, got, want in (("H = inf", inf, g["cust_dert"][k, 0]), ("H = 52", h52, g["cust_dert"][k, 1])):
        err = rel(got, want).max()
        print(f"set {k} DERT {name}: measured {err:.3g}, bound {bound(g['eref_cust'][k]):.3g}")
        assert err <= bound(g["eref_cust"][k])
    prev = np.zeros(len(x))
    for H in (1e-3, 1.0, 52.0, 520.0, 5200.0):
        cur = f.discounted_expected_transactions(x, tx, T, horizon=H)
        assert (cur > prev).all() and (cur <= inf).all(), H
        prev = cur


def test_classical_lifetime_value_is_dert_times_spend(fits):
    from mcmc_clv_model_amd import GammaGammaFitter, classical_lifetime_value
    df, plain, cov = fits
    df = df.iloc[:600]
    gg = GammaGammaFitter()
    gg.params_ = pd.Series([6.25, 3.74, 15.44], index=["p", "q", "gamma"])
    n = df["x"].to_numpy() + 1
    m = df["sales"].to_numpy() / n
    n = np.where(m > 0, n, 0)
    out = classical_lifetime_value(plain, gg, df, monetary_frequency=n, monetary_value=m)
    assert list(out.columns) == ["p_alive", "dert", "expected_spend", "clv"] and out.index.equals(df.index)
    assert np.array_equal(bits(out["clv"]), bits(out["dert"].to_numpy() * out["expected_spend"].to_numpy()))
    assert np.array_equal(bits(out["dert"]), bits(plain.discounted_expected_transactions(df["x"], df["t_x"], df["T_cal"])))
    assert np.array_equal(bits(out["p_alive"]), bits(plain.conditional_probability_alive(df["x"], df["t_x"], df["T_cal"])))
    assert np.array_equal(bits(out["expected_spend"]), bits(gg.conditional_expected_average_profit(n, m)))
    assert (out["clv"] > 0).all()
    z = df[["first_sales_scaled"]]
    oc = classical_lifetime_value(cov, gg, df, monetary_frequency=n, monetary_value=m, covariates=z, horizon=104.0)
    assert (oc["dert"] < cov.discounted_expected_transactions(df["x"], df["t_x"], df["T_cal"], covariates=z)).all()


# ---------------------------------------------------------------------------------------------
# 8. validation
# ---------------------------------------------------------------------------------------------
def test_einval_paths_leave_the_handle_usable(abe, fits):
    from mcmc_clv_model_amd.mle import GgData, PnbdData, device_dert_integral
    x, tx, T, Z = (a[:300] for a in abe)
    p = np.array(NEAR_OPT + (0.1, 0.0, -0.1))
    with PnbdData(x, tx, T, covariates=Z, covariates_dropout=Z[:, :1]) as d:
        s0, _ = d.eval_cov(p)
        L, h = d._L, d._h
        from mcmc_clv_model_amd._lib import dptr
        zz = np.zeros((9, 300))
        assert L.clv_pnbd_set_covariates(h, 9, dptr(zz), 0, None) == -1 and b"0..8" in L.clv_last_error()
        assert L.clv_pnbd_set_covariates(h, 1, None, 0, None) == -1
        zz[0, 7] = np.inf
        assert L.clv_pnbd_set_covariates(h, 1, dptr(zz), 0, None) == -1 and b"non-finite" in L.clv_last_error()
        for bad in (np.r_[0.0, p[1:]], np.r_[p[:4], np.nan, 0.0, 0.0], np.r_[p[:6], np.inf]):
            with pytest.raises(ValueError):
                d.eval_cov(bad)
            with pytest.raises(ValueError):
                d.customers_cov(bad, 39.0)
            with pytest.raises(ValueError):
                d.dert(bad, 0.01, np.inf)
        with pytest.raises(ValueError, match="t_star"):
            d.customers_cov(p, -1.0)
        for delta, H in ((0.0, np.inf), (-0.1, 10.0), (np.nan, 10.0), (0.01, 0.0), (0.01, np.nan)):
            with pytest.raises(ValueError):
                d.dert(p, delta, H)
        s1, _ = d.eval_cov(p)
        assert np.array_equal(bits(s0), bits(s1))              # the covariates the handle had are still there
        assert np.isfinite(d.dert(p, 0.0, 52.0)).all()         # no discounting needs a finite horizon only
    with PnbdData(x, tx, T) as d:                               # a handle without covariates
        assert d._L.clv_pnbd_eval_cov(d._h, dptr(np.array(NEAR_OPT)), dptr(np.empty(6)), None) == -1
        assert np.isfinite(d.dert(NEAR_OPT, 0.01, np.inf)).all()
    for kw in (dict(covariates=np.zeros((300, 9))), dict(covariates=np.zeros((299, 1))),
               dict(covariates=np.full((300, 1), np.nan)), dict(covariates=Z, covariates_dropout=np.zeros((300, 2, 2))),
               dict(covariates_dropout=Z)):
        with pytest.raises(ValueError):
            PnbdData(x, tx, T, **kw)
    df, plain, cov = fits
    a = (df["x"], df["t_x"], df["T_cal"])
    for call in (lambda: cov.conditional_probability_alive(*a), lambda: cov.pointwise_log_likelihood(*a),
                 lambda: cov.information_criteria(*a), lambda: cov.discounted_expected_transactions(*a),
                 lambda: cov.conditional_expected_number_of_purchases_up_to_time(39.0, *a),
                 lambda: cov.conditional_probability_alive(*a, covariates=df[["first_sales_scaled", "age_scaled"]]),
                 lambda: plain.conditional_probability_alive(*a, covariates=df[["first_sales_scaled"]]),
                 lambda: plain.discounted_expected_transactions(*a, discount_rate=0.0),
                 lambda: plain.discounted_expected_transactions(*a, horizon=-1.0)):
        with pytest.raises(ValueError):
            call()
    assert np.isfinite(cov.conditional_probability_alive(*a, covariates=df[["first_sales_scaled"]])).all()
    with pytest.raises(ValueError):
        device_dert_integral([1.0], [10.0], [0.0], [np.inf])
    for n, m in (([0, 1], [1.0, 1.0]), ([1, 2], [1.0, 0.0]), ([1, 2], [1.0, -3.0]), ([1, 2], [np.nan, 1.0]), ([1.5], [1.0])):
        with pytest.raises(ValueError):
            GgData(n, m)
    with GgData([1, 2], [3.0, 4.0]) as d:
        e0 = d.eval((1.0, 2.0, 3.0))
        for bad in ((0.0, 1, 1), (1, np.inf, 1), (1, 1, np.nan)):
            with pytest.raises(ValueError):
                d.eval(bad)
            with pytest.raises(ValueError):
                d.customers(bad)
        assert np.array_equal(bits(e0), bits(d.eval((1.0, 2.0, 3.0))))

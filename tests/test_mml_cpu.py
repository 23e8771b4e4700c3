"""CPU: the float64 model of the maximum-marginal-likelihood kernels (tests/mml_ref.py, DESIGN.md
section 4n) against the exact moments of tests/golden/mml_exact.npz, Fisher's identity on the exact
side, the score-driven optimiser, the model's fits of the CDNOW table, and the host algebra of
mcmc_clv_model_amd.mle (log-Cholesky chain rule, delta method, summary)."""
import functools
import os

import numpy as np

from tests import marginal_ref as M
from tests import mml_ref as R
from tests.helpers import cdnow, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clv_mml_create", "clv_mml_destroy", "clv_mml_eval", "clv_mml_customers", "clv_debug_mml_eval",
               "clv_mml_info")
# The order-32 model against the exact fixture, relative to each column's scale (scale_of): the largest
# error over the fixture's 40 cells is 1.25e-6 (E[X*]; the five moments 2.9e-7, P(alive) 4.2e-8, l 9.5e-9),
# held to 4 times that for cells not sampled.  Order 8 reaches 3.2e-3 on the same cells.
MOMENT_TOL = 4.0 * 1.25e-6


def scale_of(rows):
    sa, sb = np.sqrt(rows[:, 4]), np.sqrt(rows[:, 6])
    return np.stack([np.maximum(1.0, np.abs(rows[:, 0])), np.ones(len(sa)), sa, sb, rows[:, 4], sa * sb, rows[:, 6],
                     np.abs(rows[:, 7])], axis=1)


def test_header_declares_and_library_exports_the_new_symbols():
    from mcmc_clv_model_amd import _lib
    import mcmc_clv_model_amd as pkg
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported"
    assert "LogNormalParetoNBDFitter" in pkg.__all__ and callable(pkg.LogNormalParetoNBDFitter)


def model_errors(nodes):
    f = golden("mml_exact.npz")
    errs = []
    for r in range(f["level2"].shape[0]):
        rows = R.customers(f["level2"][r], 2, f["cov"], f["x"], f["t_x"], f["T_cal"], nodes, float(f["t_star"]))
        errs.append(np.abs(rows - f["exact"][r]) / scale_of(f["exact"][r]))
    return np.array(errs)


def test_model_moments_against_the_exact_fixture():
    f = golden("mml_exact.npz")
    assert float(f["panel_gap"]) < 1e-10 and f["exact"].shape == (4, 10, 8)
    e32, e8 = model_errors(32), model_errors(8)
    print("order 32, worst per column", np.array2string(e32.max(axis=(0, 1)), precision=3))
    print("order  8, worst per column", np.array2string(e8.max(axis=(0, 1)), precision=3))
    assert e32.max() <= MOMENT_TOL
    # order 8 is visibly worse on the same cells, in every column: a constant could not pass both
    assert (e8.max(axis=(0, 1)) > 10.0 * e32.max(axis=(0, 1))).all() and e8.max() > 100.0 * MOMENT_TOL


def test_fishers_identity_on_the_exact_side():
    """P E[(da, db)] and P (S - Sigma) P / 2 from the fixture's exact moments against central differences of
    the fixture's exact l in (m_0, m_1, Sigma_00, Sigma_01, Sigma_11).  The differences at h and h / 2 are
    Richardson-extrapolated; the extrapolant's error is of higher order in h than the correction it
    applies, so the correction bounds it, plus the rounding of l (the panel gap) over the step."""
    f = golden("mml_exact.npz")
    K, rec, h, gap = 2, f["level2"][0], float(f["shift_h"]), float(f["panel_gap"])
    s00, s01, s11 = rec[2 * K:]
    det = s00 * s11 - s01 * s01
    P = np.array([[s11, -s01], [-s01, s00]]) / det
    for cell in range(f["shift_l"].shape[0]):
        l, _, eda, edb, saa, sab, sbb, _ = f["exact"][0, cell]
        gm = P @ np.array([eda, edb])
        G = 0.5 * P @ (np.array([[saa, sab], [sab, sbb]]) - np.array([[s00, s01], [s01, s11]])) @ P
        want = np.array([gm[0], gm[1], G[0, 0], 2.0 * G[0, 1], G[1, 1]])      # Sigma_01 stands for both off-diagonals
        for j, p in enumerate((0, K, 2 * K, 2 * K + 1, 2 * K + 2)):
            up, dn, up2, dn2 = f["shift_l"][cell, j]
            d1 = (up - dn) / ((rec[p] + h) - (rec[p] - h))
            d2 = (up2 - dn2) / ((rec[p] + 0.5 * h) - (rec[p] - 0.5 * h))
            est = (4.0 * d2 - d1) / 3.0
            tol = abs(d2 - d1) / 3.0 + 8.0 * gap * max(1.0, abs(l)) / h
            print(f"cell {cell} parameter {j}: identity {want[j]:.12g}, difference {est:.12g}, apart {abs(est - want[j]):.3g} "
                  f"(tolerance {tol:.3g})")
            assert abs(est - want[j]) <= tol
            assert tol <= 1e-3 * max(1.0, abs(want[j]))          # the check has teeth


def test_the_score_optimiser_finds_the_scores_root_where_the_value_disagrees():
    from mcmc_clv_model_amd.mle import minimize_bfgs, minimize_bfgs_score
    rng = np.random.default_rng(5)
    B = rng.standard_normal((5, 5))
    A = B @ B.T + 5.0 * np.eye(5)
    a, off = rng.standard_normal(5), 1e-2 * rng.standard_normal(5)

    def vg(x):                      # the value's minimum is a; the "gradient" vanishes at a + off
        return 0.5 * (x - a) @ A @ (x - a), A @ (x - a - off)

    res = minimize_bfgs_score(vg, np.full(5, 3.0), 1e-10, 200)
    assert res.converged and res.grad_norm <= 1e-10 and np.abs(res.x - (a + off)).max() <= 1e-10
    old = minimize_bfgs(vg, np.full(5, 3.0), 1e-10, 200)
    assert not old.converged and np.abs(old.x - (a + off)).max() > 1e-4
    # a consistent objective: both find the minimum
    good = minimize_bfgs_score(lambda x: (vg(x)[0], A @ (x - a)), np.full(5, 3.0), 1e-10, 200)
    assert good.converged and np.abs(good.x - a).max() <= 1e-10
    # a non-finite start and a non-finite trial
    assert not minimize_bfgs_score(lambda x: (np.nan, x), np.zeros(2)).converged

    def wall(x):
        return (np.nan, x * np.nan) if x[0] > 2.0 else (0.5 * float(x @ x), x.copy())
    w = minimize_bfgs_score(wall, np.array([1.9, -4.0]), 1e-10, 100)
    assert w.converged and np.abs(w.x).max() <= 1e-10


@functools.lru_cache(maxsize=None)
def model_fit(K):
    """The float64 model fitted to the abe CBS: K = 1 from the default start, K = 2 from K = 1's root."""
    from mcmc_clv_model_amd.mle import minimize_bfgs_score
    df = cdnow("abe")
    x, t_x, T_cal = df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float)
    if K == 1:
        cov, start = None, R.default_start(1, x, t_x, T_cal)
    else:
        cov = np.ascontiguousarray(df[["first_sales_scaled"]].to_numpy(float).T)
        t1 = model_fit(1).x
        start = np.array([t1[0], 0.0, t1[1], 0.0, t1[2], t1[3], t1[4]])
    return minimize_bfgs_score(R.objective(K, cov, x, t_x, T_cal), start, 1e-7, 200)


def test_the_models_fit_of_the_abe_cbs():
    f = golden("mml_fit.npz")
    published = {1: -9573.413, 2: -9561.180}
    for K in (1, 2):
        res = model_fit(K)
        theta, ll = f[f"abe_k{K}_theta"], float(f[f"abe_k{K}_loglik"])
        print(f"K={K}: {res.n_eval} evaluations, max |score| {res.grad_norm:.3g}, log L {-res.fun:.6f}, "
              f"|theta - fixture| {np.abs(res.x - theta).max():.3g}, record {R.record_of(res.x, K)}")
        assert res.converged and res.grad_norm <= 1e-7
        # two roots to |score| <= 1e-7 each: apart by at most |H^-1| 2e-7, the entries of H^-1 (the
        # parameters' variances) below 0.05; the value is flat to second order there
        assert np.abs(res.x - theta).max() <= 1e-6 and abs(-res.fun - ll) <= 1e-8
        assert abs(ll - published[K]) < 1e-3        # the figures are given to three decimals: one unit of the last
    lr = 2.0 * (float(f["abe_k2_loglik"]) - float(f["abe_k1_loglik"]))
    assert abs(lr - 24.5) < 0.1
    assert bool(f["full_k2_score"] <= 1e-7) and int(f["full_rows"]) == 4096    # the full-CBS slice converged too


def test_log_cholesky_chain_rule_on_a_closed_form():
    """With the likelihood a point mass at y, l = log N2(y; m, Sigma), E[(da, db)] = y - m and S = (y - m)(y - m)':
    mle.mml_score of those moments is the gradient of the closed form in theta = (m, c0, c1, c2)."""
    from mcmc_clv_model_amd.mle import log_cholesky_sigma, mml_score, sigma_log_cholesky
    y = np.array([0.7, -1.1])

    def logn(theta):
        d = y - theta[:2]
        s00, s01, s11 = log_cholesky_sigma(theta[2:])
        det = s00 * s11 - s01 * s01
        return -np.log(2.0 * np.pi) - 0.5 * np.log(det) - 0.5 * (s11 * d[0] ** 2 - 2.0 * s01 * d[0] * d[1] + s00 * d[1] ** 2) / det

    theta = np.array([0.2, -0.4, 0.15, -0.6, 0.4])
    d = y - theta[:2]
    got = mml_score(theta, 1, np.array([d[0]]), np.array([d[1]]), np.array([d[0] ** 2, d[0] * d[1], d[1] ** 2]), np.float64(1.0))
    h = 2.0 ** -17
    want = np.array([(logn(theta + h * e) - logn(theta - h * e)) / (2.0 * h) for e in np.eye(5)])
    print("chain rule: closed form", want, "mml_score", got)
    assert np.abs(got - want).max() <= 1e-8        # h^2 / 6 times third derivatives of order 10
    assert np.abs(got - R.score_of_sums(np.array([0, 1.0, 0, d[0] ** 2, d[0] * d[1], d[1] ** 2, d[0], d[1]]), theta, 1)).max() <= 1e-14
    assert np.abs(sigma_log_cholesky(log_cholesky_sigma(theta[2:])) - theta[2:]).max() <= 1e-15


def test_delta_method_and_the_summary_shape():
    from mcmc_clv_model_amd.mle import LogNormalParetoNBDFitter, mml_params
    theta = np.array([-3.4, 0.2, -3.6, 0.1, 0.1, 0.2, 0.6])
    p, J = mml_params(theta, 2)
    h = 2.0 ** -17
    Jn = np.array([(mml_params(theta + h * e, 2)[0] - mml_params(theta - h * e, 2)[0]) / (2.0 * h) for e in np.eye(7)]).T
    assert np.abs(J - Jn).max() <= 1e-8 and abs(p[7] - p[5] / np.sqrt(p[4] * p[6])) <= 1e-15
    fit = LogNormalParetoNBDFitter()
    fit._K, fit._names = 2, ["z"]
    fit._adopt(theta)
    A = np.random.default_rng(2).standard_normal((7, 7))
    H = -(A @ A.T + 7.0 * np.eye(7))
    fit._set_uncertainty(H)
    names = ["purchase:intercept", "purchase:z", "dropout:intercept", "dropout:z", "Sigma_00", "Sigma_01", "Sigma_11", "rho"]
    assert list(fit.params_.index) == names == list(fit.summary_.index) and fit.summary_.shape == (8, 6)
    assert fit.covariance_.shape == (7, 7) and list(fit.covariance_.index)[-3:] == ["c0", "c1", "c2"]
    cov = np.linalg.inv(-H)
    assert np.allclose(fit.standard_errors_.to_numpy(), np.sqrt(np.diag(J @ cov @ J.T)), rtol=1e-12, atol=0)
    assert np.allclose(fit.summary_["estimate"].to_numpy(), p, rtol=0, atol=0)
    assert fit.as_level2_record().shape == (1, 1, 7) and np.array_equal(fit.as_level2_record()[0, 0, :4], theta[:4])

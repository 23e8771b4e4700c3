"""The marginal likelihood on the GPU (csrc/marginal.hip) against the float64
model tests/marginal_ref.py (4 rounding units; the model evaluated at the device's own centres) and
against the exact fixture at the accuracy target; bit-for-bit independence of the batch, the grid,
the sharding and the entry point.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from tests import marginal_ref as M
from tests.helpers import bits, cdnow, golden

pytestmark = pytest.mark.gpu

TARGET = 1e-6
OMEGA2 = 0.8


def c_marginal(level2, D, K, arrays, omega2=OMEGA2, nodes=0, debug=None, centre=False, sel=None):
    """clv_marginal_loglik (debug = (batch_customers, grid) or centre: clv_debug_marginal_loglik) on the
    customers ``sel`` (a slice; default all): (l_marg [R][n], centres [R][n][12] or None)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    sel = slice(None) if sel is None else sel
    cov, x, tx, T, ls = arrays
    cov = None if cov is None else np.ascontiguousarray(cov[:, sel])
    x, tx, T = (np.ascontiguousarray(v[sel]) for v in (x, tx, T))
    ls = None if ls is None else np.ascontiguousarray(ls[sel])
    level2 = np.ascontiguousarray(level2, dtype=np.float64)
    R, n = level2.shape[0], x.shape[0]
    out = np.full((R, n), -7.0)
    cen = np.full((R, n, 12), -7.0) if centre else None
    head = (0, dptr(level2), D, K, dptr(cov), R, n, x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(tx), dptr(T),
            dptr(ls), omega2 if ls is not None else 1.0, nodes)
    if debug is None and not centre:
        _lib.check(L.clv_marginal_loglik(*head, dptr(out)))
    else:
        b, g = debug or (0, 0)
        _lib.check(L.clv_debug_marginal_loglik(*head, b, g, dptr(out), dptr(cen)))
    return out, cen


@functools.lru_cache(maxsize=None)
def case(N, R, D, K, spend):
    """(level2, arrays, frame, covariate names) of a device case; the 600-customer frame and the
    25 records are shared by every shape that is a prefix of them."""
    df, names = M.case_customers(600, K, 17)
    recs = M.case_records(25, D, K, 100 * D + K)
    df = df.iloc[:N].reset_index(drop=True)
    return recs[:R], M.case_arrays(df, names, spend), df, names


def hold_to_model(level2, D, K, arrays, nodes, lm, cen, label):
    """The device's l_marg within 4 units of the model evaluated at the device's centres; the
    device's centres within 1e-6 of the model's own (Newton has converged on both sides)."""
    cov, x, tx, T, ls = arrays
    want, _ = M.marginal_loglik(level2, D, K, cov, x, tx, T, ls, OMEGA2, nodes=nodes or M.DEFAULT_ORDER, centres=cen)
    cen_m = M.model_centres(level2, D, K, cov, x, tx, T, ls, OMEGA2)
    dev = np.abs(lm - want) / M.unit_tol(want)
    move = np.abs(cen[..., [0, 1, 6, 7]] - cen_m[..., [0, 1, 6, 7]]).max()
    print(f"{label}: worst |device - model at the device's centre| = {dev.max():.3g} of 4 units; "
          f"centres differ from the model's own by {move:.3g}; Newton steps used <= {cen[..., [5, 11]].max():.0f}")
    assert np.isfinite(lm).all()
    assert dev.max() <= 1.0
    assert move <= 1e-6 and cen[..., [5, 11]].max() < M.NEWTON_STEPS


@pytest.mark.parametrize("R", [8, 25])
@pytest.mark.parametrize("N", [1, 255, 257, 600])
@pytest.mark.parametrize("D, K, spend", [(2, 1, False), (2, 3, False), (3, 1, True), (3, 3, True), (3, 3, False)])
def test_device_against_model(N, R, D, K, spend):
    level2, arrays, _, _ = case(N, R, D, K, spend)
    lm, cen = c_marginal(level2, D, K, arrays, centre=True)
    hold_to_model(level2, D, K, arrays, 0, lm, cen, f"N={N} R={R} D={D} K={K} spend={spend}")


@pytest.mark.parametrize("nodes", M.ORDERS)
def test_device_against_model_at_every_order(nodes):
    for D, K, spend in ((2, 3, False), (3, 1, True)):
        level2, arrays, _, _ = case(257, 8, D, K, spend)
        lm, cen = c_marginal(level2, D, K, arrays, nodes=nodes, centre=True)
        hold_to_model(level2, D, K, arrays, nodes, lm, cen, f"nodes={nodes} D={D} K={K}")
    if nodes == M.DEFAULT_ORDER:
        assert np.array_equal(bits(lm), bits(c_marginal(level2, D, K, arrays, nodes=0)[0]))


def test_device_against_the_exact_fixture():
    f = golden("marginal_exact.npz")
    fam = f["bi_k1_family"]
    bi = (None, f["bi_k1_x"], f["bi_k1_t_x"], f["bi_k1_T_cal"], None)
    lm, _ = c_marginal(f["bi_k1_level2"], 2, 1, bi)
    e_bi = np.abs(lm - f["bi_k1_exact"])
    tri = (f["tri_k3_cov"], f["tri_k3_x"], f["tri_k3_t_x"], f["tri_k3_T_cal"], f["tri_k3_log_s"])
    w2 = float(f["tri_k3_omega2"])
    e_sp = np.abs(c_marginal(f["tri_k3_level2"], 3, 3, tri, omega2=w2)[0] - f["tri_k3_exact"])
    e_tx = np.abs(c_marginal(f["tri_k3_level2"], 3, 3, tri[:4] + (None,))[0] - f["tri_k3_exact_tx"])
    print(f"default order against the exact integral: CDNOW-like {e_bi[fam == 0].max():.3g}, with spend {e_sp.max():.3g}, "
          f"trivariate without spend {e_tx.max():.3g}; wide {e_bi[fam == 1].max():.3g} (recorded, not held)")
    assert max(e_bi[fam == 0].max(), e_sp.max(), e_tx.max()) <= TARGET
    assert np.isfinite(e_bi).all()


def test_batches_grids_and_shards_give_the_same_bits():
    from mcmc_clv_model_amd import _lib
    level2, arrays, _, _ = case(600, 8, 3, 3, True)
    one, _ = c_marginal(level2, 3, 3, arrays)
    info = _lib.marginal_info()
    print("marginal_info", info)
    assert info["scratch_bytes"] == 0 and info["vgprs"] > 0 and info["kernel_ns"] > 0
    for debug in ((256, 0), (0, 1), (0, 2), (256, 2)):          # three batches; grids of 1 and 2 workgroups
        got, cen = c_marginal(level2, 3, 3, arrays, debug=debug, centre=True)
        assert np.array_equal(bits(got), bits(one)), debug
        assert not np.any(cen == -7.0)
    halves = [c_marginal(level2, 3, 3, arrays, sel=s)[0] for s in (slice(0, 300), slice(300, 600))]
    assert np.array_equal(bits(np.concatenate(halves, axis=1)), bits(one))


def test_nan_cells_leave_their_neighbours_untouched():
    level2, arrays, _, _ = case(257, 8, 2, 1, False)
    clean, _ = c_marginal(level2, 2, 1, arrays)
    rec = level2.copy()
    rec[3, 3] = 2.0 * np.sqrt(rec[3, 2] * rec[3, 4])          # |rho| = 2: Sigma_12 not positive definite
    cov, x, tx, T, ls = arrays
    tx = tx.copy()
    tx[200] = np.nan
    got, _ = c_marginal(rec, 2, 1, (cov, x, tx, T, ls))
    bad = np.zeros(got.shape, bool)
    bad[3, :] = True
    bad[:, 200] = True
    assert np.array_equal(np.isnan(got), bad)
    assert np.array_equal(bits(got[~bad]), bits(clean[~bad]))
    # the statistics: the customer's seven columns are NaN, the others are what they were without it
    from mcmc_clv_model_amd import analysis as A
    _, _, df, names = case(257, 8, 2, 1, False)
    ok = A.marginal_information_criteria(dict(level_2=[level2]), df, names)
    df2 = df.copy()
    df2.loc[200, "t_x"] = np.nan
    ic = A.marginal_information_criteria(dict(level_2=[level2]), df2, names)["pointwise"].to_numpy()
    assert np.isnan(ic[200]).all()
    assert np.array_equal(bits(np.delete(ic, 200, 0)), bits(np.delete(ok["pointwise"].to_numpy(), 200, 0)))


def test_fused_equals_two_steps():
    from mcmc_clv_model_amd import analysis as A
    for D, K, spend in ((2, 1, False), (3, 3, True)):
        level2, _, df, names = case(257, 25, D, K, spend)
        draws = dict(level_2=[level2[:13], level2[:13]])       # two chains, stacked in order
        kw = dict(spend=spend, omega2=OMEGA2) if spend else {}
        lm = A.marginal_log_likelihood(draws, df, names, **kw)
        assert lm.shape == (26, 257)
        two = A.psis_loo(lm, reff=0.7)
        fused = A.marginal_information_criteria(draws, df, names, reff=0.7, **kw)
        assert fused["kind"] == "marginal" and "kind" not in two
        for k in ("pointwise", "waic", "loo"):
            assert np.array_equal(bits(fused[k].to_numpy(dtype=np.float64)), bits(two[k].to_numpy(dtype=np.float64))), k
        assert list(A.compare_models({"a": fused, "b": fused}).index) == ["a", "b"]
        with pytest.raises(ValueError, match="conditional"):
            A.compare_models({"a": fused, "b": two})


RUN = dict(mcmc=40, burnin=20, thin=2, chains=2, seed=5)


@pytest.mark.parametrize("D", [2, 3])
def test_entry_points_give_the_same_bits(D):
    from mcmc_clv_model_amd import _lib, mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", n=300)
    covs = ["first_sales_scaled"]
    kw = dict(reff=0.8, nodes=16)
    if D == 3:
        kw.update(spend=True, omega2=0.9)
    with HipSampler(build_problem(df, covs, D=D), n_mh_steps=20, **RUN) as s:
        with pytest.raises(_lib.ClvError, match="-3"):          # CLV_ESTATE: the run has not stored its records
            s.marginal_information_criteria(**kw)
        s.run(60)
        dev = s.marginal_information_criteria(**kw)
        _, l2, _ = s.read_draws(level1=False)
    host = A.marginal_information_criteria(dict(level_2=list(l2)), df, covs, **kw)
    fit = mcmc_draw_parameters if D == 2 else mcmc_draw_parameters_rfm_m
    out = fit(df, covs, trace=0, marginal_information_criteria=kw, **RUN)
    for other in (dev, out["marginal_information_criteria"]):
        assert other["kind"] == "marginal"
        for k in ("pointwise", "waic", "loo"):
            assert np.array_equal(bits(other[k].to_numpy(dtype=np.float64)), bits(host[k].to_numpy(dtype=np.float64))), k
    assert host["loo"]["n_samples"].iloc[0] == 40 and np.isfinite(host["pointwise"].to_numpy()[:, :5]).all()
    assert "marginal_information_criteria" not in fit(df, covs, trace=0, **RUN)
    with pytest.raises(ValueError):
        fit(df, covs, trace=0, marginal_information_criteria=dict(nodes=7), **RUN)


def test_log_score_of_new_customers_against_the_model():
    from mcmc_clv_model_amd import analysis as A
    level2, arrays, df, names = case(257, 25, 2, 3, False)
    got = A.marginal_log_score(dict(level_2=[level2]), df, names)
    cov, x, tx, T, _ = arrays
    lm_dev, cen = c_marginal(level2, 2, 3, arrays, centre=True)
    lm, _ = M.marginal_loglik(level2, 2, 3, cov, x, tx, T, centres=cen)
    want = M.log_score(lm)
    score = got["pointwise"]["log_score"].to_numpy()
    # the log score averages the records' densities: its error is at most the largest over the records
    tol = M.unit_tol(lm).max(axis=0) + 4 * np.spacing(np.abs(want))
    print(f"log score: worst |device - model| / tolerance = {(np.abs(score - want) / tol).max():.3g}")
    assert np.all(np.abs(score - want) <= tol)
    assert np.array_equal(bits(score), bits(M.log_score(lm_dev)))
    tot = got["total"].iloc[0]
    assert tot["log_score"] == A.fixed_order_sum(score) and tot["n_records"] == 25 and tot["n_customers"] == 257
    dev = score - tot["log_score"] / 257
    assert tot["se"] == float(np.sqrt(257 * (A.fixed_order_sum(dev * dev) / 257)))

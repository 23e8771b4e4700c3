"""GPU: the Pareto/NBD likelihood kernels (csrc/pnbd.hip) and mle.ParetoNBDFitter against the exact
fixtures of tests/golden/pnbd_*.npz (mpmath quadrature of the integral; made by
tests/golden/make_pnbd_goldens.py).  Neither mpmath nor a host fit is needed here.

Bound for a device value against the exact one, relative to max(1, |value|): 8 x the fixture's
recorded error of the float64 numpy model (E_ref), floor 64 ulp.  The margin: the device log, lgamma
and log1p each differ from glibc's by a few ulp, and log L adds about eight such terms.

The block strides (more than PNBD_MAX_GRID = 2,048 blocks) and the lane stride of the final reduction
(more than 256 block partials) are reached at n = 524,545 and 65,537; measured: DESIGN.md section 4e."""
import math

import numpy as np
import pandas as pd
import pytest

from tests import pnbd_ref as R
from tests.helpers import bits, cdnow, golden

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
NEAR_OPT = (0.55, 10.58, 0.61, 11.67)


def bound(e_ref):
    return max(8.0 * float(e_ref), 64.0 * ULP)


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@pytest.fixture(scope="module")
def edge():
    e = golden("pnbd_edge.npz")
    return {k: e[k] for k in e.files}


@pytest.fixture(scope="module")
def abe():
    df = cdnow("abe")
    return df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy()


@pytest.mark.parametrize("k", range(6))
def test_edge_grid_against_the_quadrature(edge, k):
    from mcmc_clv_model_amd.mle import PnbdData
    p, nan = edge["params"][k], edge["model_nan"][k]
    with PnbdData(edge["x"], edge["t_x"], edge["T"]) as d:
        cust = d.customers(p, float(edge["t_star"]))
        sums, n_unc = d.eval(p)
    assert np.array_equal(np.isnan(cust[:, 0]), nan) and np.array_equal(np.isnan(cust).any(1), nan)
    ok = ~nan
    for col, key in enumerate(("logL", "p_alive", "ey")):
        err = rel(cust[ok, col], edge[key][k][ok]).max()
        print(f"set {k} {key}: measured {err:.3g}, bound {bound(edge['eref_' + key][k]):.3g}")
        assert err <= bound(edge["eref_" + key][k]), (k, key, err)
    assert n_unc == int(nan.sum()) and sums[5] == 12.0
    if nan.any():       # reported, not a number: nothing is truncated silently
        assert n_unc > 0 and np.isnan(sums[0])
    else:
        assert sums[0] == R.device_sum(cust[:, 0])
        err = (np.abs(sums[1:5] - edge["grad_sum"][k]) / np.maximum(1.0, edge["grad_abs"][k])).max()
        print(f"set {k} gradient sums: measured {err:.3g}, bound {bound(edge['eref_grad'][k]):.3g}")
        assert err <= bound(edge["eref_grad"][k]), (k, err)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2357])
def test_block_edges_fixed_order_sums(abe, n):
    from mcmc_clv_model_amd.mle import PnbdData
    x, tx, T = (a[:n] for a in abe)
    with PnbdData(x, tx, T) as d:
        cust = d.customers(NEAR_OPT, 39.0)
        s1, u1 = d.eval(NEAR_OPT)
        s2, u2 = d.eval(NEAR_OPT)
    assert u1 == 0 and u2 == 0 and np.isfinite(cust).all()
    assert np.array_equal(bits(s1), bits(s2))                                  # two calls: the same bits
    assert bits(s1[0]) == bits(R.device_sum(cust[:, 0])) and s1[5] == float(n)   # the fixed order, bit for bit
    m = R.model_customers(x, tx, T, NEAR_OPT)
    scale = np.maximum(1.0, np.abs(m["grad"]).sum(0))
    # device and model run the same algorithm; they differ by the few ulp between the device's and
    # glibc's log / log1p / exp / lgamma in each of a term's ~10 summands: far below 1e-12 of sum |terms|
    assert (np.abs(s1[1:5] - m["grad"].sum(0)) / scale).max() <= 1e-12
    # weights of 2 on a table = the table twice
    with PnbdData(x, tx, T, np.full(n, 2.0)) as d:
        sw, _ = d.eval(NEAR_OPT)
    with PnbdData(np.tile(x, 2), np.tile(tx, 2), np.tile(T, 2)) as d:
        sd, _ = d.eval(NEAR_OPT)
    assert sw[5] == 2.0 * n == sd[5]
    assert np.allclose(sw, sd, rtol=1e-13, atol=0)


@pytest.mark.parametrize("n", [65_537, 524_545])
def test_beyond_one_grid_and_one_reduction_pass(abe, n):
    """The abe table tiled to n = 65,537 (nb = 257 block partials: lane 0 of pnbd_final_kernel takes
    partials 0 and 256, the lane stride) and n = 524,545 (nb = 2,050 > PNBD_MAX_GRID = 2,048: the block
    stride b += gridDim.x of pnbd_eval_kernel, the lane stride of pnbd_customers_kernel).  A strided
    customer has the bits of the same row among the first 2,357; the sums are those of the fixed order
    (tests/pnbd_ref.device_sum, whose second level tests/test_pnbd_cpu.py holds to math.fsum)."""
    from mcmc_clv_model_amd.mle import PnbdData
    idx = np.arange(n) % len(abe[0])
    x, tx, T = (a[idx] for a in abe)
    nb = -(-n // 256)
    assert nb == {65_537: 257, 524_545: 2_050}[n]
    with PnbdData(x, tx, T) as d:
        cust = d.customers(NEAR_OPT, 39.0)
        s1, u1 = d.eval(NEAR_OPT)
        s2, u2 = d.eval(NEAR_OPT)
    assert cust.shape == (n, 3) and not np.isnan(cust).any()
    moved = (bits(cust) != bits(cust[:len(abe[0])][idx])).any(axis=1)
    print(f"n = {n}: {int(moved.sum())} customers differ from their row among the first {len(abe[0])}")
    assert not moved.any(), np.flatnonzero(moved)[:5]
    assert u1 == 0 and u2 == 0 and np.array_equal(bits(s1), bits(s2))
    assert bits(s1[0]) == bits(R.device_sum(cust[:, 0])) and s1[5] == float(n)
    g = R.model_customers(*abe, NEAR_OPT)["grad"][idx]
    want = np.array([math.fsum(g[:, j]) for j in range(4)])
    scale = np.maximum(1.0, [math.fsum(np.abs(g[:, j])) for j in range(4)])
    err = (np.abs(s1[1:5] - want) / scale).max()
    print(f"n = {n} gradient sums: measured {err:.3g} of sum |terms|, bound 1e-12")
    assert err <= 1e-12
    # weights of 0 on all but the last 300 customers = the table of those 300: a strided block reads its own w
    w = np.zeros(n)
    w[-300:] = 1.0
    with PnbdData(x, tx, T, w) as d:
        sw, uw = d.eval(NEAR_OPT)
    with PnbdData(x[-300:], tx[-300:], T[-300:]) as d:
        s300, _ = d.eval(NEAR_OPT)
    print(f"n = {n} weights: largest relative deviation from the 300-customer table "
          f"{np.max(np.abs(sw[:5] / s300[:5] - 1.0)):.3g}")
    assert sw[5] == 300.0 == s300[5] and uw == 0
    assert np.allclose(sw[:5], s300[:5], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["abe", "full"])
def test_fit_reaches_the_golden_optimum(edge, name):
    from mcmc_clv_model_amd import ParetoNBDFitter
    g = golden("pnbd_fit.npz")
    df = cdnow(name)
    f = ParetoNBDFitter(penalizer_coef=0.0)
    assert f.fit(frequency=df["x"], recency=df["t_x"], T=df["T_cal"]) is f
    print(name, f.params_.to_dict(), f.log_likelihood_, f.n_iter_, f.n_eval_, f.grad_norm_)
    assert f.converged_ is True and f.n_eval_ < 200 and f.grad_norm_ <= 1e-7 and f.n_unconverged_ == 0
    assert list(f.params_.index) == ["r", "alpha", "s", "beta"] and isinstance(f.params_, pd.Series)
    assert abs(f.log_likelihood_ - float(g[f"{name}_logL"])) <= 1e-6
    assert np.allclose(f.params_.to_numpy(), g[f"{name}_params"], rtol=1e-4, atol=0)
    # the fit methods against the float64 model at the fitted parameters
    x, tx, T = df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy()
    m = R.model_customers(x, tx, T, f.params_.to_numpy(), 39.0)
    ey = f.conditional_expected_number_of_purchases_up_to_time(39.0, df["x"], df["t_x"], df["T_cal"])
    pa = f.conditional_probability_alive(df["x"], df["t_x"], df["T_cal"])
    assert ey.shape == pa.shape == (len(df),)
    assert rel(ey, m["ey"]).max() <= bound(edge["eref_ey"].max())
    assert rel(pa, m["p_alive"]).max() <= bound(edge["eref_p_alive"].max())
    assert (pa > 0).all() and (pa <= 1).all() and (ey >= 0).all()


def test_weekly_tracking_curve():
    from mcmc_clv_model_amd import ParetoNBDFitter, pnbd_weekly_tracking
    rng = np.random.default_rng(11)
    birth = rng.integers(1, 91, 130)                     # births on the integers, some after week 78
    times = np.arange(1, 79)
    assert (birth > times[-1]).any() and (birth < 10).any()
    f = ParetoNBDFitter()
    f.params_ = pd.Series(NEAR_OPT, index=["r", "alpha", "s", "beta"])
    cum = pnbd_weekly_tracking(f, birth, times)
    want = np.array([f.expected_number_of_purchases_up_to_time(np.clip(t - birth, 0, None)).sum() for t in times])
    assert cum.shape == (78,) and cum[0] == 0.0
    assert np.allclose(cum, want, rtol=1e-13, atol=0)
    assert (np.diff(cum) >= 0).all() and cum[-1] > cum[1] > 0
    rel_t = np.clip(times[:, None] - birth[None, :], 0, None).astype(np.float64)
    part = R.model_expected_purchases(rel_t, NEAR_OPT)
    assert np.allclose(cum, [R.device_sum(row) for row in part], rtol=1e-14, atol=0)
    # more than one block of customers (700 = 3 blocks, the last one partly filled)
    birth3 = rng.integers(1, 60, 700)
    cum3 = pnbd_weekly_tracking(f, birth3, times)
    want3 = [f.expected_number_of_purchases_up_to_time(np.clip(t - birth3, 0, None)).sum() for t in times]
    assert np.allclose(cum3, want3, rtol=1e-13, atol=0) and (np.diff(cum3) >= 0).all()


def test_weekly_tracking_beyond_one_grid():
    """524,545 births (2,050 blocks > PNBD_MAX_GRID: the block stride of pnbd_track_kernel; 9 partials
    per lane of pnbd_final_kernel) and 3 times, against the fixed-order sum of the float64 model."""
    from mcmc_clv_model_amd import ParetoNBDFitter, pnbd_weekly_tracking
    n = 524_545
    birth = np.random.default_rng(12).integers(1, 91, n)
    times = np.array([10.0, 40.0, 78.0])
    f = ParetoNBDFitter()
    f.params_ = pd.Series(NEAR_OPT, index=["r", "alpha", "s", "beta"])
    cum = pnbd_weekly_tracking(f, birth, times)
    rel_t = np.clip(times[:, None] - birth[None, :], 0, None).astype(np.float64)
    want = np.array([R.device_sum(row) for row in R.model_expected_purchases(rel_t, NEAR_OPT)])
    print(f"tracking n = {n}: largest relative deviation from the model's fixed-order sum {np.max(np.abs(cum / want - 1.0)):.3g}")
    assert cum.shape == (3,) and (np.diff(cum) > 0).all() and cum[0] > 0
    assert np.allclose(cum, want, rtol=1e-14, atol=0)


def test_einval_paths_leave_the_handle_usable(abe):
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, PnbdData, pnbd_weekly_tracking
    x, tx, T = (a[:300] for a in abe)
    with PnbdData(x, tx, T) as d:
        s0, _ = d.eval(NEAR_OPT)
        for bad in ((0.0, 1, 1, 1), (1, -1.0, 1, 1), (1, 1, np.inf, 1), (1, 1, 1, np.nan)):
            with pytest.raises(ValueError, match="positive and finite"):
                d.eval(bad)
            with pytest.raises(ValueError, match="positive and finite"):
                d.customers(bad, 39.0)
        for t_star in (-1.0, np.inf, np.nan):
            with pytest.raises(ValueError, match="t_star"):
                d.customers(NEAR_OPT, t_star)
        s1, _ = d.eval(NEAR_OPT)
        assert np.array_equal(bits(s0), bits(s1))
    for kw, msg in ((dict(x=np.zeros(0, np.int32), tx=np.zeros(0), T=np.zeros(0)), "n must be"),
                    (dict(x=-x), "negative x"), (dict(tx=T + 1.0), "t_x <= T"), (dict(T=np.full(300, np.inf)), "non-finite"),
                    (dict(w=np.full(300, -1.0)), "weight"), (dict(w=np.full(300, np.nan)), "weight")):
        a = dict(x=x, tx=tx, T=T, w=None)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            PnbdData(a["x"], a["tx"], a["T"], a["w"])
    with pytest.raises(ValueError, match="integer"):
        PnbdData(x + 0.5, tx, T)
    f = ParetoNBDFitter()
    f.params_ = pd.Series(NEAR_OPT, index=["r", "alpha", "s", "beta"])
    for b, t in (([1.0, np.nan], [1.0, 2.0]), ([1.0, 2.0], [np.inf]), ([], [1.0]), ([1.0], [])):
        with pytest.raises(ValueError):
            pnbd_weekly_tracking(f, b, t)
    with pytest.raises(ValueError, match="initial_params"):
        f.fit(x, tx, T, initial_params=(1, 1, 0, 1))


def test_penalizer_and_weights_through_the_fitter(abe):
    """penalizer_coef adds penalizer_coef * sum(params^2) to the mean objective: the penalised optimum
    has smaller parameters and its gradient condition holds for the penalised objective."""
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, PnbdData
    x, tx, T = (a[:600] for a in abe)
    f0 = ParetoNBDFitter().fit(x, tx, T)
    f1 = ParetoNBDFitter(penalizer_coef=0.001).fit(x, tx, T)
    assert f0.converged_ and f1.converged_
    p = f1.params_.to_numpy()
    with PnbdData(x, tx, T) as d:
        s, _ = d.eval(p)
    assert np.abs(-s[1:5] / s[5] + 2.0 * 0.001 * p ** 2).max() <= 1e-7
    assert (p ** 2).sum() < (f0.params_.to_numpy() ** 2).sum()
    assert f1.log_likelihood_ < f0.log_likelihood_

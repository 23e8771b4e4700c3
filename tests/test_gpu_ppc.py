"""Posterior predictive checks on the GPU (csrc/ppc.hip) against the float64 model tests/ppc_ref.py,
value by value: on clear lanes (decision margin > RTOL) x_rep is exact and t_x_rep within RTOL, the
set-aside share stays within BORDERLINE_CAP, and every aggregate equals the same aggregate recomputed
from the device's own replicates — integers exactly, the floating-point sums bit for bit.  Every figure
is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from tests import ppc_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu


def c_ppc(case, seed, k_hist=16, replicates=True, debug=None, offset=0, sel=None):
    """clv_ppc (debug: (batch_customers, grid) through clv_debug_ppc) on a case of ppc_ref, optionally on
    the customers ``sel`` (a slice) alone: dict(customers, draws_int, sum_tx, x_rep, t_x_rep)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    sel = slice(None) if sel is None else sel
    x = np.ascontiguousarray(case["x"][sel], dtype=np.int32)
    tx, T = np.ascontiguousarray(case["t_x"][sel]), np.ascontiguousarray(case["T_cal"][sel])
    n = x.shape[0]
    l1 = l2 = cov = None
    w, D, K = 0, 0, 0
    if case["level"] == 0:
        l1 = np.ascontiguousarray(case["level1"][:, sel])
        nd, w = l1.shape[0], l1.shape[2]
    else:
        l2 = np.ascontiguousarray(case["level2"])
        nd, D, K = l2.shape[0], case["D"], case["K"]
        cov = None if case["cov"] is None else np.ascontiguousarray(case["cov"][:, sel])
    i64 = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    cu = np.full((n, 7), -7.0)
    di = np.full((nd, k_hist + 5), -7, np.int64)
    df = np.full((nd, 1), -7.0)
    xr = np.full((nd, n), -7, np.int64) if replicates else None
    tr = np.full((nd, n), -7.0) if replicates else None
    head = (0, case["level"], dptr(l1), w, dptr(l2), D, K, dptr(cov), nd, n,
            x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(tx), dptr(T), k_hist, seed, offset, dptr(cu), i64(di),
            dptr(df), i64(xr), dptr(tr))
    if debug is None:
        _lib.check(L.clv_ppc(*head))
    else:
        _lib.check(L.clv_debug_ppc(*head, debug[0], debug[1]))
    return dict(customers=cu, draws_int=di, sum_tx=df[:, 0], x_rep=xr, t_x_rep=tr)


@functools.lru_cache(maxsize=None)
def cases():
    return R.gpu_cases()


@functools.lru_cache(maxsize=None)
def model(name, seed):
    return R.model(cases()[name], seed)


def same_bits(a, b, what=""):
    for k in ("customers", "draws_int", "sum_tx", "x_rep", "t_x_rep"):
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k}"


def check_against_model(case, m, got, k_hist, label):
    """The checks of the module docstring; returns the clear mask."""
    clear = m["margin"] > R.RTOL
    share = 1.0 - clear.mean()
    x_bad = int(np.count_nonzero((got["x_rep"] != m["x_rep"]) & clear))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got["t_x_rep"] - m["t_x_rep"]) / np.abs(m["t_x_rep"])
    rel = np.where(m["t_x_rep"] == 0.0, np.where(got["t_x_rep"] == 0.0, 0.0, np.inf), rel)
    worst = float(rel[clear].max()) if clear.any() else 0.0
    print(label, "set aside", share, "x_rep mismatches on clear lanes", x_bad, "worst t_x_rep rel err", worst)
    assert share <= R.BORDERLINE_CAP
    assert x_bad == 0
    assert worst <= R.RTOL
    T = np.broadcast_to(case["T_cal"], got["t_x_rep"].shape)
    assert (got["t_x_rep"] <= T).all() and (got["t_x_rep"] >= 0.0).all()
    # alive, through N_ALIVE and p_alive_rep: exact wherever every contributing lane is clear
    unclear_d, unclear_c = (~clear).sum(axis=1), (~clear).sum(axis=0)
    n_alive = got["draws_int"][:, k_hist + 1 + R.DRAW_INTS.index("n_alive")]
    assert (np.abs(n_alive - m["alive"].sum(axis=1)) <= unclear_d).all()
    S = m["alive"].shape[0]
    pa = got["customers"][:, R.STATS.index("p_alive_rep")]
    assert (np.abs(pa * S - m["alive"].sum(axis=0)) <= unclear_c + 1e-9).all()
    # every other aggregate from the device's own replicates
    ag = R.aggregates(got["x_rep"], got["t_x_rep"], m["alive"], case["x"], case["t_x"], k_hist)
    keep = [j for j, s in enumerate(R.STATS) if s != "p_alive_rep"]
    assert np.array_equal(bits(got["customers"][:, keep]), bits(ag["customers"][:, keep])), "customer rows"
    assert np.array_equal(got["draws_int"][:, :k_hist + 4], ag["draws_int"][:, :k_hist + 4]), "per-draw integers"
    assert np.array_equal(bits(got["sum_tx"]), bits(ag["sum_tx"])), "SUM_TX"
    assert (got["draws_int"][:, :k_hist + 1].sum(axis=1) == len(case["x"])).all()
    return clear


# ---- 1. value by value, customer level ------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS, ids=["seed_lo", "seed_hi"])
@pytest.mark.parametrize("width", [4, 5])
def test_customer_level_value_by_value(width, seed):
    name = f"customer_w{width}"
    case, m = cases()[name], model(name, seed)
    got = c_ppc(case, seed, k_hist=16)
    check_against_model(case, m, got, 16, name)
    # both Poisson branches and both sides of tau vs T are in the case
    mean = m["lam"] * m["L"]
    assert ((mean > 0) & (mean < 10)).any() and (mean >= 10).any() and m["alive"].any() and (~m["alive"]).any()
    assert (case["x"] == 0).mean() > 0.3


# ---- 2. value by value, population level ----------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS, ids=["seed_lo", "seed_hi"])
@pytest.mark.parametrize("D, K", R.POPULATION_DK)
def test_population_level_value_by_value(D, K, seed):
    name = f"population_{D}{K}"
    case, m = cases()[name], model(name, seed)
    got = c_ppc(case, seed, k_hist=16)
    check_against_model(case, m, got, 16, name)
    if D == 3:   # only beta's first two columns and Sigma's leading 2 x 2 block are read
        other = dict(case)
        l2 = case["level2"].copy()
        l2[:, 2 * K:3 * K] += 1.5                       # the eta column of beta
        l2[:, 3 * K + 2] *= 0.5                         # Sigma02
        l2[:, 3 * K + 4] *= -2.0                        # Sigma12
        l2[:, 3 * K + 5] *= 3.0                         # Sigma22
        other["level2"] = l2
        same_bits(got, c_ppc(other, seed, k_hist=16), "trivariate record")


# ---- 3. geometry ----------------------------------------------------------------------------------
def test_geometry_leaves_every_bit_alone(monkeypatch):
    case, seed = cases()["customer_w4"], R.SEEDS[1]
    base = c_ppc(case, seed, k_hist=16)
    same_bits(base, c_ppc(case, seed, k_hist=16, debug=(256, 1)), "batch 256, grid 1")
    same_bits(base, c_ppc(case, seed, k_hist=16, debug=(1, 2)), "batch 1, grid 2")
    same_bits(base, c_ppc(case, seed, k_hist=16, replicates=False), "NULL replicate outputs")
    blk = c_ppc(case, seed, k_hist=16, offset=256, sel=slice(256, 512))
    assert np.array_equal(bits(blk["customers"]), bits(base["customers"][256:512]))
    assert np.array_equal(blk["x_rep"], base["x_rep"][:, 256:512])
    assert np.array_equal(bits(blk["t_x_rep"]), bits(base["t_x_rep"][:, 256:512]))
    for item_draws in ("64", "1000000"):                # work items of two chunks / of every draw
        monkeypatch.setenv("CLV_PPC_ITEM_DRAWS", item_draws)
        same_bits(base, c_ppc(case, seed, k_hist=16), f"CLV_PPC_ITEM_DRAWS={item_draws}")
        same_bits(base, c_ppc(case, seed, k_hist=16, debug=(256, 1)), f"CLV_PPC_ITEM_DRAWS={item_draws}, grid 1")
    monkeypatch.delenv("CLV_PPC_ITEM_DRAWS")
    long = cases()["long"]
    lb = c_ppc(long, seed, k_hist=8)
    monkeypatch.setenv("CLV_PPC_ITEM_DRAWS", "4096")
    same_bits(lb, c_ppc(long, seed, k_hist=8), "65,537 draws in work items of 4,096")
    monkeypatch.delenv("CLV_PPC_ITEM_DRAWS")
    pop = cases()["population_23"]
    pb = c_ppc(pop, seed, k_hist=16)
    same_bits(pb, c_ppc(pop, seed, k_hist=16, debug=(1, 2)), "population: batch 1, grid 2")
    pblk = c_ppc(pop, seed, k_hist=16, offset=256, sel=slice(256, 300))
    assert np.array_equal(bits(pblk["customers"]), bits(pb["customers"][256:300]))
    assert np.array_equal(pblk["x_rep"], pb["x_rep"][:, 256:300])


# ---- 4. histogram edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("k_hist", [1, 4096])
def test_histogram_edges(k_hist):
    case, seed = cases()["customer_w4"], R.SEEDS[0]
    got = c_ppc(case, seed, k_hist=k_hist)
    hist = got["draws_int"][:, :k_hist + 1]
    assert (hist.sum(axis=1) == 513).all()
    assert np.array_equal(hist[:, k_hist], (got["x_rep"] >= k_hist).sum(axis=1))
    assert (got["x_rep"] >= 4096).any()                 # the 1e5 means reach past the largest k_hist
    ag = R.aggregates(got["x_rep"], got["t_x_rep"], np.zeros_like(got["x_rep"], bool), case["x"], case["t_x"], k_hist)
    assert np.array_equal(got["draws_int"][:, :k_hist + 4], ag["draws_int"][:, :k_hist + 4])
    assert np.array_equal(got["x_rep"], c_ppc(case, seed, k_hist=16)["x_rep"])


# ---- 5. shapes ------------------------------------------------------------------------------------
def test_one_customer_one_draw():
    case = R.long_case(1)
    got = c_ppc(case, R.SEEDS[0], k_hist=8)
    check_against_model(case, R.model(case, R.SEEDS[0]), got, 8, "n = 1, 1 draw")


def test_one_customer_65537_draws():
    case, m = cases()["long"], model("long", R.SEEDS[1])
    got = c_ppc(case, R.SEEDS[1], k_hist=8)
    check_against_model(case, m, got, 8, "n = 1, 65,537 draws")


# ---- 6. edge draws --------------------------------------------------------------------------------
def test_edge_draws_stay_finite():
    case, m = cases()["edge"], model("edge", R.SEEDS[0])
    got = c_ppc(case, R.SEEDS[0], k_hist=8)
    check_against_model(case, m, got, 8, "edge draws")
    i = np.arange(64)
    assert np.isfinite(got["customers"]).all() and np.isfinite(got["sum_tx"]).all() and np.isfinite(got["t_x_rep"]).all()
    assert (got["customers"][i % 3 == 0, R.STATS.index("p_alive_rep")] == 1.0).all()      # mu = 1e-300
    assert (got["x_rep"][:, i % 3 == 1] == 0).all() and (got["customers"][i % 3 == 1, 6] == 0.0).all()   # mu = 1e300
    assert (got["x_rep"][:, i % 3 == 2] == 0).all() and (got["t_x_rep"][:, i % 3 == 2] == 0.0).all()     # NaN lambda


# ---- 7. entry points ------------------------------------------------------------------------------
RUN = dict(mcmc=40, burnin=20, thin=2, chains=2, seed=5)


def frames_equal(a, b):
    for k in ("customers", "frequency", "draws", "statistics"):
        assert list(a[k].columns) == list(b[k].columns) and list(a[k].index) == list(b[k].index), k
        assert np.array_equal(bits(a[k].to_numpy(dtype=np.float64)), bits(b[k].to_numpy(dtype=np.float64))), k
    assert np.array_equal(a["x_rep"], b["x_rep"]) and np.array_equal(bits(a["t_x_rep"]), bits(b["t_x_rep"]))
    assert (a["level"], a["n_samples"], a["seed"]) == (b["level"], b["n_samples"], b["seed"])


@pytest.mark.parametrize("level", ["customer", "population"])
def test_entry_points_give_the_same_bits(level):
    from mcmc_clv_model_amd import _lib, mcmc_draw_parameters
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", n=300)
    covs = ["first_sales_scaled"]
    kw = dict(level=level, k_hist=12, seed=11, replicates=True)
    with HipSampler(build_problem(df, covs, D=2), n_mh_steps=20, **RUN) as s:
        with pytest.raises(_lib.ClvError, match="-3"):          # CLV_ESTATE: the run has not stored its draws
            s.posterior_predictive_check(**kw)
        s.run(60)
        dev = s.posterior_predictive_check(**kw)
        info = _lib.ppc_info()
        l1, l2, _ = s.read_draws()
    print("ppc_info", info)
    assert info["scratch_bytes"] == 0 and info["vgprs"] > 0 and info["kernel_ns"] > 0
    host = A.posterior_predictive_check(dict(level_1=list(l1), level_2=list(l2)), df, covs, **kw)
    frames_equal(dev, host)
    out = mcmc_draw_parameters(df, covs, trace=0, ppc=kw, **RUN)
    frames_equal(out["ppc"], host)
    assert host["n_samples"] == 40 and host["x_rep"].shape == (40, 300) and len(host["frequency"]) == 13
    assert np.isfinite(host["customers"].to_numpy()).all() and int(A.ppc_pit(host).sum()) == 300
    assert "ppc" not in mcmc_draw_parameters(df, covs, trace=0, **RUN)
    with pytest.raises(ValueError):
        mcmc_draw_parameters(df, covs, trace=0, ppc=dict(level="nobody"), **RUN)

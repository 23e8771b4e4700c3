"""Many fits in one launch (csrc/batch.hip, batch_fit_kernel): every fit of a batch equals its
single call bit for bit — np.array_equal on the raw arrays, no tolerance — at the tile edges, for
every compiled (D, K) instance, with more workgroups than the card holds at once, on both sides of
PRE_STEPS, in either order, through the routing and the seed rule, and in the K-fold glue."""
import numpy as np
import pytest

from mcmc_clv_model_amd import (kfold_cross_validation, marginal_log_score, mcmc_draw_parameters,
                                mcmc_draw_parameters_many, mcmc_draw_parameters_rfm_m,
                                mcmc_draw_parameters_rfm_m_many)
from mcmc_clv_model_amd import batch as B
from tests.helpers import cdnow, with_covariates

pytestmark = pytest.mark.gpu

SINGLE = {2: mcmc_draw_parameters, 3: mcmc_draw_parameters_rfm_m}
MANY = {2: mcmc_draw_parameters_many, 3: mcmc_draw_parameters_rfm_m_many}


def assert_same_fit(got, want, what=""):
    """Every array of a fit's output dict, its types and its summary means: equal bits."""
    assert set(got) == set(want), what
    if want["level_1"] is None:
        assert got["level_1"] is None, what
    else:
        assert len(got["level_1"]) == len(want["level_1"]), what
        for c, (a, b) in enumerate(zip(got["level_1"], want["level_1"])):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, c)
            assert np.array_equal(a, b), (what, "level_1", c, int(np.count_nonzero(a != b)))
    assert len(got["level_2"]) == len(want["level_2"]), what
    for c, (a, b) in enumerate(zip(got["level_2"], want["level_2"])):
        assert a.shape == b.shape and np.array_equal(a, b), (what, "level_2", c)
    assert type(got["log_likelihood"]) is type(want["log_likelihood"]), what
    assert np.array_equal(got["log_likelihood"], want["log_likelihood"]), (what, "log_likelihood")
    if "summary" in want:
        assert set(got["summary"]) == set(want["summary"]), what
        assert got["summary"]["n_draws"] == want["summary"]["n_draws"], what
        for k, v in want["summary"].items():
            if k != "n_draws":
                assert np.array_equal(got["summary"][k], v), (what, "summary", k)


def single(D, cbs, covs, seed, **kw):
    return SINGLE[D](cbs, covs, seed=seed, trace=0, **kw)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("sink", ["full", "summary"])
def test_tile_edges(sink, D):
    full = with_covariates(cdnow("full"), 1)
    # the smallest fit: one customer; trivariate two (omega2 is the variance of log_s: NaN of one row)
    ns = (1 if D == 2 else 2, 255, 256, 257, 513, 1000)
    fits = [full.iloc[2:2 + n].reset_index(drop=True) for n in ns]  # row 2: x > 0 (a fit of one x = 0 row has lam_init 0)
    seeds = [100 + 7 * j for j in range(len(ns))]
    kw = dict(mcmc=7, burnin=3, thin=3, chains=2, n_mh_steps=20, draw_sink=sink)
    out, info = MANY[D](fits, ["c1"], seeds=seeds, return_info=True, **kw)
    assert list(info["path"]) == ["batch"] * len(ns) and list(info["blocks"]) == [1, 1, 1, 2, 3, 4]
    assert info.attrs["kernel_ms"] > 0.0
    for j, n in enumerate(ns):
        assert_same_fit(out[j], single(D, fits[j], ["c1"], seeds[j], **kw), f"N = {n}")


@pytest.mark.parametrize("D,K", [(D, K) for D in (2, 3) for K in range(1, 10)])
def test_every_instance(D, K):
    covs = [f"c{k}" for k in range(1, K)]
    fits = [with_covariates(cdnow("abe", n), K - 1) for n in (300, 257)]
    seeds = [1000 + 10 * D + K, 5]
    kw = dict(mcmc=3, burnin=2, thin=1, chains=2, n_mh_steps=6)
    out = MANY[D](fits, covs, seeds=seeds, **kw)
    for j in range(2):
        assert_same_fit(out[j], single(D, fits[j], covs, seeds[j], **kw), f"D = {D}, K = {K}, fit {j}")


def test_more_workgroups_than_the_card_holds():
    full = cdnow("full")
    fits = [full.iloc[7 * j:7 * j + 64].reset_index(drop=True) for j in range(300)]
    kw = dict(mcmc=4, burnin=2, thin=2, chains=4, n_mh_steps=20)
    out = mcmc_draw_parameters_many(fits, seed=11, **kw)
    again = mcmc_draw_parameters_many(fits, seed=11, **kw)
    for j in range(300):
        assert_same_fit(again[j], out[j], f"second call, fit {j}")
    for j in (0, 1, 149, 298, 299):
        assert_same_fit(out[j], single(2, fits[j], None, 11 + 4 * j, **kw), f"fit {j}")


@pytest.mark.parametrize("steps", [24, 4])
def test_mh_steps_either_side_of_the_drawn_ahead_pool(steps):
    cbs = cdnow("abe", 300)
    kw = dict(mcmc=4, burnin=2, thin=1, chains=2, n_mh_steps=steps)
    out = mcmc_draw_parameters_many([cbs], seeds=[3], **kw)
    assert_same_fit(out[0], single(2, cbs, None, 3, **kw), f"S = {steps}")


def test_order_of_the_list_is_the_order_of_the_output():
    full = cdnow("full")
    fits = [full.iloc[a:b].reset_index(drop=True) for a, b in ((0, 300), (300, 900), (900, 1000), (1000, 1257))]
    seeds = [5, 6, 7, 8]
    kw = dict(mcmc=4, burnin=2, thin=2, chains=2)
    fwd = mcmc_draw_parameters_many(fits, seeds=seeds, **kw)
    rev = mcmc_draw_parameters_many(fits[::-1], seeds=seeds[::-1], **kw)
    for j in range(4):
        assert_same_fit(rev[3 - j], fwd[j], f"fit {j}")


def test_routing_is_invisible_in_the_results():
    full = cdnow("full")
    fits = [full.iloc[:300].reset_index(drop=True), full.iloc[300:1300].reset_index(drop=True)]
    kw = dict(mcmc=4, burnin=2, thin=2, chains=2, seeds=[21, 22])
    out2, info2 = mcmc_draw_parameters_many(fits, max_blocks=2, return_info=True, **kw)
    out8, info8 = mcmc_draw_parameters_many(fits, max_blocks=8, return_info=True, **kw)
    out0, info0 = mcmc_draw_parameters_many(fits, max_blocks=0, return_info=True, **kw)
    assert list(info2["path"]) == ["batch", "solo"]
    assert list(info8["path"]) == ["batch", "batch"] and list(info0["path"]) == ["solo", "solo"]
    for j in range(2):
        assert_same_fit(out2[j], out8[j], f"max_blocks 2 / 8, fit {j}")
        assert_same_fit(out2[j], out0[j], f"max_blocks 2 / 0, fit {j}")


def test_seed_rule():
    full = cdnow("full")
    fits = [full.iloc[100 * j:100 * j + 90].reset_index(drop=True) for j in range(3)]
    kw = dict(mcmc=3, burnin=2, thin=1, chains=3)
    out = mcmc_draw_parameters_many(fits, seed=7, **kw)
    for j in range(3):
        assert_same_fit(out[j], single(2, fits[j], None, 7 + j * 3, **kw), f"fit {j}")


def test_kfold_equals_its_pieces_assembled_by_hand():
    cbs = cdnow("full").iloc[:600].reset_index(drop=True)
    kw = dict(mcmc=4, burnin=4, thin=1, chains=2)
    res = kfold_cross_validation(cbs, k=3, fold_seed=5, nodes=8, seed=9, **kw)
    fold = res["pointwise"]["fold"].to_numpy()
    assert sorted(np.bincount(fold, minlength=3)) == [200, 200, 200] and len(fold) == 600
    assert np.array_equal(fold, B.fold_assignment(600, 3, 5))
    want = np.full(600, np.nan)
    for f in range(3):
        fit = mcmc_draw_parameters(cbs[fold != f].reset_index(drop=True), seed=9 + 2 * f, trace=0, **kw)
        s = marginal_log_score(fit, cbs[fold == f].reset_index(drop=True), nodes=8)
        want[fold == f] = s["pointwise"]["log_score"].to_numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(res["pointwise"]["elpd_kfold"].to_numpy(), want)
    assert np.isfinite(res["estimates"]["elpd_kfold"][0]) and res["estimates"]["se"][0] > 0.0
    assert list(res["folds"]["n"]) == [200, 200, 200]


def test_batch_info():
    n_cu = None
    for D in (2, 3):
        for K in range(1, 10):
            info = B.batch_info(D, K)
            print(D, K, info)
            n_cu = info["n_cu"]
            assert info["vgprs"] > 0 and info["blocks_per_cu"] >= 1
            assert info["slots"] == info["n_cu"] * info["blocks_per_cu"] and info["slots"] >= n_cu > 0
            if D == 2 or K <= 5:
                assert info["scratch_bytes"] == 0, (D, K)

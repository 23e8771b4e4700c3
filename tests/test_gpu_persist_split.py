"""The split layout of the persistent sweep (persist_kernel_split: six customer and two helper
wavefronts per workgroup, a chain's wave rows dealt six at a time) against the block layout and the
launch-per-sweep kernel: the same results to the bit — carried state, level-1 / level-2 / log-likelihood
draws, the summary sink's sums — at sizes where a split block's second half is empty, where both halves
hold customers, and where the last workgroup has vacant customer wavefronts; K = 1, 2, 5; S = 20, 7
(partial last chunk), 1; thin 2 across the burn-in boundary; launches of 1, 1, 1, 5, 2 and 3 sweeps
(the deferred level-2 draw and the prologue's variates on every launch).  A few dozen sweeps in all."""
import numpy as np
import pytest

from tests.helpers import bits, cdnow_tiled, with_covariates

pytestmark = pytest.mark.gpu

RUNS = (1, 1, 1, 5, 2, 3)  # 13 sweeps: burn-in 6 ends inside the run of 5
KW = dict(mcmc=8, burnin=6, thin=2, seed=77)

# (customers, chains, chain_first, K, MH steps, sink)
CASES = [
    (257, 2, 0, 2, 20, "full"),      # 2 blocks: block 1 split, its second half (rows 2, 3) all inactive
    (640, 2, 0, 1, 7, "full"),       # block 1 split with live lanes in both halves
    (640, 1, 0, 2, 20, "summary"),
    (1537, 2, 0, 5, 20, "summary"),  # 7 blocks (1 and 4 split), a one-customer last block, and a last
    (1537, 2, 0, 1, 1, "full"),      # workgroup with vacant customer wavefronts
    (1537, 4, 3, 2, 7, "full"),
]


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def _problem(n, K):
    from mcmc_clv_model_amd.sampler import build_problem
    df = with_covariates(cdnow_tiled(n), K - 1) if K > 1 else cdnow_tiled(n)
    return build_problem(df, [f"c{k}" for k in range(1, K)], 2)


def _run(monkeypatch, p, mode, chains, chain_first, S, sink):
    """One handle under `mode` (the environment is read at create), driven through RUNS."""
    from mcmc_clv_model_amd.sampler import HipSampler
    monkeypatch.delenv("CLV_PERSISTENT", raising=False)
    monkeypatch.delenv("CLV_PERSIST_LAYOUT", raising=False)
    if mode == "fused":
        monkeypatch.setenv("CLV_PERSISTENT", "0")
    else:
        monkeypatch.setenv("CLV_PERSIST_LAYOUT", mode)
    nb = -(-len(p.x) // 256)
    with HipSampler(p, chains=chains, chain_first=chain_first, n_mh_steps=S, draw_sink=sink, **KW) as s:
        info = s.launch_info()
        assert info["persistent"] == (mode != "fused")
        assert info["layout"] == (None if mode == "fused" else mode)
        assert info["workgroups"] == (nb + (mode != "fused")) * chains  # logical, in either layout
        if mode == "split":
            assert info["physical_workgroups"] == (-(-2 * nb // 3) + 1) * chains
        elif mode == "block":
            assert info["physical_workgroups"] == info["workgroups"]
        for k in RUNS:
            s.run(k)
        out = dict(zip(("lam", "mu", "beta", "sigma"), s.get_state()))
        l1, l2, ll = s.read_draws()
        out.update(level2=l2, loglik=ll)
        if sink == "full":
            out["level1"] = l1
        else:
            sums, k = s.read_summary()
            out.update(sums=sums, n_summed=np.array([k], np.float64))
    return out


@pytest.mark.parametrize("n,chains,chain_first,K,S,sink", CASES)
def test_split_block_and_fused_bitwise_equal(L, monkeypatch, n, chains, chain_first, K, S, sink):
    p = _problem(n, K)
    res = {m: _run(monkeypatch, p, m, chains, chain_first, S, sink) for m in ("split", "block", "fused")}
    for key, ref in res["fused"].items():
        assert np.isfinite(ref).all() or key == "level1", key
        for m in ("split", "block"):
            got = res[m][key]
            same = np.array_equal(bits(got), bits(ref))
            assert same, f"{m} vs launch-per-sweep: {key} differs in {int((bits(got) != bits(ref)).sum())} of {ref.size}"
    assert res["fused"]["level2"].shape[1] == 4 and res["fused"]["level2"].any()  # draws were stored


def test_more_steps_than_the_pool_declines_split(L, monkeypatch):
    """S = 21 > PRE_STEPS: the variates of a sweep do not fit the pool, so a forced split layout is
    declined (block layout), and the run still matches the launch-per-sweep kernel."""
    p = _problem(640, 2)
    a = _run(monkeypatch, p, "block", 1, 0, 21, "full")
    from mcmc_clv_model_amd.sampler import HipSampler
    monkeypatch.setenv("CLV_PERSIST_LAYOUT", "split")
    with HipSampler(p, chains=1, n_mh_steps=21, draw_sink="full", **KW) as s:
        assert s.launch_info()["layout"] == "block" and s.launch_info()["physical_workgroups"] == 4
        for k in RUNS:
            s.run(k)
        lam = s.get_state()[0]
    assert np.array_equal(bits(lam), bits(a["lam"]))


def test_layout_env_rejected(L, monkeypatch):
    from mcmc_clv_model_amd.sampler import HipSampler
    monkeypatch.setenv("CLV_PERSIST_LAYOUT", "both")
    with pytest.raises(ValueError, match="CLV_PERSIST_LAYOUT"):
        HipSampler(_problem(257, 1), chains=1, **KW)

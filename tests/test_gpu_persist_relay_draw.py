"""The relay instance of the split layout with its relay wavefronts drawing ahead in their idle gaps
(split_draw_plan: before the row's flag the first chunks of the rows on the owner's SIMD, staged in
LDS and copied into the pool by their readers; after the row's reduction their own chunks, straight
into the pool; whatever a gap left is drawn in the window by the chunk's reader) against the
launch-per-sweep kernel (CLV_PERSISTENT=0): the same results to the bit — carried state, level-1 /
level-2 / log-likelihood draws, the summary sink's sums.  Who draws a chunk and when must not show.

Launch patterns that exercise the edges of drawing ahead: (1, 1, 2, 1, 5, 3), where one-sweep launches
(no gap code runs; the prologue draws everything) follow multi-sweep ones and the reverse, and one
launch of 12 sweeps, where the staging buffer and the per-row masks are reused eleven times.  Burn-in
(6) ends inside a launch, thin 2.  Sizes, the smallest where it can go wrong:

  n = 257   row 4 holds one live lane and row 5 none: gap 1 draws for a nearly vacant and a vacant row
  n = 384   one workgroup, every row full
  n = 385   a second workgroup whose row 0 has one live lane and whose relay rows are vacant
  n = 769   three workgroups, the second with live relayed rows
  n = 1537  several workgroups (4 chains from chain 3, K = 5, summary sink)

S = R + 1 (a relay range of one step), 13 (a partial last chunk), 16 (whole chunks), 20 (all five);
K = 1, 2, 5; both sinks.  R is read from launch_info() of a forced handle."""
import ctypes

import numpy as np
import pytest

from tests.helpers import bits, cdnow_tiled, with_covariates

pytestmark = pytest.mark.gpu

MIXED = (1, 1, 2, 1, 5, 3)  # 13 sweeps: burn-in 6 ends inside the run of 5
ONE = (12,)                 # burn-in ends inside the launch
KW = dict(mcmc=8, burnin=6, thin=2, seed=91)

# (customers, chains, chain_first, K, MH steps, sink, launches)
CASES = [
    (257, 2, 0, 2, "20", "full", MIXED),
    (257, 1, 0, 1, "R+1", "summary", ONE),
    (384, 2, 0, 2, "16", "full", ONE),
    (384, 1, 0, 5, "13", "summary", MIXED),
    (385, 2, 0, 1, "R+1", "full", MIXED),
    (385, 1, 0, 2, "20", "summary", ONE),
    (769, 2, 0, 2, "13", "full", ONE),
    (769, 1, 0, 1, "16", "full", MIXED),
    (769, 2, 0, 5, "R+1", "summary", ONE),
    (1537, 4, 3, 5, "20", "summary", MIXED),
    (1537, 4, 3, 5, "20", "summary", ONE),
]


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


_problems = {}


def _problem(n, K):
    from mcmc_clv_model_amd.sampler import build_problem
    if (n, K) not in _problems:
        df = with_covariates(cdnow_tiled(n), K - 1) if K > 1 else cdnow_tiled(n)
        _problems[n, K] = build_problem(df, [f"c{k}" for k in range(1, K)], 2)
    return _problems[n, K]


def _env(monkeypatch, mode):
    for v in ("CLV_PERSISTENT", "CLV_PERSIST_LAYOUT", "CLV_SPLIT_RELAY"):
        monkeypatch.delenv(v, raising=False)
    if mode == "fused":
        monkeypatch.setenv("CLV_PERSISTENT", "0")
    else:
        monkeypatch.setenv("CLV_PERSISTENT", "1")
        monkeypatch.setenv("CLV_PERSIST_LAYOUT", "split")
        monkeypatch.setenv("CLV_SPLIT_RELAY", "1")


@pytest.fixture(scope="module")
def R(L):
    """The library's relay point, as a forced handle reports it."""
    from mcmc_clv_model_amd.sampler import HipSampler
    mp = pytest.MonkeyPatch()
    try:
        _env(mp, "relay")
        with HipSampler(_problem(384, 1), chains=1, n_mh_steps=20, **KW) as s:
            info = s.launch_info()
    finally:
        mp.undo()
    assert info["layout"] == "split"
    assert info["relay_steps"] in (8, 12), info
    return info["relay_steps"]


def _run(monkeypatch, p, mode, chains, chain_first, S, sink, R, runs):
    from mcmc_clv_model_amd.sampler import HipSampler
    _env(monkeypatch, mode)
    with HipSampler(p, chains=chains, chain_first=chain_first, n_mh_steps=S, draw_sink=sink, **KW) as s:
        info = s.launch_info()
        assert info["persistent"] == (mode != "fused")
        assert info["layout"] == (None if mode == "fused" else "split")
        assert info["relay_steps"] == (R if mode == "relay" else 0), (mode, S, info)
        for k in runs:
            s.run(k)
        assert s.launch_info()["layout"] == info["layout"]  # (no abort: the split layout was kept)
        out = dict(zip(("lam", "mu", "beta", "sigma"), s.get_state()))
        l1, l2, ll = s.read_draws()
        out.update(level2=l2, loglik=ll)
        if sink == "full":
            out["level1"] = l1
        else:
            sums, k = s.read_summary()
            out.update(sums=sums, n_summed=np.array([k], np.float64))
    return out


def test_built_share_is_reported(L):
    out = np.full(1, -7, np.int32)
    assert L.clv_debug_split_draw_plan(8, -1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    print("draw share of this library:", int(out[0]))
    assert 0 <= int(out[0]) <= 5


@pytest.mark.parametrize("n,chains,chain_first,K,S_sym,sink,runs", CASES)
def test_relay_drawing_ahead_and_fused_bitwise_equal(L, R, monkeypatch, n, chains, chain_first, K, S_sym, sink, runs):
    S = {"R+1": R + 1, "13": 13, "16": 16, "20": 20}[S_sym]
    p = _problem(n, K)
    res = {m: _run(monkeypatch, p, m, chains, chain_first, S, sink, R, runs) for m in ("relay", "fused")}
    for key, ref in res["fused"].items():
        assert np.isfinite(ref).all() or key == "level1", key
        got = res["relay"][key]
        same = np.array_equal(bits(got), bits(ref))
        assert same, f"relay vs launch-per-sweep: {key} differs in {int((bits(got) != bits(ref)).sum())} of {ref.size}"
    assert res["fused"]["level2"].shape[1] == 4 and res["fused"]["level2"].any()  # draws were stored

"""The relay instance of the split layout (persist_kernel_split with a relay point R: wavefronts 4 and 5
run the first R MH steps of their rows, hand the lane's record over through LDS, and wavefronts 6 and 7
run the rest, finish the rows and reduce them) against the helper instance (CLV_SPLIT_RELAY=0) and the
launch-per-sweep kernel (CLV_PERSISTENT=0): the same results to the bit — carried state, level-1 /
level-2 / log-likelihood draws, the summary sink's sums — over the split test's launch pattern (1, 1, 1,
5, 2, 3 sweeps, burn-in ending inside the run of 5, thin 2), at the smallest sizes where the relay can go
wrong:

  n = 257   row 4 holds one live lane and row 5 none
  n = 384   one workgroup with rows 4 and 5 full
  n = 385   a second workgroup whose relay rows are vacant (their flags are still raised and awaited)
  n = 640   two workgroups; the second's rows 0-3 are live, its relay rows (customers 640..767) vacant
  n = 769   three workgroups, the second with live relayed rows (customers 640..767), full sink: its
            stored level-1 draws are compared
  n = 1537  several workgroups, vacant wavefronts in the last (4 chains from chain 3, K = 5, summary)

K = 1, 2, 5; both sinks; S = 1, R - 1, R (not relayed: relay_steps reports 0), R + 1, 13, 20 with R read
from launch_info()["relay_steps"] of a forced handle.  A few hundred sweeps in all."""
import numpy as np
import pytest

from tests.helpers import bits, cdnow_tiled, with_covariates

pytestmark = pytest.mark.gpu

RUNS = (1, 1, 1, 5, 2, 3)  # 13 sweeps: burn-in 6 ends inside the run of 5
KW = dict(mcmc=8, burnin=6, thin=2, seed=77)

# (customers, chains, chain_first, K, MH steps, sink)
CASES = [
    (257, 2, 0, 2, "20", "full"),
    (257, 1, 0, 1, "R+1", "summary"),
    (384, 2, 0, 2, "20", "full"),
    (384, 1, 0, 5, "13", "summary"),
    (385, 2, 0, 1, "R+1", "full"),
    (385, 1, 0, 2, "R", "summary"),
    (640, 2, 0, 2, "R-1", "full"),
    (640, 1, 0, 1, "1", "full"),
    (640, 2, 0, 5, "20", "full"),
    (640, 1, 0, 2, "13", "summary"),
    (769, 2, 0, 2, "R+1", "full"),
    (769, 1, 0, 1, "20", "full"),
    (1537, 4, 3, 5, "20", "summary"),
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
        monkeypatch.setenv("CLV_SPLIT_RELAY", "1" if mode == "relay" else "0")


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


def _steps(sym, R):
    return {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "13": 13, "20": 20}[sym]


def _run(monkeypatch, p, mode, chains, chain_first, S, sink, R):
    """One handle under `mode` (the environment is read at create), driven through RUNS."""
    from mcmc_clv_model_amd.sampler import HipSampler
    _env(monkeypatch, mode)
    nb = -(-len(p.x) // 256)
    with HipSampler(p, chains=chains, chain_first=chain_first, n_mh_steps=S, draw_sink=sink, **KW) as s:
        info = s.launch_info()
        assert info["persistent"] == (mode != "fused")
        assert info["layout"] == (None if mode == "fused" else "split")
        assert info["relay_steps"] == (R if mode == "relay" and S > R else 0), (mode, S, info)
        if mode != "fused":
            assert info["physical_workgroups"] == (-(-2 * nb // 3) + 1) * chains
        for k in RUNS:
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


@pytest.mark.parametrize("n,chains,chain_first,K,S_sym,sink", CASES)
def test_relay_helpers_and_fused_bitwise_equal(L, R, monkeypatch, n, chains, chain_first, K, S_sym, sink):
    S = _steps(S_sym, R)
    p = _problem(n, K)
    res = {m: _run(monkeypatch, p, m, chains, chain_first, S, sink, R) for m in ("relay", "helpers", "fused")}
    for key, ref in res["fused"].items():
        assert np.isfinite(ref).all() or key == "level1", key
        for m in ("relay", "helpers"):
            got = res[m][key]
            same = np.array_equal(bits(got), bits(ref))
            assert same, f"{m} vs launch-per-sweep: {key} differs in {int((bits(got) != bits(ref)).sum())} of {ref.size}"
    assert res["fused"]["level2"].shape[1] == 4 and res["fused"]["level2"].any()  # draws were stored


@pytest.mark.parametrize("bad", ["2", "on", ""])
def test_relay_env_rejected(L, monkeypatch, bad):
    from mcmc_clv_model_amd.sampler import HipSampler
    _env(monkeypatch, "relay")
    monkeypatch.setenv("CLV_SPLIT_RELAY", bad)
    with pytest.raises(ValueError, match="CLV_SPLIT_RELAY"):
        HipSampler(_problem(257, 1), chains=1, **KW)

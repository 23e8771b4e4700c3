"""The shipped relay instance of the split layout, whose relay wavefronts draw part of the next sweep's
variates in their idle gaps (split_draw_plan), against the float64 model of tests/philox_sweep_ref.py,
value by value: the comparison of tests/test_gpu_split_model.py over a launch long enough for the gaps
to matter.  That module's cases run one and two sweeps per launch, so a chunk drawn ahead is read once at
most; here a launch of 1 is followed by a launch of 12 (the staging buffer and the per-row masks reused
eleven times, every sweep stored), at N = 769, S = 14 (a partial last chunk under either relay point), K =
2: 4 blocks in 3 workgroups, the second with all six rows live, the last with one live lane.  The bitwise
test (test_gpu_persist_relay_draw.py) compares with the launch-per-sweep kernel only; a variate drawn by
the wrong wavefront from the wrong customer's slot in both would pass it, not this."""
import pytest

from tests import philox_sweep_ref as M
from tests.test_gpu_production_sweep import Device, _assert_parity, _report, compare

pytestmark = pytest.mark.gpu

_ENV = {"CLV_PERSISTENT": "1", "CLV_PERSIST_LAYOUT": "split", "CLV_SPLIT_RELAY": "1"}
CASE = dict(D=2, covs=["c1"], data=("tiled", 769, 1), S=M.SPLIT_S, chains=2, chain_first=1, seed=3391,
            burnin=0, mcmc=13, thin=1, drive=[("run", 1), ("run", 12)])


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def test_relay_instance_drawing_ahead_matches_model(L, monkeypatch):
    for k, v in _ENV.items():
        monkeypatch.setenv(k, v)
    mp = M.ModelProblem(M.case_frame(CASE), CASE["covs"], CASE["D"])
    nb = -(-mp.N // M.BLOCK)
    assert mp.N == 769 and nb == 4 and M.split_wgs(nb) == 3
    seen = []

    def on_info(info, when):
        print(f"split_draw ({when} the run): {info}")
        assert info["layout"] == "split" and info["relay_steps"] in (8, 12) and info["relay_steps"] < CASE["S"], \
            (info, L.clv_last_error().decode(errors="replace"))
        assert info["physical_workgroups"] == (M.split_wgs(nb) + 1) * CASE["chains"]
        seen.append(when)

    dev = Device(L, CASE, mp, True, on_info=on_info)
    assert seen == ["before", "after"]
    r = compare(dev, range(dev.C))
    _report("split_draw", dev, r)
    _assert_parity(r, (13, 13))
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0
    # power: the next sweep's variates in the model's place fail most customers
    share = compare(dev, [0], level2=False, var_of=lambda c, s: dev.var[c, s + 1])["fail"].mean()
    print(f"split_draw: power, next sweep's variates fail {share:.2f} of the customers")
    assert share > 0.5

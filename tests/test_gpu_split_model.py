"""The split layout of the persistent sweep (persist_kernel_split, helper and relay instances, and
persist_level2's SPLIT path) against the float64 model of tests/philox_sweep_ref.py, value by value: the
comparison of tests/test_gpu_production_sweep.py (its Device, compare, tolerances and borderline cap,
imported and unchanged) pointed at the kernel that runs the headline workload.  The bitwise tests
(test_gpu_persist_split.py, test_gpu_persist_relay.py) compare the split kernels with the launch-per-sweep
kernel only; an error common to both at a split-specific shape would pass them.

* SPLIT_INSTANCE_CASES (test_every_split_instance_matches_model): every compiled bivariate instance K =
  1..9, helper (CLV_SPLIT_RELAY=0) and relay (=1), forced (CLV_PERSISTENT=1, CLV_PERSIST_LAYOUT=split) at
  N = 769, S = 14, launches of 1 and 2 sweeps with a state read between them.  The layout, the physical
  workgroup count (the plan rule: ceil(4 nb / 6) + 1 per chain) and the relay point are asserted before
  the run and again after it, so a launch that aborted and reverted to the block layout fails.
* SPLIT_GRID_CASES (test_split_grid_matches_model): nb = 129 (level-2 lanes in three wavefronts, block
  127 paired with lane 126), nb = 256 (SPLIT_MAX_NB, default environment), nb = 257 (the forced layout
  declined) and the benchmark's own c2 grid (default environment, 4 chains x 93 blocks).  In the default
  environment the device must take the choice clv_debug_split_choice gives for its own CU count; on a
  256-CU card the expected figures are asserted literally.  nb = 129 and nb = 257 run again under
  CLV_PERSISTENT=0 (test_split_grid_shapes_launch_per_sweep), so a failure can be assigned to the layout
  or to the shape.

Power, on the model's side (same device outputs, one thing wrong in the model's inputs): the next
sweep's variates, the next chain key's, t_l / t_m swapped each fail more than half the customers; the
beta normals' slots shifted by one fails the level-2 record; a split block's extension rows, a relayed
row pair, single wave rows of blocks 127, 124, 64, 253, 91 or a one-customer last block left out of the
level-2 model and of the log-likelihood's sum fail both.

Measured on MI355X (256 CUs, relay point 8; c2 took the split layout with 252 of 376 workgroups, nb = 256
with 172) over the 24 runs: 1 of 795,398 lanes set aside (sg_bi1_256; the model's free run sets aside
the same share, 1 of 130,562, and none elsewhere); largest relative deviations tau 9.1e-15, lambda
1.1e-15, mu 2.3e-15, log-likelihood 3.4e-16, beta 7.9e-12 and Sigma 4.3e-10 elementwise (on entries
near zero, inside the absolute term), level-2 record 2.3e-13 beyond the absolute term.  Helper and
relay runs of a case give the same figures.  Every power check failed its comparison: shares 1.00; a
dropped wave row moves the level-2 record by >= 4.5e-3 and the log-likelihood by >= 1.7e-3 relative, a
one-customer last block by >= 1.2e-4 and >= 7.1e-6 (tolerances 1e-10 and 1e-12).  The module takes 5.7 s of wall time, 2.9 s of it loading the
library and creating the first handle; the slowest case is sg_c2 at 0.3 s.

Checked once against the kernel itself: a library built with persist_level2's third pairing branch (lane
b - 1 polling row 3 of a block b at its wavefront's last lane) disabled fails sg_bi2_129 and sg_bi1_256
on the log-likelihood and the level-2 record, while sg_c2 (no block 127) and the launch-per-sweep rerun
of nb = 129 still pass.
"""
import ctypes

import numpy as np
import pytest

from tests import philox_sweep_ref as M
from tests.test_gpu_production_sweep import Device, _assert_parity, _report, compare

pytestmark = pytest.mark.gpu

_ENV = ("CLV_PERSISTENT", "CLV_PERSIST_LAYOUT", "CLV_SPLIT_RELAY")


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    lib.clv_debug_split_choice.argtypes = [ctypes.c_int32] * 4
    lib.clv_debug_split_choice.restype = ctypes.c_int32
    return lib


def _set_env(monkeypatch, env):
    for v in _ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def R(L):
    """The library's relay point, as a forced handle reports it (as test_gpu_persist_relay.py reads it)."""
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow_tiled
    mp = pytest.MonkeyPatch()
    try:
        _set_env(mp, {"CLV_PERSISTENT": "1", "CLV_PERSIST_LAYOUT": "split", "CLV_SPLIT_RELAY": "1"})
        with HipSampler(build_problem(cdnow_tiled(384), [], 2), chains=1, n_mh_steps=20, mcmc=1, burnin=0, thin=1,
                        seed=1) as s:
            info = s.launch_info()
    finally:
        mp.undo()
    assert info["layout"] == "split"
    assert info["relay_steps"] in (8, 12) and info["relay_steps"] < M.SPLIT_S, info
    return info["relay_steps"]


# largest figures over every run of the module, printed after each (the docstring's record)
_SEEN = dict(runs=0, lanes=0, set_aside=0, tau=0.0, lam=0.0, mu=0.0, loglik=0.0, beta=0.0, Sigma=0.0, l2_net=0.0)


def _record(r):
    _SEEN["runs"] += 1
    for k in ("lanes", "set_aside"):
        _SEEN[k] += r[k]
    for k in ("tau", "lam", "mu", "loglik", "beta", "Sigma", "l2_net"):
        _SEEN[k] = max(_SEEN[k], r[k])
    print("module so far: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in _SEEN.items()))


def _layout_check(L, name, want):
    """The on_info hook: launch_info() must show ``want`` (a dict) before the first launch and after the
    last.  A split launch that aborts makes the run itself raise with clv_last_error()'s text; should a
    handle ever revert without that, the reason is reported here."""
    def check(info, when):
        print(f"{name} ({when} the run): {info}")
        for k, v in want.items():
            assert info[k] == v, (f"{name} {when} the run: {k} is {info[k]!r}, expected {v!r}; last error: "
                                  f"{L.clv_last_error().decode(errors='replace')!r}")
    return check


def _drop_checks(name, dev, mp, l1, drops):
    for what, (lo, hi) in drops.items():
        assert 0 <= lo < hi <= mp.N
        drop = np.zeros(mp.N, bool)
        drop[lo:hi] = True
        d = compare(dev, [0], l1_cache=l1, drop=drop)
        print(f"{name}: power, customers [{lo}, {hi}) ({what}) left out: level-2 record off by {d['l2_net']:.1e}, "
              f"log-likelihood by {d['loglik']:.1e}")
        assert d["l2_fail"] and d["ll_fail"], what


SPLIT_INSTANCE_RUNS = [(n, m) for n in M.SPLIT_INSTANCE_CASES for m in ("helpers", "relay")]


@pytest.mark.parametrize("name,mode", SPLIT_INSTANCE_RUNS, ids=[f"{n}-{m}" for n, m in SPLIT_INSTANCE_RUNS])
def test_every_split_instance_matches_model(L, R, monkeypatch, name, mode):
    case = M.SPLIT_INSTANCE_CASES[name]
    _set_env(monkeypatch, {"CLV_PERSISTENT": "1", "CLV_PERSIST_LAYOUT": "split",
                           "CLV_SPLIT_RELAY": "1" if mode == "relay" else "0"})
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    nb = -(-mp.N // M.BLOCK)
    assert nb == 4 and M.split_wgs(nb) == 3 and case["S"] > R
    want = dict(layout="split", physical_workgroups=(M.split_wgs(nb) + 1) * case["chains"],
                workgroups=(nb + 1) * case["chains"], relay_steps=R if mode == "relay" else 0)
    assert want["physical_workgroups"] == 4 * case["chains"]
    dev = Device(L, case, mp, True, on_info=_layout_check(L, f"{name}-{mode}", want))
    l1 = {}
    r = compare(dev, range(dev.C), l1_cache=l1)
    _report(f"{name}-{mode}", dev, r)
    _record(r)
    _assert_parity(r, (3, 3))
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0
    if mode != "helpers":
        return

    # ---- power: one thing wrong at a time in the model's inputs, same device outputs, chain 0
    def l1_share(**kw):
        return compare(dev, [0], level2=False, **kw)["fail"].mean()

    shares = dict(next_sweep=l1_share(var_of=lambda c, s: dev.var[c, s + 1]),
                  next_chain_key=l1_share(var_of=lambda c, s: dev.var_next_key[s]),
                  t_swapped=l1_share(swap_t=True))
    print(f"{name}: power, share of customers failing: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v > 0.5, (k, v)
    assert compare(dev, [0], l1_cache=l1, beta_slot_shift=1)["l2_fail"]
    _drop_checks(name, dev, mp, l1, M.SPLIT_INSTANCE_DROP)


def _grid_want(L, case, nb, C, n_cu, R):
    """What launch_info() must show for a grid case: the layout the case forces, or, in the default
    environment, the one clv_debug_split_choice gives for the device's CU count."""
    layout = case["layout"]
    if layout == "choice":
        layout = "split" if L.clv_debug_split_choice(C, nb, 1, n_cu) else "block"
    split = layout == "split"
    return dict(layout=layout, workgroups=(nb + 1) * C,
                physical_workgroups=((M.split_wgs(nb) if split else nb) + 1) * C,
                relay_steps=R if split and case["S"] > R else 0)


# what a 256-CU MI355X must show in the default environment, literally
ON_256_CUS = {"sg_c2": dict(layout="split", physical_workgroups=252, workgroups=376),
              "sg_bi1_256": dict(layout="split", physical_workgroups=172)}


@pytest.mark.parametrize("name", list(M.SPLIT_GRID_CASES))
def test_split_grid_matches_model(L, R, monkeypatch, name):
    case = M.SPLIT_GRID_CASES[name]
    _set_env(monkeypatch, case["env"])
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    nb, C = -(-mp.N // M.BLOCK), case["chains"]
    assert mp.N == case["data"][1] and (nb <= M.SPLIT_MAX_NB) == (case["layout"] != "block")
    checks = []

    def on_info(info, when):
        want = _grid_want(L, case, nb, C, info["n_cu"], R)
        print(f"{name}: n_cu {info['n_cu']}, expecting {want}")
        if case["layout"] == "choice" and info["n_cu"] == 256:
            want.update(ON_256_CUS[name])
            if name == "sg_c2":
                want["relay_steps"] = R
        _layout_check(L, name, want)(info, when)
        checks.append(when)

    dev = Device(L, case, mp, True, geometry=(nb, 1, nb, nb), on_info=on_info)
    assert checks == ["before", "after"]
    l1 = {}
    r = compare(dev, range(dev.C), l1_cache=l1)
    _report(name, dev, r)
    _record(r)
    _assert_parity(r, (2, 2))
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0

    # ---- power, on the model's side: rows missing from the reduction break the level-2 record and the
    # log-likelihood; another chain key's variates break the customers
    _drop_checks(name, dev, mp, l1, case["drop"])
    fail = compare(dev, [0], var_of=lambda c, s: dev.var_next_key[s], level2=False)["fail"][0]
    print(f"{name}: power, next_chain_key fails {fail.mean():.2f} of the customers"
          + (f", {fail[65536:].sum()} of the {fail[65536:].size} with index >= 65,536" if mp.N > 65536 else ""))
    assert fail.mean() > 0.5


@pytest.mark.parametrize("name", ["sg_bi2_129", "sg_bi1_257"])
def test_split_grid_shapes_launch_per_sweep(L, monkeypatch, name):
    """The same shapes through the launch-per-sweep kernel, parity only: with the run above it tells a
    fault of the layout from one of the shape."""
    case = M.SPLIT_GRID_CASES[name]
    _set_env(monkeypatch, {"CLV_PERSISTENT": "0"})
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    nb = -(-mp.N // M.BLOCK)
    dev = Device(L, case, mp, False, geometry=(nb, 1, nb, nb), on_info=_layout_check(L, name, dict(layout=None)))
    r = compare(dev, range(dev.C))
    _report(name, dev, r)
    _record(r)
    _assert_parity(r, (2, 2))
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0

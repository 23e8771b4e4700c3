"""The shard plans at their edges, without a GPU (tests/shard_edge_cases.py; the GPU side is
tests/test_gpu_shard_edges.py):

* every case's geometry as ``distributed.plan`` gives it — the shard ranges, the empty ranks, the live
  lanes of each rank's last block, units_per_rank, n_units_global, the partly filled units — so a case
  that stops reaching its edge fails here;
* ``slice_problem`` of an empty range: zero-length columns and a (K - 1, 0) covariate block;
* every rank's kernel choice through clv_debug_sweep_plan against the table in shard_edge_cases (an empty
  rank is fused-only), and the world rule on top of it: a plan with an empty shard takes the fused
  exchange on every rank (clv_debug_world_has_empty_shard, held to the plans themselves);
* the model cases added for the unsharded side (philox_sweep_ref.SHARD_EDGE_GRID) describe the same
  problems, assert their geometry, and follow the oracle's chain to the production module's tolerances.
  (test_philox_sweep_cpu's borderline cap, level-2 sensitivity and summation-order tests run over
  ALL_CASES / GRID_CASES and so over these rows too.)
"""
import ctypes

import numpy as np
import pytest

from tests import philox_sweep_ref as M
from tests import shard_edge_cases as E

BLOCK = E.BLOCK


@pytest.mark.parametrize("name", list(E.CASES))
def test_plan_reaches_the_edge(name):
    case = E.CASES[name]
    plan = E.plan_of(case)
    W, n = case["world"], case["N"]
    assert plan.blocks_per_unit == (case["blocks_per_unit"] or 1)  # (every default here is one block per unit)
    shards = [plan.shard(r) for r in range(W)]
    assert shards == case["shards"]
    assert shards[0][0] == 0 and shards[-1][1] == n and all(shards[r][1] == shards[r + 1][0] for r in range(W - 1))
    assert [r for r, (b, e) in enumerate(shards) if b == e] == E.EMPTY_RANKS[name]
    last = [0 if e == b else (e - b - 1) % BLOCK + 1 for b, e in shards]
    assert last == case["last_lanes"]
    assert plan.units_per_rank == case["units_per_rank"] and plan.n_units_global == case["n_units_global"]
    # customers of every global unit (unit u of rank r is global unit r * units_per_rank + u)
    per_unit = plan.blocks_per_unit * BLOCK
    held = {}
    for r, (b, e) in enumerate(shards):
        assert b == e or b == r * plan.blocks_per_rank * BLOCK  # a shard starts on its rank's first block
        for u in range(plan.units_per_rank):
            lo = b + u * per_unit
            held[r * plan.units_per_rank + u] = max(0, min(e, lo + per_unit) - lo)
    assert sum(held.values()) == n
    assert [u for u, k in sorted(held.items()) if 0 < k < per_unit] == case["part_units"]
    # the units that hold customers are the global units 0 .. n_units_global - 1: the level-2 sum reads no other
    assert [u for u, k in sorted(held.items()) if k > 0] == list(range(plan.n_units_global))


def test_every_edge_is_reached_by_some_case():
    empty = [n for n in E.CASES if E.EMPTY_RANKS[n]]
    assert set(empty) == {"exact_empty", "two_empty", "tail_empty", "abe_world8"}
    assert E.PERSISTENT_CASES == ["one_lane", "part_unit", "part_unit3"]
    assert all(E.CASES[n]["world"] <= 3 for n in E.PERSISTENT_CASES)  # at most three resident grids on one card
    one_lane_only = [n for n, c in E.CASES.items() if any(e - b == 1 for b, e in c["shards"])]
    assert set(one_lane_only) == {"one_lane", "part_unit3"}
    # a partly filled last unit on a rank other than rank 0, with blocks_per_unit > 1
    assert all(E.CASES[n]["blocks_per_unit"] > 1 and E.CASES[n]["part_units"][0] >= E.CASES[n]["units_per_rank"]
               for n in ("part_unit", "part_unit3"))
    assert {c["sink"] for c in E.CASES.values()} == {"full", "summary"}
    assert [n for n, c in E.CASES.items() if c["sink"] == "full"] == ["one_lane", "two_empty", "part_unit"]


@pytest.mark.parametrize("name", ["exact_empty", "two_empty", "abe_world8"])
def test_slice_problem_of_an_empty_range(name):
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.sampler import build_problem
    case = E.CASES[name]
    p = build_problem(E.frame(case), E.covariates(case), case["D"])
    assert (p.N, p.K, p.D) == (case["N"], case["K"], case["D"])
    for r in E.EMPTY_RANKS[name]:
        q = Dm.slice_problem(p, *case["shards"][r])
        assert q.N == 0 and q.x.shape == q.t_x.shape == q.T_cal.shape == (0,)
        assert q.x.dtype == np.int32 and q.t_x.dtype == q.T_cal.dtype == np.float64
        assert q.cov.shape == (case["K"] - 1, 0) and q.cov.flags.c_contiguous
        assert (q.log_s is None) == (case["D"] == 2) and (q.log_s is None or q.log_s.shape == (0,))
        assert q.lam_init == p.lam_init and q.V is p.V  # the setup constants stay the whole problem's
    b, e = case["shards"][0]
    q0 = Dm.slice_problem(p, b, e)
    assert q0.N == e - b and np.array_equal(q0.cov, p.cov[:, b:e])


# scratch bytes per lane of the peer instances capi.hip documents (PERSIST_SCRATCH_MAX's comment); 0 elsewhere
_PEER_SCRATCH = {(2, 5): 56, (3, 3): 48}
_CHOICE = {"peer": dict(p2p_capable=1, p2p_persist_fits=1, fx_capable=1), "fused": dict(fx_capable=1)}
_KEYS = ("persistent", "split", "relay_steps", "p2p_capable", "p2p_persist_fits", "fx_capable", "defer", "need")


def _sweep_plan(L, case, nb):
    v = [case["D"], case["K"], E.RUN["n_mh_steps"], E.RUN["chains"], nb, case["blocks_per_unit"] or 1,
         case["n_units_global"], case["world"], 0, 256, 2, _PEER_SCRATCH.get((case["D"], case["K"]), 0), 1, 0, 1, 0,
         -1, 0, -1, 1]
    out = (ctypes.c_int32 * 8)()
    assert L.clv_debug_sweep_plan((ctypes.c_int64 * 20)(*v), out) == 0
    return dict(zip(_KEYS, out))


@pytest.mark.parametrize("name", list(E.CASES))
def test_kernel_choice_of_every_rank(name):
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    case = E.CASES[name]
    plan = E.plan_of(case)
    for r, (b, e) in enumerate(case["shards"]):
        got = _sweep_plan(L, case, -(-(e - b) // BLOCK))
        assert got == dict(dict.fromkeys(_KEYS, 0), **_CHOICE[case["choice"][r]]), (name, r, got)
        assert (case["choice"][r] == "fused") == (r in E.EMPTY_RANKS[name])  # here only an empty rank is fused-only
    # the world rule: a plan with an empty shard runs no persistent peer kernel on any rank
    has_empty = L.clv_debug_world_has_empty_shard(case["N"], case["world"], plan.blocks_per_rank)
    assert bool(has_empty) == bool(E.EMPTY_RANKS[name])
    assert (name in E.PERSISTENT_CASES) == (not has_empty and all(c == "peer" for c in case["choice"]))


def test_world_rule_agrees_with_the_plan_everywhere():
    """clv_debug_world_has_empty_shard against distributed.plan's own shard ranges, at every world size up
    to 9 and every block count up to 70 (a lane short of, on and past each block boundary)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd import distributed as Dm
    L = _lib.lib()
    assert L.clv_debug_world_has_empty_shard(2357, 8, 2) == 1 and L.clv_debug_world_has_empty_shard(23570, 8, 12) == 0
    assert L.clv_debug_world_has_empty_shard(1, 1, 1) == 0
    n_empty = 0
    for world in range(1, 10):
        for nb in range(1, 71):
            for n in (nb * BLOCK - 255, nb * BLOCK - 1, nb * BLOCK):
                for bpu in (None, 2, 4):
                    plan = Dm.plan(n, world, blocks_per_unit=bpu)
                    empty = any(b == e for b, e in (plan.shard(r) for r in range(world)))
                    assert bool(L.clv_debug_world_has_empty_shard(n, world, plan.blocks_per_rank)) == empty, (n, world, bpu)
                    n_empty += empty
    assert n_empty > 100


@pytest.mark.parametrize("name", list(E.CASES))
def test_model_case_of_the_unsharded_side(name):
    case, grid = E.CASES[name], M.GRID_CASES[M.SHARD_EDGE_GRID[name]]
    assert M.SHARD_EDGE_GRID[name] in M.ALL_CASES
    assert (grid["D"], len(grid["covs"]) + 1, grid["data"][1], grid["blocks_per_unit"]) == \
        (case["D"], case["K"], case["N"], case["blocks_per_unit"])
    assert grid["covs"] == E.covariates(case) and grid["data"][0] == case["data"]
    assert M.case_frame(grid).equals(E.frame(case))  # the same customers, the same covariates
    nb = -(-case["N"] // BLOCK)
    bpu = case["blocks_per_unit"] or 1
    assert M.grid_geometry(grid) == grid["geometry"] == (nb, bpu, -(-nb // bpu), case["n_units_global"])
    assert grid["chains"] == E.RUN["chains"]
    # a blocks_per_unit > 1 run at world size 1 is never persistent (its fused tail sums the units)
    assert grid["modes"] == (dict(default=False) if bpu > 1 else dict(default=True, launch_per_sweep=False))
    for lo, hi in grid["drop"].values():
        assert 0 <= lo < hi <= case["N"]


@pytest.mark.parametrize("name", sorted(M.SHARD_EDGE_GRID.values()))
def test_model_case_follows_the_oracle_chain(name):
    """Pinned to the reference as the production module's cases are: the model, teacher-forced along the
    oracle's own chain on oracle.philox's variates, at RTOL / L2_RTOL / L2_ATOL and the borderline cap."""
    from tests.test_philox_sweep_cpu import test_model_sweep_agrees_with_the_oracle_chain as pin
    pin(name)

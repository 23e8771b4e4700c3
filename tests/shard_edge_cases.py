"""The shard plans at their edges: one table for tests/test_shard_edges_cpu.py (the geometry and the
kernel choice, no GPU) and tests/test_gpu_shard_edges.py (every sharded exchange against the unsharded
run, bit for bit).  Each row names a plan that ``distributed.plan`` returns in ordinary use and that no
comfortable shape reaches: a shard with no customers, a shard whose only block has one live lane, a last
unit that is only partly filled on a rank other than rank 0.

Per case: D, K, N, world and blocks_per_unit (0: the plan's default) as run; ``shards``: every rank's
customer range; ``last_lanes``: live lanes of each rank's last block (0: no block); ``units_per_rank``,
``n_units_global``; ``part_units``: the global units holding fewer than blocks_per_unit * 256 customers
(but some); ``sink``: the draw sink the GPU module compares under; ``choice``: each rank's kernel choice
by clv_create's per-rank rule (clv_debug_sweep_plan on 256 CUs) — "peer": the persistent peer kernel and
the fused exchange, "fused": the fused exchange only, as every rank without a block.  A world with an
empty rank takes the fused exchange on every rank (clv_debug_world_has_empty_shard), so the persistent
peer kernel may run in the cases without one only.
"""
BLOCK = 256

# the run every route makes: 2 chains, 8 sweeps (3 burn-in, 5 kept at thin 2: 3 draws), driven in calls
# of 1, 3 and 4 where the route takes run(n), so a launch both starts and ends mid-run
RUN = dict(mcmc=5, burnin=3, thin=2, chains=2, n_mh_steps=6)
CHUNKS = (1, 3, 4)
SWEEPS = sum(CHUNKS)


def _case(D, K, n, world, bpu, shards, last_lanes, upr, nug, part_units, sink, choice, data="tiled", seed=0):
    return dict(D=D, K=K, N=n, world=world, blocks_per_unit=bpu, shards=shards, last_lanes=last_lanes,
                units_per_rank=upr, n_units_global=nug, part_units=part_units, sink=sink, choice=choice, data=data,
                seed=seed)


CASES = {
    # rank 1 = customers (256, 257): one block, one live lane
    "one_lane": _case(2, 2, 257, 2, 0, [(0, 256), (256, 257)], [256, 1], 1, 2, [1], "full", ["peer", "peer"], seed=5101),
    # N a multiple of the block: rank 1 is empty
    "exact_empty": _case(2, 1, 256, 2, 0, [(0, 256), (256, 256)], [256, 0], 1, 1, [], "summary", ["peer", "fused"],
                         seed=5102),
    # rank 1 has 44 customers, ranks 2 and 3 are empty; trivariate: no initial exchange
    "two_empty": _case(3, 3, 300, 4, 0, [(0, 256), (256, 300), (300, 300), (300, 300)], [256, 44, 0, 0], 1, 2, [1],
                       "full", ["peer", "peer", "fused", "fused"], seed=5103),
    # blocks_per_rank 2: rank 2 has a full block plus one lane, rank 3 is empty while ranks 0-2 have two units each
    "tail_empty": _case(2, 2, 1281, 4, 0, [(0, 512), (512, 1024), (1024, 1281), (1281, 1281)], [256, 256, 1, 0], 2, 6,
                        [5], "summary", ["peer", "peer", "peer", "fused"], seed=5104),
    # one 4-block unit per rank: rank 1 fills 2 of its unit's 4 blocks, the second with one lane, zero padding after
    "part_unit": _case(3, 3, 1281, 2, 4, [(0, 1024), (1024, 1281)], [256, 1], 1, 2, [1], "full", ["peer", "peer"],
                       seed=5105),
    # rank 2 fills one block of its 2-block unit, with one lane
    "part_unit3": _case(2, 5, 1025, 3, 2, [(0, 512), (512, 1024), (1024, 1025)], [256, 256, 1], 1, 3, [2], "summary",
                        ["peer", "peer", "peer"], seed=5106),
    # the real sample on the 8-GPU layout: ranks 5-7 are empty
    "abe_world8": _case(2, 2, 2357, 8, 0, [(0, 512), (512, 1024), (1024, 1536), (1536, 2048), (2048, 2357)] +
                        [(2357, 2357)] * 3, [256, 256, 256, 256, 53, 0, 0, 0], 2, 10, [9], "summary",
                        ["peer"] * 5 + ["fused"] * 3, data="abe", seed=5107),
}

EMPTY_RANKS = {name: [r for r, (b, e) in enumerate(c["shards"]) if b == e] for name, c in CASES.items()}
# the persistent peer exchange (route e): no empty rank, at most three resident grids on one card
PERSISTENT_CASES = [name for name, c in CASES.items() if not EMPTY_RANKS[name]]


def covariates(case):
    return ["first_sales_scaled"] if case["data"] == "abe" else [f"c{k}" for k in range(1, case["K"])]


def frame(case):
    """The case's CBS: the tiled CDNOW frame with K - 1 uniform covariates (philox_sweep_ref.case_frame), or
    the sample itself."""
    from tests import philox_sweep_ref as M
    from tests.helpers import cdnow
    if case["data"] == "abe":
        return cdnow("abe", case["N"])
    return M.case_frame(dict(data=("tiled", case["N"], case["K"] - 1)))


def plan_of(case):
    from mcmc_clv_model_amd import distributed as Dm
    return Dm.plan(case["N"], case["world"], blocks_per_unit=case["blocks_per_unit"] or None)

"""Measurements of many fits in one launch (csrc/batch.hip); a record, not a
gate.  Writes one JSON object (default profiles/batch_fits.json) and prints it.

  headline  64 fits x 4 chains of 2,357 CDNOW customers each (the ten disjoint tenths of the full
            CBS, reused with different seeds), one covariate, 2,000 sweeps, summary sink.
  tiles     T in {1, 2, 4, 8, 16, 32, 64} tiles of 256 customers per fit (rows of the full CBS taken
            cyclically), with enough fits that fits x chains >= 2 x clv_batch_info's slots ("full
            card"), and again with 4 fits only.
For every case: the wall time of the one mcmc_draw_parameters_many call (max_blocks forced above T,
so every fit takes the batch kernel) with its kernel time by hipEvents, and the wall time of the
Python loop of mcmc_draw_parameters calls over the same fits and seeds — what a user had before —
in the same process on the same card, each after bench.settle_clocks; gpu_clock_ghz by a probe
kernel right after each leg.  ratio = loop wall / batch wall.  default_max_blocks: the largest T
whose full-card ratio is at least 2.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

COVS = ["first_sales_scaled"]
CHAINS = 4
TILES = (1, 2, 4, 8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fits.json"))
    ap.add_argument("--sweeps", type=int, default=2000)
    ap.add_argument("--headline-fits", type=int, default=64)
    ap.add_argument("--tiles", default=",".join(str(t) for t in TILES))
    ap.add_argument("--reps", type=int, default=3, help="timed batch calls per case (median); the loop runs once")
    ap.add_argument("--settle-ms", type=float, default=300.0)
    args = ap.parse_args()

    import bench
    from mcmc_clv_model_amd import _lib, mcmc_draw_parameters, mcmc_draw_parameters_many
    from mcmc_clv_model_amd.batch import batch_info
    from mcmc_clv_model_amd.sampler import build_problem
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_batch: no HIP device visible")
    full = cdnow("full")
    info = batch_info(2, len(COVS) + 1)
    burnin = args.sweeps // 4
    kw = dict(mcmc=args.sweeps - burnin, burnin=burnin, thin=50, chains=CHAINS, draw_sink="summary")
    scratch = bench.scratch_sampler(build_problem(full.iloc[:2357], COVS, D=2), CHAINS, 0)

    def settle():
        bench.settle_clocks(args.settle_ms, 0, scratch)

    def clock():
        return round(scratch.clock_probe(50.0), 4) if scratch is not None else None

    def case(label, fits, T):
        seeds = [1000 + CHAINS * j for j in range(len(fits))]
        mcmc_draw_parameters_many(fits[:2], COVS, seeds=seeds[:2], max_blocks=512, **dict(kw, mcmc=8, burnin=8, thin=4))
        mcmc_draw_parameters(fits[0], COVS, seed=1, trace=0, **dict(kw, mcmc=8, burnin=8, thin=4))
        walls, kms, clocks = [], [], []
        for _ in range(args.reps):
            settle()
            t0 = time.perf_counter()
            out, inf = mcmc_draw_parameters_many(fits, COVS, seeds=seeds, max_blocks=512, return_info=True, **kw)
            walls.append(time.perf_counter() - t0)
            clocks.append(clock())
            kms.append(inf.attrs["kernel_ms"])
            assert set(inf["path"]) == {"batch"}
        settle()
        t0 = time.perf_counter()
        solo = [mcmc_draw_parameters(f, COVS, seed=s, trace=0, **kw) for f, s in zip(fits, seeds)]
        loop = time.perf_counter() - t0
        loop_clock = clock()
        same = all(np.array_equal(a["level_2"][c], b["level_2"][c]) for a, b in zip(out, solo) for c in range(CHAINS))
        wall = float(np.median(walls))
        rec = dict(label=label, fits=len(fits), chains=CHAINS, tiles_per_fit=T, customers_per_fit=len(fits[0]),
                   sweeps=args.sweeps, workgroups=len(fits) * CHAINS, batch_wall_s=round(wall, 4),
                   batch_wall_all_s=[round(w, 4) for w in walls], batch_kernel_s=round(float(np.median(kms)) * 1e-3, 4),
                   batch_us_per_sweep_and_tile=round(float(np.median(kms)) * 1e3 / args.sweeps / T, 3),
                   loop_wall_s=round(loop, 4), ratio=round(loop / wall, 3), same_level2_bits=bool(same),
                   gpu_clock_ghz=dict(batch=clocks, loop=loop_clock))
        print(json.dumps(rec), flush=True)
        return rec

    def rows(start, n):
        return full.iloc[(start + np.arange(n)) % len(full)].reset_index(drop=True)

    rec = dict(timing=f"host wall clock around each call (the calls synchronise), after bench.settle_clocks("
                      f"{args.settle_ms} ms); batch: median of {args.reps}, loop: one run; kernel time by hipEvents",
               model=f"bivariate, covariates {COVS}, {CHAINS} chains, summary sink, thin 50", batch_info=info)
    tenths = [full.iloc[2357 * q:2357 * (q + 1)].reset_index(drop=True) for q in range(10)]
    rec["headline"] = case(f"{args.headline_fits} fits x {CHAINS} chains x 2,357 customers (tenths of the CBS)",
                           [tenths[j % 10] for j in range(args.headline_fits)], 10)
    n_full = -(-2 * info["slots"] // CHAINS)
    table = []
    for T in (int(t) for t in args.tiles.split(",")):
        n = 256 * T
        a = case(f"full card: {n_full} fits of {T} tiles", [rows(j * n, n) for j in range(n_full)], T)
        b = case(f"4 fits of {T} tiles", [rows(j * n, n) for j in range(4)], T)
        table.append(dict(T=T, full_card=a, four_fits=b))
    rec["tiles"] = table
    ok = [r["T"] for r in table if r["full_card"]["ratio"] >= 2.0]
    rec["default_max_blocks"] = max(ok) if ok else 0
    rec["default_max_blocks_rule"] = "the largest T of the sweep whose full-card ratio (loop wall / batch wall) is >= 2"
    rec["resources"] = {f"D{D}K{K}": batch_info(D, K) for D in (2, 3) for K in range(1, 10)}
    if scratch is not None:
        scratch.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

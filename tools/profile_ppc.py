"""Time of the posterior predictive checks on device (csrc/ppc.hip) on c2: the full CDNOW CBS (23,570
customers), 4 chains x 1,000 stored draws, draw_sink="full".  HipSampler.posterior_predictive_check()
at both levels against HipSampler.predict() on the same sampler in the same process: predict does the
nearest existing work, one Poisson count per (draw, customer); a replicate adds one Philox block, an
exponential lifetime, the recency's exp / log pair and the statistics (and, at the population level,
a second block, a Box-Muller pair and two exps).

Kernel time: for the checks, device events around the call's kernels (clv_ppc_info), median of --reps
calls after one warm-up call, the calls alternating; for predict, which has no such record, a kernel
trace taken in a run of its own (``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
python tools/profile_ppc.py --only kernels``) and merged with ``--merge-trace DIR``, which also records the trace's split of a
check over its four kernels.  Host wall-clock times of the synchronous calls are recorded beside them
(predict's includes the read-back of its n_draws x n counts).

The kernel's shape is timed too: work items of 32 draws (the default) against 128, 512 and all draws
(the workgroup-per-block shape), through the CLV_PPC_ITEM_DRAWS knob.

--scale also times 1,000,000 customers (the CBS tiled) x 1,000 level-2 records at the population level
through the host-array route.  Writes one JSON object (default profiles/ppc_c2.json) and prints it.  A
record, not a gate: no target is fixed in advance.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def merge_trace(rec, trace_dir):
    """Kernel rows of rocprofv3's *kernel_stats.csv below trace_dir whose name is one of ours."""
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                for key in ("predict_kernel", "ppc_rep_kernel<0>", "ppc_rep_kernel<1>", "ppc_cust_kernel",
                            "ppc_block_sum_kernel", "ppc_final_kernel"):
                    if key in name:
                        rows[key] = dict(calls=int(r["Calls"]), average_ns=float(r["AverageNs"]),
                                         min_ns=float(r["MinNs"]), max_ns=float(r["MaxNs"]))
    if "predict_kernel" not in rows:
        raise SystemExit(f"profile_ppc: no predict_kernel row below {trace_dir}")
    rec["kernel_trace"] = rows
    pk = rows["predict_kernel"]["average_ns"]
    rec["predict_kernel_s"] = round(pk * 1e-9, 6)
    for lv in ("customer", "population"):
        rec[f"ratio_{lv}_to_predict"] = round(rec[f"ppc_{lv}_kernels_s"] / (pk * 1e-9), 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc_c2.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=2000)
    ap.add_argument("--only", default=None, help="'kernels': one warm-up and one call of each, nothing written "
                                                 "(for a kernel trace)")
    ap.add_argument("--scale", action="store_true", help="also time 1,000,000 customers x 1,000 records")
    ap.add_argument("--merge-trace", default=None, help="add the kernel rows of a rocprofv3 trace to --out")
    args = ap.parse_args()
    if args.merge_trace:
        with open(args.out) as f:
            rec = merge_trace(json.load(f), args.merge_trace)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec))
        return
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow, cdnow_tiled
    if _lib.device_count() < 1:
        raise SystemExit("profile_ppc: no HIP device visible")
    df = cdnow("full")
    covs = ["first_sales_scaled"]
    chains, mcmc = 4, args.draws * args.thin
    p = build_problem(df, covs, D=2)
    info = {}
    S_ALL = chains * args.draws
    with HipSampler(p, mcmc=mcmc, burnin=args.burnin, thin=args.thin, chains=chains, seed=42) as s:
        s.run(args.burnin + mcmc)

        def check(level):
            out = s.posterior_predictive_check(level=level, seed=1)
            info[level] = _lib.ppc_info()
            return out
        fns = dict(ppc_customer=lambda: check("customer"), ppc_population=lambda: check("population"),
                   predict=lambda: s.predict(39.0, seed=1))
        for fn in fns.values():      # warm-up: code objects, allocations
            fn()
        reps = 1 if args.only else args.reps
        ts = {k: [] for k in fns}
        kns = dict(customer=[], population=[])
        for _ in range(reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
                if k != "predict":
                    kns[k[4:]].append(info[k[4:]]["kernel_ns"])
        if args.only:
            print(json.dumps({k: float(np.median(v)) for k, v in ts.items()}))
            return
        # the kernel's shape: work items of 32 draws (the default) against longer ones, up to the shape in
        # which a workgroup walks every draw of its 256-customer block; same bits (tests/test_gpu_ppc.py)
        shapes = {}
        for item in (32, 128, 512, S_ALL):
            os.environ[_lib.PPC_ITEM_ENV] = str(item)
            for lv in ("customer", "population"):
                t = []
                for _ in range(3):
                    check(lv)
                    t.append(info[lv]["kernel_ns"])
                shapes.setdefault(lv, {})["all" if item == S_ALL else str(item)] = round(float(np.median(t)) * 1e-9, 6)
        del os.environ[_lib.PPC_ITEM_ENV]
        res = {lv: check(lv) for lv in ("customer", "population")}
        _, l2, _ = s.read_draws(level1=False)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    n, S = p.N, chains * args.draws
    rec = dict(workload=f"c2: {n} customers, {chains} chains x {args.draws} draws (thin {args.thin}), full sink",
               reps=args.reps, replicates=int(S * n),
               ppc_customer_kernels_s=round(float(np.median(kns["customer"])) * 1e-9, 6),
               ppc_population_kernels_s=round(float(np.median(kns["population"])) * 1e-9, 6),
               ppc_customer_kernels_all_ns=[int(v) for v in kns["customer"]],
               ppc_population_kernels_all_ns=[int(v) for v in kns["population"]],
               ns_per_replicate_customer=round(float(np.median(kns["customer"])) / (S * n), 5),
               ns_per_replicate_population=round(float(np.median(kns["population"])) / (S * n), 5),
               ppc_customer_host_s=round(med["ppc_customer"], 6), ppc_population_host_s=round(med["ppc_population"], 6),
               predict_host_s=round(med["predict"], 6),
               vgprs=dict(customer=info["customer"]["vgprs"], population=info["population"]["vgprs"]),
               scratch_bytes=dict(customer=info["customer"]["scratch_bytes"],
                                  population=info["population"]["scratch_bytes"]),
               kernels_s_by_draws_per_work_item=shapes,
               timing="kernels: device events around the call's kernels (clv_ppc_info), median of reps after one "
                      "warm-up call of each, the calls alternating; host: wall clock around the synchronous call "
                      "(allocation, launches and read-back included); predict's kernel time: --merge-trace",
               statistics={lv: json.loads(res[lv]["statistics"].to_json(orient="index")) for lv in res},
               frequency_0_to_7={lv: json.loads(res[lv]["frequency"].iloc[:8].to_json(orient="index")) for lv in res})
    if args.scale:
        big = cdnow_tiled(1_000_000)
        draws = dict(level_2=[np.ascontiguousarray(l2[0][:1000])])
        A.posterior_predictive_check(draws, big.iloc[:4096], covs, level="population", seed=1)   # warm-up
        t0 = time.perf_counter()
        out = A.posterior_predictive_check(draws, big, covs, level="population", seed=1)
        host = time.perf_counter() - t0
        kn = _lib.ppc_info()["kernel_ns"]
        rec["scale"] = dict(workload="1,000,000 customers (the CBS tiled) x 1,000 level-2 records, population level, "
                                     "host-array route, one call after a small warm-up call",
                            replicates=int(1e9), kernels_s=round(kn * 1e-9, 4), ns_per_replicate=round(kn / 1e9, 5),
                            host_s=round(host, 3), batches=int(-(-1_000_000 // ((_lib.PPC_BATCH_DOUBLES // 1000 // 256) * 256))),
                            share_zero_rep_mean=float(out["statistics"].loc["share_zero", "rep_mean"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

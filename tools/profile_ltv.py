"""Time of the posterior customer lifetime value on device (csrc/ltv.hip) on c2: the full CDNOW CBS
(23,570 customers), 4 chains x 1,000 stored draws, draw_sink="full".  HipSampler.lifetime_value()
(infinite horizon, and a 10-year one, which adds an expm1 per draw and customer) against
HipSampler.level1_summary() on the same sampler in the same process: that call exists unchanged
before this feature, sorts the same number of keys (two series per customer) and reads the draws
three times where lifetime_value reads them once.

Each time is the median of --reps host-timed synchronous calls after one warm-up call, the two
calls alternating.  Writes one JSON object (default profiles/ltv_c2.json) and prints it.  A record,
not a gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltv_c2.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=200)
    args = ap.parse_args()
    from mcmc_clv_model_amd import _lib, analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_ltv: no HIP device visible")
    df = cdnow("full")
    p = build_problem(df, ["first_sales_scaled"], D=2)
    chains, mcmc = 4, args.draws * args.thin
    calls = {}
    with HipSampler(p, mcmc=mcmc, burnin=args.burnin, thin=args.thin, chains=chains, seed=42) as s:
        s.run(args.burnin + mcmc)
        fns = dict(lifetime_value=lambda: s.lifetime_value(),
                   lifetime_value_h520=lambda: s.lifetime_value(horizon=520.0),
                   level1_summary=lambda: s.level1_summary())
        for fn in fns.values():      # warm-up: code objects, the sort's algorithm choice, allocations
            fn()
        ts = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
        ltv = s.lifetime_value()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    ce = A.customer_equity(ltv).iloc[0]
    n, S = p.N, chains * args.draws
    rec = dict(workload=f"c2: {n} customers, {chains} chains x {args.draws} draws (thin {args.thin}), full sink",
               reps=args.reps, level1_bytes=int(S * n * 4 * 8), sorted_keys=int(2 * S * n),
               lifetime_value_s=round(med["lifetime_value"], 6),
               lifetime_value_h520_s=round(med["lifetime_value_h520"], 6),
               level1_summary_s=round(med["level1_summary"], 6),
               ratio=round(med["lifetime_value"] / med["level1_summary"], 3),
               ratio_h520=round(med["lifetime_value_h520"] / med["level1_summary"], 3),
               lifetime_value_min_s=round(min(ts["lifetime_value"]), 6),
               level1_summary_min_s=round(min(ts["level1_summary"]), 6),
               **{k + "_all_s": [round(t, 6) for t in v] for k, v in ts.items()},
               timing="host wall clock around the synchronous call (scratch allocation, launches and the read-back "
                      "included), median of reps after one warm-up call of each, the calls alternating; *_min_s the "
                      "fastest",
               dert=dict(note="discounted expected transactions (monetary = 1), 15 % a year, infinite horizon",
                         equity_mean=float(ce["mean"]), equity_p025=float(ce["p025"]), equity_p975=float(ce["p975"]),
                         value_total_mean=float(ce["value_total_mean"]),
                         n_alive_mean=float(ltv["draws"]["n_alive"].mean()),
                         mu_share_mean=float(ltv["draws"]["mu_share"].mean()),
                         customer_value_mean_median=float(ltv["customers"]["value_mean"].median()),
                         customer_residual_mean_median=float(ltv["customers"]["residual_mean"].median())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

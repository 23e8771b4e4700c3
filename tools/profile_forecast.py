"""Time of the closed-form holdout forecast on device (csrc/forecast.hip) on c2: the full CDNOW CBS
(23,570 customers), 4 chains x 1,000 stored draws, draw_sink="full".  HipSampler.forecast() at k_max 64
(and at 256) against HipSampler.information_criteria() on the same sampler in the same process: both
make one pass over the same 3.0 GB of level-1 draws; per (draw, customer) the forecast runs about
2 k_max float64 recurrence steps where information_criteria evaluates a handful of transcendental
functions (and then sorts).

Each time is the median of --reps host-timed synchronous calls after one warm-up call, the calls
alternating.  Writes one JSON object (default profiles/forecast_c2.json) and prints it.  A record,
not a gate: no target is fixed in advance.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast_c2.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=200)
    ap.add_argument("--only", default=None, help="time this one call alone (for a kernel trace)")
    args = ap.parse_args()
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_forecast: no HIP device visible")
    df = cdnow("full")
    chains, mcmc = 4, args.draws * args.thin
    p = build_problem(df, ["first_sales_scaled"], D=2)
    with HipSampler(p, mcmc=mcmc, burnin=args.burnin, thin=args.thin, chains=chains, seed=42) as s:
        s.run(args.burnin + mcmc)
        fns = dict(forecast_k64=lambda: s.forecast(39.0, k_max=64),
                   forecast_k256=lambda: s.forecast(39.0, k_max=256),
                   forecast_k64_pmf=lambda: s.forecast(39.0, k_max=64, pmf=True),
                   information_criteria=lambda: s.information_criteria())
        if args.only:
            fns = {args.only: fns[args.only]}
        for fn in fns.values():      # warm-up: code objects, allocations
            fn()
        ts = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
        if args.only:
            print(json.dumps({k: float(np.median(v)) for k, v in ts.items()}))
            return
        fc = s.forecast(39.0, k_max=64, pmf=True)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    n, S = p.N, chains * args.draws
    pw = fc["pointwise"]
    rec = dict(workload=f"c2: {n} customers, {chains} chains x {args.draws} draws (thin {args.thin}), full sink",
               reps=args.reps, level1_bytes=int(S * n * 4 * 8),
               recurrence_steps_k64=int(S * n * 2 * 64), recurrence_steps_k256=int(S * n * 2 * 256),
               forecast_k64_s=round(med["forecast_k64"], 6), forecast_k256_s=round(med["forecast_k256"], 6),
               forecast_k64_pmf_s=round(med["forecast_k64_pmf"], 6),
               information_criteria_s=round(med["information_criteria"], 6),
               ratio_to_information_criteria=round(med["forecast_k64"] / med["information_criteria"], 3),
               ratio_k256_to_k64=round(med["forecast_k256"] / med["forecast_k64"], 3),
               ns_per_step_k64=round(med["forecast_k64"] / (S * n * 2 * 64) * 1e9, 5),
               **{k + "_all_s": [round(t, 6) for t in v] for k, v in ts.items()},
               timing="host wall clock around the synchronous call (scratch allocation, the launch and the "
                      "read-back included), median of reps after one warm-up call of each, the calls alternating",
               result=dict(note="bivariate model with first_sales_scaled, T_star = 39, no x_star",
                           expected_total=float(pw["xstar_mean"].sum()), mean_p_alive=float(pw["p_alive"].mean()),
                           mean_p_zero=float(pw["p_zero"].mean()), max_tail_mass=float(pw["tail_mass"].max()),
                           expected_frequency_0_to_7=[float(v) for v in fc["frequency"].to_numpy()[:8]]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

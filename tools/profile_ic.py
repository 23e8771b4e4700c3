"""Time of WAIC and PSIS-LOO on device (csrc/ic.hip) on c2: the full CDNOW CBS (23,570 customers),
4 chains x 1,000 stored draws, draw_sink="full".  HipSampler.information_criteria() against
HipSampler.lifetime_value() and HipSampler.level1_summary() on the same sampler in the same process:
all three read the same 3.0 GB of level-1 draws; information_criteria sorts one series per customer
where the other two sort two, and adds the generalised Pareto fit and two logsumexp per customer.

Each time is the median of --reps host-timed synchronous calls after one warm-up call, the calls
alternating.  Writes one JSON object (default profiles/ic_c2.json) and prints it.  A record, not a
gate: no target is fixed in advance.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ic_c2.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=200)
    ap.add_argument("--only", default=None, help="time this one call alone (for a kernel trace)")
    args = ap.parse_args()
    from mcmc_clv_model_amd import _lib, analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_ic: no HIP device visible")
    df = cdnow("full")
    chains, mcmc = 4, args.draws * args.thin
    ics = {}
    rec = {}
    for model, covs in (("M2", ["first_sales_scaled"]), ("M1", [])):
        p = build_problem(df, covs, D=2)
        with HipSampler(p, mcmc=mcmc, burnin=args.burnin, thin=args.thin, chains=chains, seed=42) as s:
            s.run(args.burnin + mcmc)
            if model == "M1":        # the second model only for the comparison
                ics[model] = s.information_criteria()
                continue
            fns = dict(information_criteria=lambda: s.information_criteria(),
                       lifetime_value=lambda: s.lifetime_value(),
                       level1_summary=lambda: s.level1_summary())
            if args.only:
                fns = {args.only: fns[args.only]}
            for fn in fns.values():      # warm-up: code objects, the sort's algorithm choice, allocations
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
            ics[model] = s.information_criteria()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        n, S = p.N, chains * args.draws
        rec = dict(workload=f"c2: {n} customers, {chains} chains x {args.draws} draws (thin {args.thin}), full sink",
                   reps=args.reps, level1_bytes=int(S * n * 4 * 8), sorted_keys=int(S * n),
                   tail_values=int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S)))),
                   information_criteria_s=round(med["information_criteria"], 6),
                   lifetime_value_s=round(med["lifetime_value"], 6),
                   level1_summary_s=round(med["level1_summary"], 6),
                   ratio_to_lifetime_value=round(med["information_criteria"] / med["lifetime_value"], 3),
                   ratio_to_level1_summary=round(med["information_criteria"] / med["level1_summary"], 3),
                   information_criteria_min_s=round(min(ts["information_criteria"]), 6),
                   **{k + "_all_s": [round(t, 6) for t in v] for k, v in ts.items()},
                   timing="host wall clock around the synchronous call (scratch allocation, launches and the "
                          "read-back included), median of reps after one warm-up call of each, the calls "
                          "alternating; *_min_s the fastest")
    k = ics["M2"]["pointwise"]["pareto_k"].to_numpy()
    cmp = A.compare_models(ics)
    rec["result"] = dict(
        note="M2 = bivariate model with first_sales_scaled, M1 = without; transaction likelihood, reff = 1",
        **{m: dict(elpd_loo=float(ic["loo"]["elpd"].iloc[0]), se=float(ic["loo"]["se"].iloc[0]),
                   p_loo=float(ic["loo"]["p"].iloc[0]), elpd_waic=float(ic["waic"]["elpd"].iloc[0]),
                   p_waic=float(ic["waic"]["p"].iloc[0]), n_bad_k=int(ic["loo"]["n_bad_k"].iloc[0]))
           for m, ic in ics.items()},
        pareto_k_quantiles_M2={q: float(np.quantile(k[np.isfinite(k)], float(q))) for q in ("0.5", "0.9", "0.99", "1.0")},
        pareto_k_not_fitted_M2=int(np.count_nonzero(~np.isfinite(k))),
        compare={m: dict(rank=int(r["rank"]), elpd_diff=float(r["elpd_diff"]), dse=float(r["dse"]))
                 for m, r in cmp.iterrows()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

"""Time of the on-device convergence diagnostics (csrc/diag.hip) at the c2 shape: 23,570 CDNOW
customers, 4 chains x 1,000 stored draws, full sink — 94,280 level-1 series of 4 x 1,000 draws.

After a warm-up call it times, on the same sampler, HipSampler.diagnostics() (level 1 and level 2)
and level1_summary(), the existing function closest in work (it gathers two columns and sorts
them), and records the distribution of the truncation lag, which is what the per-lag pass costs by.
Writes one JSON object (default profiles/diag_c2.json) and prints it.  A record, not a gate.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_c2.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import bench
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df, D, covs, chains, burnin, mcmc, thin, sink = bench.load_workload("c2")
    p = build_problem(df, covs, D)
    with HipSampler(p, mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=42, draw_sink="full") as s:
        s.run(burnin + mcmc)

        def timed(fn):
            fn()  # warm-up
            s.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), ts

        t_diag, all_diag = timed(lambda: s.diagnostics())
        t_l1, _ = timed(lambda: s.diagnostics(level2=False))
        t_sum, all_sum = timed(lambda: s.level1_summary())
        d = s.diagnostics()
        n_draws, n = s.n_draws, s.n
    l1 = d["level_1"]
    rec = dict(workload=f"c2: {n} customers, {chains} chains x {n_draws} draws, full sink",
               n_series_level1=int(n * (D + 2)), reps=args.reps,
               diagnostics_s=round(t_diag, 6), diagnostics_level1_only_s=round(t_l1, 6),
               level1_summary_s=round(t_sum, 6), ratio=round(t_diag / t_sum, 3),
               diagnostics_all_s=[round(t, 6) for t in all_diag], level1_summary_all_s=[round(t, 6) for t in all_sum],
               diagnostics_min_s=round(min(all_diag), 6), level1_summary_min_s=round(min(all_sum), 6),
               timing="host wall clock around the synchronous call (scratch allocation included), median of reps "
                      "after one warm-up call; *_min_s the fastest")
    for col in [c for c in l1.columns if c.startswith("lag_")]:
        v = l1[col].to_numpy()
        ok = np.isfinite(v)
        q = np.percentile(v[ok], [0, 50, 90, 99, 100]) if ok.any() else [float("nan")] * 5
        rec[col] = dict(nan=int((~ok).sum()), min=float(q[0]), median=float(q[1]), p90=float(q[2]), p99=float(q[3]),
                        max=float(q[4]), beyond_first_64_lags=int((v[ok] + 2 >= 64).sum()))
    for col in [c for c in l1.columns if c.startswith(("rhat_", "ess_"))]:
        v = l1[col].to_numpy()
        ok = np.isfinite(v)
        if ok.any():
            rec[col] = dict(median=float(np.median(v[ok])), p99=float(np.percentile(v[ok], 99)), max=float(v[ok].max()),
                            min=float(v[ok].min()))
    rec["level_2"] = {k: {c: float(x) for c, x in row.items()} for k, row in d["level_2"].to_dict("index").items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

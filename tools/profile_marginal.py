"""Time and outcome of the marginal WAIC / PSIS-LOO on device (csrc/marginal.hip) on c2: the full CDNOW
CBS (23,570 customers), 4 chains x 1,000 stored draws, draw_sink="full", for M1 (no covariate) and M2
(first_sales_scaled).  On the same sampler in the same process: HipSampler.information_criteria() (the
conditional criteria of csrc/ic.hip) against HipSampler.marginal_information_criteria().

Kernel time of the quadrature: device events around the call's kernels (clv_marginal_info), median of
--reps calls after one warm-up call; the achieved fp64 rate counts what the kernel's source spends per
(record, customer) item at order Q — 2 components x (Q^2 + Q + 2 (NEWTON + 1)) calls of exp, Q^2 + 2 of log and the
arithmetic between them — as FLOPS_PER_NODE flops per node, a round figure of the instruction mix, so
the rate is indicative only.  Host wall-clock times of the synchronous calls are recorded beside them.
Outcome: n_bad_k, the median Pareto k and p_loo of both kinds on both fits, and the compare_models table
of the marginal entries with the Pareto/NBD maximum-likelihood row (in-sample).

Writes one JSON object (default profiles/marginal_c2.json) and prints it.  A record, not a gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FLOPS_PER_NODE = 150   # exp(b), log(lambda + mu), the running maximum's exp: about 40 fp64 operations each, and h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_c2.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=2000)
    ap.add_argument("--customers", type=int, default=None, help="the first N customers only (a quick look)")
    args = ap.parse_args()
    from mcmc_clv_model_amd import ParetoNBDFitter, _lib
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_marginal: no HIP device visible")
    df = cdnow("full", args.customers)
    chains, mcmc = 4, args.draws * args.thin
    R = chains * args.draws
    rec = dict(workload=f"c2: {len(df)} customers, {chains} chains x {args.draws} draws (thin {args.thin}), full sink",
               reps=args.reps, items=int(R * len(df)))
    entries = {}
    for name, covs in (("M1", []), ("M2", ["first_sales_scaled"])):
        p = build_problem(df, covs, D=2)
        with HipSampler(p, mcmc=mcmc, burnin=args.burnin, thin=args.thin, chains=chains, seed=42) as s:
            s.run(args.burnin + mcmc)
            fns = dict(conditional=lambda: s.information_criteria(), marginal=lambda: s.marginal_information_criteria())
            res, ts, kns = {}, {k: [] for k in fns}, []
            for k, fn in fns.items():      # warm-up: code objects, allocations
                res[k] = fn()
            for _ in range(args.reps):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    res[k] = fn()
                    ts[k].append(time.perf_counter() - t0)
                    if k == "marginal":
                        kns.append(_lib.marginal_info()["kernel_ns"])
            info = _lib.marginal_info()
            by_order = {}
            for q in _lib.MARGINAL_ORDERS:
                out = s.marginal_information_criteria(nodes=q)
                by_order[str(q)] = dict(kernel_s=round(_lib.marginal_info()["kernel_ns"] * 1e-9, 5),
                                        elpd_loo=float(out["loo"]["elpd"].iloc[0]))
        kern = float(np.median(kns)) * 1e-9
        Q = info["default_nodes"]
        nodes = 2 * (Q * Q + 2 * (info["newton"] + 1))
        row = dict(host_s={k: round(float(np.median(v)), 5) for k, v in ts.items()}, marginal_kernel_s=round(kern, 5),
                   marginal_kernel_all_ns=[int(v) for v in kns], kernel_share_of_call=round(kern / float(np.median(ts["marginal"])), 3),
                   ns_per_item=round(kern * 1e9 / (R * len(df)), 4), vgprs=info["vgprs"], scratch_bytes=info["scratch_bytes"],
                   fp64_tflops_indicative=round(R * len(df) * nodes * FLOPS_PER_NODE / kern * 1e-12, 2), by_order=by_order)
        for kind in ("conditional", "marginal"):
            pw = res[kind]["pointwise"]
            loo, waic = res[kind]["loo"].iloc[0], res[kind]["waic"].iloc[0]
            row[kind] = dict(elpd_loo=float(loo["elpd"]), se=float(loo["se"]), p_loo=float(loo["p"]), n_bad_k=int(loo["n_bad_k"]),
                             median_k=float(np.nanmedian(pw["pareto_k"].to_numpy())),
                             max_k=float(np.nanmax(pw["pareto_k"].to_numpy())), elpd_waic=float(waic["elpd"]),
                             p_waic=float(waic["p"]), n_p_waic_above_0p4=int(np.count_nonzero(pw["p_waic"].to_numpy() > 0.4)))
        rec[name] = row
        entries["HB " + name] = res["marginal"]
    fit = ParetoNBDFitter().fit(df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float))
    entries["Pareto/NBD (MLE)"] = fit.information_criteria(df["x"].to_numpy(), df["t_x"].to_numpy(float),
                                                           df["T_cal"].to_numpy(float))
    rec["compare_models"] = json.loads(A.compare_models(entries).to_json(orient="index"))
    rec["timing"] = ("kernel: device events around the quadrature kernels (clv_marginal_info), median of reps after one "
                     "warm-up call, alternating with the conditional call; host: wall clock around the synchronous call")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

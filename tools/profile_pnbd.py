"""Time of the Pareto/NBD likelihood on device (csrc/pnbd.hip, mcmc_clv_model_amd/mle.py) at
N = 23,570 (the full CDNOW CBS) and N = 1,000,000 (data.synthetic_cbs): one clv_pnbd_eval, a whole
ParetoNBDFitter.fit from params = 1, and the float64 numpy model's evaluation (tests/pnbd_ref.py)
on the same host, with the series-term counts of the model at the evaluated parameters.

Each device time is the median of --reps host-timed synchronous calls after one warm-up call.
Writes one JSON object (default profiles/pnbd_eval.json) and prints it.  A record, not a gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PARAMS = (0.55, 10.58, 0.61, 11.67)   # near the CDNOW optimum


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 6) for t in ts]


def one_size(name, x, tx, T, reps, model_rows):
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, PnbdData
    from tests import pnbd_ref as R
    with PnbdData(x, tx, T) as d:
        t_eval, all_eval = timed(lambda: d.eval(PARAMS), reps)
        t_cust, _ = timed(lambda: d.customers(PARAMS, 39.0), max(3, reps // 3))
        sums, n_unc = d.eval(PARAMS)
    t0 = time.perf_counter()
    f = ParetoNBDFitter().fit(x, tx, T)
    t_fit = time.perf_counter() - t0
    k = min(len(x), model_rows)           # the numpy model on the first k rows, scaled to N
    t0 = time.perf_counter()
    m = R.model_customers(x[:k], tx[:k], T[:k], PARAMS)
    t_model = (time.perf_counter() - t0) * len(x) / k
    return dict(workload=name, n=int(len(x)), params=list(PARAMS), reps=reps, eval_s=round(t_eval, 6), eval_all_s=all_eval,
                customers_s=round(t_cust, 6), customers_per_s_eval=round(len(x) / t_eval, 1),
                fit_s=round(t_fit, 4), fit_n_eval=f.n_eval_, fit_n_iter=f.n_iter_, fit_converged=bool(f.converged_),
                fit_params=[float(v) for v in f.params_], fit_log_likelihood=f.log_likelihood_,
                sum_log_l=float(sums[0]), n_unconverged=n_unc,
                numpy_model_eval_s=round(t_model, 4), numpy_model_rows=int(k),
                numpy_over_device=round(t_model / t_eval, 1),
                series_terms_mean=float(m["terms"].mean()), series_terms_max=int(m["terms"].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnbd_eval.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--model-rows", type=int, default=100_000)
    args = ap.parse_args()
    from mcmc_clv_model_amd.data import synthetic_cbs
    from tests.helpers import cdnow
    df = cdnow("full")
    syn = synthetic_cbs(1_000_000, 2)
    rec = dict(timing="host wall clock around the synchronous call (launches, the fixed-order final sum and the "
                      "read-back included), median of reps after one warm-up; fit_s is one whole fit from params = 1 "
                      "incl. the upload; the numpy model is timed on numpy_model_rows rows and scaled to n",
               sizes=[one_size("cdnow full CBS", df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy(),
                               args.reps, args.model_rows),
                      one_size("synthetic_cbs(1,000,000, K=2)", syn["x"].to_numpy(), syn["t_x"].to_numpy(),
                               syn["T_cal"].to_numpy(), args.reps, args.model_rows)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

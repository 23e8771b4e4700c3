"""Time of the maximum-marginal-likelihood kernels (csrc/mml.hip) at N = 23,570 (the full
CDNOW CBS with first_sales_scaled) and N = 1,000,000 (data.synthetic_cbs, K = 2), with the method of
tools/profile_pnbd.py: each time is the median of --reps host-timed synchronous calls after one warm-up call.

Per size, in one process on the same data: one clv_mml_eval (value and the 2K + 6 moment sums) against one
marginal_log_likelihood of the same single record (the value-only kernel of csrc/marginal.hip), one
clv_mml_customers, and a whole fit from the default start with its evaluation count (with and without standard
errors).  Then the c2 comparison (tools/profile_mle_ext.py's workload: the full CDNOW CBS, 4 chains x 1,000 stored
draws): HB M2, HB M1, the log-normal MML with and without first_sales_scaled and the two gamma-mixed MLEs in one
compare_models table.

Writes one JSON object (default profiles/mml.json) and prints it.  A record, not a gate.
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RECORD = (-3.48, 0.2, -3.66, 0.1, 1.3, 0.33, 4.06)   # near the CDNOW optimum with first_sales_scaled


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def one_size(name, df, cov_name, reps):
    from mcmc_clv_model_amd import LogNormalParetoNBDFitter, _lib, marginal_log_likelihood
    from mcmc_clv_model_amd.mle import MmlData
    a = (df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float))
    rec = np.array(RECORD)
    row = dict(workload=name, n=int(len(df)), K=2, reps=reps)
    with MmlData(*a, None, df[[cov_name]]) as d:
        row["mml_eval_s"] = round(timed(lambda: d.eval(rec, 32), reps), 6)
        row["mml_eval_kernel_ns"] = _lib.mml_info()["eval_kernel_ns"]
        row["mml_customers_s"] = round(timed(lambda: d.customers(rec, 32, 39.0), reps), 6)
    draws = rec.reshape(1, 1, -1)
    row["marginal_loglik_s"] = round(timed(lambda: marginal_log_likelihood(draws, df, [cov_name], nodes=32), reps), 6)
    row["marginal_kernel_ns"] = _lib.marginal_info()["kernel_ns"]
    row["mml_eval_over_marginal"] = round(row["mml_eval_s"] / row["marginal_loglik_s"], 3)
    row["mml_kernel_over_marginal_kernel"] = round(row["mml_eval_kernel_ns"] / row["marginal_kernel_ns"], 3)
    for se in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # recorded below instead
            t0 = time.perf_counter()
            f = LogNormalParetoNBDFitter().fit(*a, covariates=df[[cov_name]], standard_errors=se)
            dt = time.perf_counter() - t0
        key = "fit_se" if se else "fit"
        row.update({f"{key}_s": round(dt, 4), f"{key}_n_eval": f.n_eval_, f"{key}_converged": bool(f.converged_),
                    f"{key}_grad_norm": f.grad_norm_})
    row.update(fit_log_likelihood=f.log_likelihood_, fit_n_nonfinite=f.n_nonfinite_, fit_params=[float(v) for v in f.params_],
               fit_se=[float(v) for v in f.standard_errors_])
    return row


def c2_comparison(draws, thin, burnin):
    from mcmc_clv_model_amd import LogNormalParetoNBDFitter, ParetoNBDFitter, likelihood_ratio_test
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    df = cdnow("full")
    chains, mcmc = 4, draws * thin
    entries = {}
    for name, covs in (("M2", ["first_sales_scaled"]), ("M1", [])):
        with HipSampler(build_problem(df, covs, D=2), mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=42) as s:
            s.run(burnin + mcmc)
            entries["HB " + name] = s.marginal_information_criteria()
    a = (df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float))
    cov = df[["first_sales_scaled"]]
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # recorded below instead
        ln1 = LogNormalParetoNBDFitter().fit(*a, standard_errors=True)
        ln2 = LogNormalParetoNBDFitter().fit(*a, covariates=cov, standard_errors=True)
        g1 = ParetoNBDFitter().fit(*a)
        g2 = ParetoNBDFitter().fit(*a, covariates=cov)
    entries["log-normal Pareto/NBD + first_sales_scaled (MML)"] = ln2.information_criteria(*a, covariates=cov)
    entries["log-normal Pareto/NBD (MML)"] = ln1.information_criteria(*a)
    entries["Pareto/NBD + first_sales_scaled (MLE)"] = g2.information_criteria(*a, covariates=cov)
    entries["Pareto/NBD (MLE)"] = g1.information_criteria(*a)
    for key, f in (("mml", ln1), ("mml_cov", ln2), ("mle", g1), ("mle_cov", g2)):
        out[key] = dict(log_likelihood=f.log_likelihood_, converged=bool(f.converged_), grad_norm=f.grad_norm_,
                        n_eval=f.n_eval_, params={k: float(v) for k, v in f.params_.items()})
    out["mml_cov"]["summary"] = json.loads(ln2.summary_.to_json(orient="index"))
    out["mml_cov"]["n_nonfinite"] = ln2.n_nonfinite_
    return dict(workload=f"c2: {len(df)} customers, {chains} chains x {draws} draws (thin {thin}), full sink",
                compare_models=json.loads(A.compare_models(entries).to_json(orient="index")), fits=out,
                covariate_max=float(cov.to_numpy().max()), likelihood_ratio_test_mml=likelihood_ratio_test(ln1, ln2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mml.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain of the c2 comparison")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=2000)
    ap.add_argument("--skip-c2", action="store_true")
    args = ap.parse_args()
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.data import synthetic_cbs
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_mml: no HIP device visible")
    rec = dict(timing="host wall clock around the synchronous call (the record's upload, the launches, the fixed-order final "
                      "sum and the read-back included; marginal_log_likelihood uploads the data on every call, clv_mml_eval "
                      "keeps it resident), median of reps after one warm-up; marginal_kernel_ns is the device time of "
                      "marginal.hip's kernels alone; the fits are one whole fit from the default start incl. the upload",
               info=_lib.mml_info(),
               sizes=[one_size("cdnow full CBS", cdnow("full"), "first_sales_scaled", args.reps),
                      one_size("synthetic_cbs(1,000,000, K=2)", synthetic_cbs(1_000_000, 2), "c1", args.reps)])
    if not args.skip_c2:
        rec["c2"] = c2_comparison(args.draws, args.thin, args.burnin)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

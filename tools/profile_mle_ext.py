"""Time of the classical baseline's extensions on device (csrc/pnbd.hip covariate kernels and DERT, csrc/gg.hip;
DESIGN.md section 4m) at N = 23,570 (the full CDNOW CBS) and N = 1,000,000 (data.synthetic_cbs), with the method
of tools/profile_pnbd.py: each time is the median of --reps host-timed synchronous calls after one warm-up call.

Per size: one clv_pnbd_eval as it stands (measured again in this process), one clv_pnbd_eval_cov at K1 = K2 = 0,
1, 3 and 8 (U(-1, 1) covariates, coefficients 0.05), a covariate fit with standard errors (K1 = K2 = 1), one
Gamma-Gamma evaluation and a whole fit, one DERT call.  Then the c2 comparison (tools/profile_marginal.py's
workload: the full CDNOW CBS, 4 chains x 1,000 stored draws): the compare_models table of HB M1, HB M2, the
Pareto/NBD MLE and the covariate MLE with M2's own covariate, first_sales_scaled.

Writes one JSON object (default profiles/mle_ext.json) and prints it.  A record, not a gate.
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
GG_PARAMS = (6.25, 3.74, 15.44)
KS = (0, 1, 3, 8)


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def one_size(name, x, tx, T, n_spend, m_spend, reps):
    from mcmc_clv_model_amd.mle import GammaGammaFitter, GgData, ParetoNBDFitter, PnbdData
    n = len(x)
    Z = np.random.default_rng(7).uniform(-1.0, 1.0, (n, 8))
    row = dict(workload=name, n=int(n), reps=reps)
    with PnbdData(x, tx, T) as d:
        row["eval_plain_s"] = round(timed(lambda: d.eval(PARAMS), reps), 6)
        row["dert_s"] = round(timed(lambda: d.dert(PARAMS, np.log1p(0.15) / 52.0, np.inf), reps), 6)
        row["dert_h52_s"] = round(timed(lambda: d.dert(PARAMS, np.log1p(0.15) / 52.0, 52.0), reps), 6)
        for k in KS:
            d.set_covariates(Z[:, :k].T, Z[:, :k].T)
            p = np.concatenate([PARAMS, np.full(2 * k, 0.05)])
            row[f"eval_cov_k{k}_s"] = round(timed(lambda: d.eval_cov(p), reps), 6)
            row[f"eval_cov_k{k}_over_plain"] = round(row[f"eval_cov_k{k}_s"] / row["eval_plain_s"], 3)
        d.set_covariates(Z[:, :3].T, Z[:, :3].T)
        row["customers_cov_k3_s"] = round(timed(lambda: d.customers_cov(np.concatenate([PARAMS, np.full(6, 0.05)]), 39.0),
                                                max(3, reps // 3)), 6)
    t0 = time.perf_counter()
    f = ParetoNBDFitter().fit(x, tx, T, covariates=Z[:, :1], standard_errors=True)
    row.update(fit_cov_se_s=round(time.perf_counter() - t0, 4), fit_cov_n_eval=f.n_eval_, fit_cov_converged=bool(f.converged_),
               fit_cov_params=[float(v) for v in f.params_], fit_cov_se=[float(v) for v in f.standard_errors_])
    t0 = time.perf_counter()
    ParetoNBDFitter().fit(x, tx, T, covariates=Z[:, :1])
    row["fit_cov_s"] = round(time.perf_counter() - t0, 4)
    with GgData(n_spend, m_spend) as d:
        row["gg_n"] = int(d.n)
        row["gg_eval_s"] = round(timed(lambda: d.eval(GG_PARAMS), reps), 6)
    t0 = time.perf_counter()
    g = GammaGammaFitter().fit(n_spend, m_spend, standard_errors=True)
    row.update(gg_fit_se_s=round(time.perf_counter() - t0, 4), gg_fit_n_eval=g.n_eval_, gg_fit_converged=bool(g.converged_),
               gg_fit_params=[float(v) for v in g.params_])
    return row


def c2_comparison(draws, thin, burnin):
    from mcmc_clv_model_amd import ParetoNBDFitter, likelihood_ratio_test
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    df = cdnow("full")
    chains, mcmc = 4, draws * thin
    entries = {}
    for name, covs in (("M1", []), ("M2", ["first_sales_scaled"])):
        with HipSampler(build_problem(df, covs, D=2), mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=42) as s:
            s.run(burnin + mcmc)
            entries["HB " + name] = s.marginal_information_criteria()
    a = (df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float))
    cov = df[["first_sales_scaled"]]
    plain = ParetoNBDFitter().fit(*a)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # recorded below instead
        full = ParetoNBDFitter().fit(*a, covariates=cov, standard_errors=True)
    entries["Pareto/NBD (MLE)"] = plain.information_criteria(*a)
    entries["Pareto/NBD + first_sales_scaled (MLE)"] = full.information_criteria(*a, covariates=cov)
    return dict(workload=f"c2: {len(df)} customers, {chains} chains x {draws} draws (thin {thin}), full sink",
                compare_models=json.loads(A.compare_models(entries).to_json(orient="index")),
                mle_log_likelihood=plain.log_likelihood_, mle_cov_log_likelihood=full.log_likelihood_,
                mle_cov_converged=bool(full.converged_), mle_cov_message=full.message_, mle_cov_grad_norm=full.grad_norm_,
                mle_cov_n_eval=full.n_eval_, covariate_max=float(cov.to_numpy().max()),
                mle_cov_summary=json.loads(full.summary_.to_json(orient="index")),
                likelihood_ratio_test=likelihood_ratio_test(plain, full))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_ext.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain of the c2 comparison")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=2000)
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--only-c2", action="store_true", help="keep the timings of the file at --out, redo the c2 comparison")
    args = ap.parse_args()
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.data import synthetic_cbs
    from tests.helpers import cdnow
    if _lib.device_count() < 1:
        raise SystemExit("profile_mle_ext: no HIP device visible")
    if args.only_c2:
        with open(args.out) as f:
            rec = json.load(f)
        rec["c2"] = c2_comparison(args.draws, args.thin, args.burnin)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec["c2"]))
        return
    df = cdnow("full")
    n_sp = df["x"].to_numpy() + 1
    m_sp = df["sales"].to_numpy() / n_sp
    syn = synthetic_cbs(1_000_000, 2)
    rng = np.random.default_rng(8)
    syn_n = syn["x"].to_numpy() + 1
    syn_m = rng.gamma(6.25 * syn_n, 1.0) / (syn_n * rng.gamma(3.74, 1.0 / 15.44, len(syn)))     # Gamma-Gamma draws
    rec = dict(timing="host wall clock around the synchronous call (launches, the fixed-order final sum and the read-back "
                      "included), median of reps after one warm-up; the fits are one whole fit incl. the upload (the covariate "
                      "fit: the plain fit from params = 1, then the covariate fit from its optimum), with standard errors "
                      "where the key says _se",
               sizes=[one_size("cdnow full CBS", df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy(),
                               n_sp[m_sp > 0], m_sp[m_sp > 0], args.reps),
                      one_size("synthetic_cbs(1,000,000, K=2)", syn["x"].to_numpy(), syn["t_x"].to_numpy(),
                               syn["T_cal"].to_numpy(), syn_n, syn_m, args.reps)])
    if not args.skip_c2:
        rec["c2"] = c2_comparison(args.draws, args.thin, args.burnin)
    elif os.path.exists(args.out):            # keep the comparison the file already holds
        with open(args.out) as f:
            old = json.load(f)
        if "c2" in old:
            rec["c2"] = old["c2"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

"""Time and resources of the two evaluations of the Pareto/NBD integral I (csrc/pnbd.hip):
the series (the default) and the Gauss-Legendre quadrature of I itself (clv_pnbd_set_integral).

  evals      one evaluation at N = 23,570 (the full CDNOW CBS) and N = 1,000,000 (data.synthetic_cbs) in "series",
             "auto" and "quadrature" at NEAR_OPT, and "auto" at the full-CBS covariate optimum (clv_pnbd_eval_cov;
             the synthetic table takes its own covariate column)
  default    the default mode of this library against the parent commit's library (--parent-lib), each timed in
             a child process of its own in this session; the margin is the spread of the parent's own repeats
  switch     the cost of the series and of the quadrature as a function of z(t_x): 65,536 copies of one customer
             at alpha chosen for each z; where the two cross is where PNBD_Z_SWITCH belongs
  resources  VGPRs, AGPRs, scratch and occupancy of every kernel instance from the compiler's resource report
             (--resources compiles csrc/pnbd.hip for gfx950 and needs no device; --parent-source adds the same
             table of another pnbd.hip)
  fit        the whole full-CBS covariate fit in "auto" with standard errors
  c2         the compare_models table of HB M1, HB M2, the plain MLE and the covariate MLE at the wall ("series")
             and converged ("auto")

Each device time is the median of --reps host-timed synchronous calls after one warm-up call.  Sections are
merged into the JSON at --out (default profiles/pnbd_tail.json), so they can be made in separate runs
(--sections).  A record, not a gate.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NEAR_OPT = (0.55, 10.58, 0.61, 11.67)
MODES = ("series", "auto", "quadrature")
SWITCH_Z = (0.1, 0.3, 0.5, 0.7, 0.8, 0.85, 0.9, 0.93, 0.95, 0.97)
SECTIONS = ("evals", "default", "switch", "fit", "c2")


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 6) for t in ts]


def tables():
    from mcmc_clv_model_amd.data import synthetic_cbs
    from tests.helpers import cdnow
    df, syn = cdnow("full"), synthetic_cbs(1_000_000, 2)
    return (("cdnow full CBS", df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float),
             df[["first_sales_scaled"]].to_numpy(float)),
            ("synthetic_cbs(1,000,000, K=2)", syn["x"].to_numpy(), syn["t_x"].to_numpy(float), syn["T_cal"].to_numpy(float),
             syn[["c1"]].to_numpy(float)))


def optimum():
    """The recorded full-CBS covariate optimum (tests/golden/pnbd_tail_exact.npz)."""
    from tests.helpers import golden
    return np.array(golden("pnbd_tail_exact.npz")["fit_params"])


def evals(reps):
    from mcmc_clv_model_amd.mle import PnbdData
    from tests import pnbd_tail_ref as Q
    opt = optimum()
    rows = []
    for name, x, tx, T, z in tables():
        row = dict(workload=name, n=int(len(x)), params=list(NEAR_OPT), optimum=[float(v) for v in opt], reps=reps)
        with PnbdData(x, tx, T, covariates=z) as d:
            for mode in MODES:
                d.set_integral(mode)
                t, every = timed(lambda: d.eval(NEAR_OPT), reps)
                row[f"{mode}_near_opt_s"], row[f"{mode}_near_opt_all_s"] = round(t, 6), every
                row[f"{mode}_near_opt_n_unconverged"] = d.eval(NEAR_OPT)[1]
            for mode in ("series", "auto"):
                d.set_integral(mode)
                t, every = timed(lambda: d.eval_cov(opt), reps)
                sums, nu = d.eval_cov(opt)
                row[f"{mode}_optimum_s"], row[f"{mode}_optimum_all_s"] = round(t, 6), every
                row[f"{mode}_optimum_n_unconverged"], row[f"{mode}_optimum_sum_log_l"] = nu, float(sums[0])
        a, b = opt[1] * np.exp(-opt[4] * z[:, 0]), opt[3] * np.exp(-opt[5] * z[:, 0])
        zz = Q.z_tx(tx, a, b)
        row.update(optimum_n_quadrature=int(Q.takes_quadrature("auto", tx, T, a, b).sum()),
                   optimum_n_z_above_cap=int((zz > 0.98).sum()), optimum_z_max=float(zz.max()))
        rows.append(row)
    return rows


def default_child(reps, lib_path):
    """Timings of the default mode of the library at ``lib_path``, in a child process of its own.  The library is
    bound here, by the few entries the timing needs: the package's binding declares every entry of the header,
    and the parent commit's library has no clv_pnbd_set_integral."""
    import ctypes
    from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p
    L = ctypes.CDLL(lib_path)
    dp = POINTER(c_double)
    for name, res, args in (("clv_pnbd_create", c_int32, [c_int32, c_int64, POINTER(c_int32), dp, dp, dp, POINTER(c_void_p)]),
                            ("clv_pnbd_destroy", None, [c_void_p]),
                            ("clv_pnbd_set_covariates", c_int32, [c_void_p, c_int32, dp, c_int32, dp]),
                            ("clv_pnbd_eval", c_int32, [c_void_p, dp, dp, POINTER(c_int64)]),
                            ("clv_pnbd_eval_cov", c_int32, [c_void_p, dp, dp, POINTER(c_int64)])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args

    def ptr(a):
        return a.ctypes.data_as(dp)

    def ok(rc):
        if rc != 0:
            raise SystemExit(f"{lib_path}: error {rc}")
    out = dict(sizes=[])
    p4, p6 = np.array(NEAR_OPT), np.array(NEAR_OPT + (0.05, -0.02))
    for name, x, tx, T, z in tables():
        x, tx, T = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(tx), np.ascontiguousarray(T)
        zz = np.ascontiguousarray(z.T)
        h, nu = c_void_p(), c_int64(0)
        ok(L.clv_pnbd_create(-1, len(x), x.ctypes.data_as(POINTER(c_int32)), ptr(tx), ptr(T), None, ctypes.byref(h)))
        ok(L.clv_pnbd_set_covariates(h, 1, ptr(zz), 1, ptr(zz)))
        s, sc = np.empty(6), np.empty(8)
        t, every = timed(lambda: ok(L.clv_pnbd_eval(h, ptr(p4), ptr(s), ctypes.byref(nu))), reps)
        tc, every_c = timed(lambda: ok(L.clv_pnbd_eval_cov(h, ptr(p6), ptr(sc), ctypes.byref(nu))), reps)
        L.clv_pnbd_destroy(h)
        out["sizes"].append(dict(workload=name, n=int(len(x)), eval_s=round(t, 6), eval_all_s=every, eval_cov_s=round(tc, 6),
                                 eval_cov_all_s=every_c, sums_hex=[float(v).hex() for v in np.concatenate([s, sc])]))
    print("__DEFAULT__" + json.dumps(out))


def default_against_parent(parent_lib, reps):
    from mcmc_clv_model_amd import _lib

    def child(lib):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--default-child", os.path.abspath(lib or _lib.LIB_PATH),
                            "--reps", str(reps)], capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(f"the timing child failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout[p.stdout.index("__DEFAULT__") + len("__DEFAULT__"):])
    runs = [("parent", child(parent_lib)), ("this", child(None)), ("parent_again", child(parent_lib)),
            ("this_again", child(None))]
    out = dict(order=[k for k, _ in runs], **dict(runs), verdict=[])
    for i, size in enumerate(runs[0][1]["sizes"]):
        for key in ("eval", "eval_cov"):
            par = [r["sizes"][i][key + "_all_s"] for k, r in runs if k.startswith("parent")]
            spread = max(max(v) - min(v) for v in par)
            p_med = float(np.median(np.concatenate(par)))
            t_med = float(np.median(np.concatenate([r["sizes"][i][key + "_all_s"] for k, r in runs if k.startswith("this")])))
            out["verdict"].append(dict(workload=size["workload"], entry=key, parent_median_s=round(p_med, 6),
                                       this_median_s=round(t_med, 6), parent_spread_s=round(spread, 6),
                                       within_parent_spread=bool(t_med - p_med <= spread),
                                       same_bits=runs[0][1]["sizes"][i]["sums_hex"] == runs[1][1]["sizes"][i]["sums_hex"]))
    return out


def switch(reps, n=65_536):
    """One customer (x = 2, t_x = 10, T = 39) n times, the smaller of alpha and beta at 0.5 and the larger chosen
    for each z(t_x) = (larger - smaller) / (larger + t_x), in both orders (alpha > beta: the series carries r + x)."""
    from mcmc_clv_model_amd.mle import PnbdData
    from tests import pnbd_ref as R
    x, tx, T = np.full(n, 2, np.int32), np.full(n, 10.0), np.full(n, 39.0)
    rows = []
    with PnbdData(x, tx, T) as d:
        for z in SWITCH_Z:
            # z (big + t_x) = big - small: at a fixed small offset of 0.5 the big one is (0.5 + z t_x) / (1 - z)
            big = (0.5 + z * 10.0) / (1.0 - z)
            for label, p in (("alpha<beta", (0.55, 0.5, 0.61, big)), ("alpha>beta", (0.55, big, 0.61, 0.5))):
                row = dict(z=z, order=label, params=list(p))
                m = R.model_customers(x[:1], tx[:1], T[:1], p)
                row["series_terms"] = int(m["terms"][0])
                for mode in ("series", "quadrature"):
                    d.set_integral(mode)
                    t, _ = timed(lambda: d.eval(p), reps)
                    row[mode + "_s"] = round(t, 6)
                    row[mode + "_n_unconverged"] = d.eval(p)[1]
                rows.append(row)
    return dict(n=n, customer=dict(x=2, t_x=10.0, T=39.0), rows=rows)


def parse_resources(text):
    out, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(kernel=m.group(1))
            out.append(cur)
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"\bSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def resources(source=None):
    """The compiler's resource report of csrc/pnbd.hip (or ``source``, compiled against this tree's headers)."""
    csrc = os.path.join(ROOT, "mcmc_clv_model_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", csrc,
               "-Rpass-analysis=kernel-resource-usage", "-c", source or os.path.join(csrc, "pnbd.hip"), "-o",
               os.path.join(tmp, "pnbd.o")]
        p = subprocess.run(cmd, capture_output=True, text=True, check=True)
    return parse_resources(p.stderr)


def fit():
    from mcmc_clv_model_amd import ParetoNBDFitter
    from tests.helpers import golden
    _, x, tx, T, z = tables()[0]
    g = golden("pnbd_tail_exact.npz")
    t0 = time.perf_counter()
    f = ParetoNBDFitter(integral="auto").fit(x, tx, T, covariates=z, covariate_names=["first_sales_scaled"],
                                             standard_errors=True)
    t = time.perf_counter() - t0
    return dict(fit_s=round(t, 4), converged=bool(f.converged_), n_eval=f.n_eval_, n_iter=f.n_iter_, grad_norm=f.grad_norm_,
                n_unconverged=f.n_unconverged_, log_likelihood=f.log_likelihood_, params=[float(v) for v in f.params_],
                standard_errors=[float(v) for v in f.standard_errors_], recorded_log_likelihood=float(g["fit_logL"]),
                distance_from_record_in_se=[float(v) for v in np.abs(f.params_.to_numpy() - g["fit_params"]) / g["fit_se"]])


def c2(draws, thin, burnin):
    import warnings
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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # the wall: recorded below instead
        wall = ParetoNBDFitter().fit(*a, covariates=cov)
    full = ParetoNBDFitter(integral="auto").fit(*a, covariates=cov, standard_errors=True)
    entries["Pareto/NBD (MLE)"] = plain.information_criteria(*a)
    entries["Pareto/NBD + first_sales_scaled (MLE, at the series' wall)"] = wall.information_criteria(*a, covariates=cov)
    entries["Pareto/NBD + first_sales_scaled (MLE, converged)"] = full.information_criteria(*a, covariates=cov)
    return dict(workload=f"c2: {len(df)} customers, {chains} chains x {draws} draws (thin {thin}), full sink",
                compare_models=json.loads(A.compare_models(entries).to_json(orient="index")),
                mle_log_likelihood=plain.log_likelihood_, wall_log_likelihood=wall.log_likelihood_,
                wall_converged=bool(wall.converged_), wall_n_eval=wall.n_eval_, converged_log_likelihood=full.log_likelihood_,
                converged=bool(full.converged_), converged_n_eval=full.n_eval_, converged_grad_norm=full.grad_norm_,
                converged_summary=json.loads(full.summary_.to_json(orient="index")),
                likelihood_ratio_test=likelihood_ratio_test(plain, full))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnbd_tail.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sections", default=",".join(SECTIONS), help="comma-separated subset of " + ",".join(SECTIONS))
    ap.add_argument("--parent-lib", help="libclvmcmc.so of the parent commit, for the section 'default'")
    ap.add_argument("--resources", action="store_true", help="compile csrc/pnbd.hip and record its resource report (no device)")
    ap.add_argument("--parent-source", help="with --resources: a pnbd.hip to report beside this one (the parent commit's)")
    ap.add_argument("--draws", type=int, default=1000, help="stored draws per chain of the c2 comparison")
    ap.add_argument("--thin", type=int, default=2)
    ap.add_argument("--burnin", type=int, default=2000)
    ap.add_argument("--default-child", metavar="LIB", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.default_child:
        return default_child(args.reps, args.default_child)
    rec = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["timing"] = ("host wall clock around the synchronous call (launch, the fixed-order final sum and the read-back "
                     "included), median of reps after one warm-up")
    if args.resources:
        rec["resources"] = dict(this=resources())
        if args.parent_source:
            rec["resources"]["parent"] = resources(args.parent_source)
    else:
        from mcmc_clv_model_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("profile_pnbd_tail: no HIP device visible (--resources needs none)")
        want = [s for s in args.sections.split(",") if s]
        for s in want:
            if s not in SECTIONS:
                raise SystemExit(f"unknown section {s!r}")
        if "evals" in want:
            rec["evals"] = evals(args.reps)
        if "default" in want:
            if not args.parent_lib:
                raise SystemExit("the section 'default' needs --parent-lib")
            rec["default"] = default_against_parent(args.parent_lib, args.reps)
        if "switch" in want:
            rec["switch"] = switch(args.reps)
        if "fit" in want:
            rec["fit"] = fit()
        if "c2" in want:
            rec["c2"] = c2(args.draws, args.thin, args.burnin)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "resources"}))


if __name__ == "__main__":
    main()

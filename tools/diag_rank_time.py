"""Time of the rank-normalised diagnostics (csrc/diag.hip, clv_rank_diagnostics_sampler) at the c2
shape: 23,570 CDNOW customers, 4 chains x 1,000 stored draws, full sink — 94,280 level-1 series of
4 x 1,000 draws — next to clv_diagnostics_sampler in the same process, on the same sampler.

Each is the median of --reps host-timed calls (level 1 and level 2) after one warm-up call.  With
--phases it also runs clv_debug_zscale (the sort and rank transform alone, plain and folded) and
both diagnostics on 4,096 synthetic series of the same shape, so that a kernel trace of the run
tells which phase of the kernel dominates.
Writes one JSON object (default profiles/diag_rank_c2.json) and prints it.  A record, not a gate.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_rank_c2.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--phases", action="store_true")
    args = ap.parse_args()
    import bench
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import check, dptr
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df, D, covs, chains, burnin, mcmc, thin, sink = bench.load_workload("c2")
    p = build_problem(df, covs, D)
    L = _lib.lib()
    w = D + 2
    with HipSampler(p, mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=42, draw_sink="full") as s:
        s.run(burnin + mcmc)
        n, n_draws = s.n, s.n_draws
        n2 = D * s.K + D * (D + 1) // 2
        six1, six2 = np.empty((n * w, len(_lib.DIAG_STATS))), np.empty((n2, len(_lib.DIAG_STATS)))
        rk1, rk2 = np.empty((n * w, len(_lib.RANK_STATS))), np.empty((n2, len(_lib.RANK_STATS)))

        def timed(fn):
            fn()  # warm-up
            s.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), ts

        t_diag, all_diag = timed(lambda: check(L.clv_diagnostics_sampler(s.h, 3, dptr(six1), dptr(six2))))
        t_rank, all_rank = timed(lambda: check(L.clv_rank_diagnostics_sampler(s.h, 3, 0.94, dptr(rk1), dptr(rk2))))
        rec = dict(workload=f"c2: {n} customers, {chains} chains x {n_draws} draws, full sink",
                   n_series_level1=int(n * w), reps=args.reps,
                   rank_diagnostics_s=round(t_rank, 6), diagnostics_s=round(t_diag, 6), ratio=round(t_rank / t_diag, 2),
                   rank_diagnostics_all_s=[round(t, 6) for t in all_rank],
                   diagnostics_all_s=[round(t, 6) for t in all_diag],
                   timing="host wall clock around the synchronous *_sampler call, level 1 and level 2 (scratch "
                          "allocation included), median of reps after one warm-up call")
        if args.phases:
            # the sort and rank transform alone (clv_debug_zscale: one sort + one transform, folded: two
            # sorts + one transform) next to both diagnostics, on 4,096 AR(1) series of the same shape
            # through the host-array entries.  Their wall clock includes the upload and the read-back;
            # the kernels' own durations are read from a kernel trace of this run.
            ns = 4096
            rng = np.random.default_rng(3)
            sl = rng.standard_normal((chains, n_draws, ns))
            for i in range(1, n_draws):
                sl[:, i] = 0.5 * sl[:, i - 1] + np.sqrt(0.75) * sl[:, i]
            sl = np.ascontiguousarray(sl)
            S = 2 * chains * (n_draws // 2)
            rk, z = np.empty((ns, S)), np.empty((ns, S))
            out = np.empty((ns, len(_lib.RANK_STATS)))
            six = np.empty((ns, len(_lib.DIAG_STATS)))
            t_z0, _ = timed(lambda: check(L.clv_debug_zscale(-1, dptr(sl), chains, n_draws, ns, 0, dptr(rk), dptr(z))))
            t_z1, _ = timed(lambda: check(L.clv_debug_zscale(-1, dptr(sl), chains, n_draws, ns, 1, dptr(rk), dptr(z))))
            t_r, _ = timed(lambda: check(L.clv_rank_diagnostics(-1, dptr(sl), chains, n_draws, ns, 1, 0, 0.94, dptr(out))))
            t_d, _ = timed(lambda: check(L.clv_diagnostics(-1, dptr(sl), chains, n_draws, ns, 1, 0, dptr(six))))
            rec["phases_slice"] = dict(n_series=ns, zscale_plain_s=round(t_z0, 6), zscale_folded_s=round(t_z1, 6),
                                       rank_diagnostics_s=round(t_r, 6), diagnostics_s=round(t_d, 6),
                                       note="host-array entries on synthetic AR(1) series: upload and read-back "
                                            "included; zscale_plain = one sort + one rank transform, zscale_folded "
                                            "= two sorts + one transform, both writing 2 x 8 S bytes per series")
    a = rk1.reshape(n, w, len(_lib.RANK_STATS))
    names = ["log_lambda", "log_mu", "tau", "z", "eta"][:w]
    for j, nm in enumerate(names):
        for k, st in enumerate(_lib.RANK_STATS):
            if st in ("rhat", "ess_bulk", "ess_tail", "lag_bulk"):
                v = a[:, j, k]
                ok = np.isfinite(v)
                if ok.any():
                    q = np.percentile(v[ok], [0, 50, 99, 100])
                    rec[f"{st}_{nm}"] = dict(nan=int((~ok).sum()), min=float(q[0]), median=float(q[1]), p99=float(q[2]),
                                             max=float(q[3]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

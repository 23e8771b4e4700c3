"""Measurements of scoring customers outside the fit (csrc/score.hip); a record,
not a gate.  Writes one JSON object (default profiles/score_c2.json) and prints it.

On the GPU (default):
  rate   the full CDNOW CBS (23,570 customers) scored against 4 x 1,000 records at R = 1 with the
         summary sink, against 1,000 sweeps of the c2 sampler (4 chains x 23,570, one covariate) in
         the same process on the same card: the same number of customer-sweeps.  Also the full sink
         and R = 5.
  probe  16,384 and 32,768 customers x 4 chains: exactly one and two workgroups on each of 256 CUs
         (one and two waves per SIMD), the two times c2's own grid of 372 workgroups lies between.
  scale  1,000,000 customers (the CBS tiled) x 4 x 1,000 records at R = 1, summary sink.
  c1     posterior mean and sd of the level-2 records of a fit on the Abe subset (2,357 customers):
         the input of the finite-R bias measurement.
Every time is a hipEvent time (the score kernel's: clv_score_info; the sampler's: clv_kernel_time)
after the benchmark's clock-settle phase (bench.settle_clocks with a scratch sampler), median of 5.

--bias (no GPU): the finite-R bias on the float64 model of tests/score_ref.py.  The records of every
chain alternate between (beta, Sigma) = c1 mean - 1.5 sd and + 1.5 sd (elementwise: 3 posterior sd
apart); the first 64 Abe customers are scored with 16 chains x 2,000 records at R = --bias-inner and
the pooled means of log lambda and log mu are set against the average of the two quadratures, in
units of each customer's posterior sd.  Reads the c1 figures from --out and adds the table to it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

REPS = 5
COVS = ["first_sales_scaled"]


def gpu_part(args):
    import bench
    from mcmc_clv_model_amd import _lib, score_customers
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow, cdnow_tiled
    if _lib.device_count() < 1:
        raise SystemExit("profile_score: no HIP device visible")
    chains, nd = 4, args.records
    full = cdnow("full")
    p = build_problem(full, COVS, D=2)
    n = p.N
    rec = dict(timing=f"hipEvent times after bench.settle_clocks({args.settle_ms} ms, scratch sampler), median of {REPS}")

    # ---- the fit whose records are scored: c2 itself (4 chains, nd stored draws)
    with HipSampler(p, mcmc=nd, burnin=500, thin=1, chains=chains, seed=42, draw_sink="summary") as s:
        s.run(500 + nd)
        _, l2, _ = s.read_draws(level1=False)
    draws = {"level_2": list(l2)}
    scratch = bench.scratch_sampler(p, chains, 0)

    def settle():
        return bench.settle_clocks(args.settle_ms, 0, scratch)

    def time_score(cbs, label, **kw):
        score_customers(draws, cbs, COVS, warmup=0, seed=1, **kw)      # warm-up: code object, allocations
        ts, info = [], None
        for _ in range(REPS):
            settle()
            score_customers(draws, cbs, COVS, warmup=0, seed=1, **kw)
            info = _lib.score_info()
            ts.append(info["kernel_ns"] * 1e-9)
        sweeps = len(cbs) * chains * nd * kw.get("inner_sweeps", 1)
        med = float(np.median(ts))
        return dict(label=label, kernel_s=round(med, 6), all_s=[round(t, 6) for t in ts], customer_sweeps=int(sweeps),
                    customer_sweeps_per_s=round(sweeps / med, 1), us_per_inner_sweep=round(med / (nd * kw.get("inner_sweeps", 1)) * 1e6, 3),
                    vgprs=info["vgprs"], scratch_bytes=info["scratch_bytes"])

    # ---- the sampler's own sweeps: the same customer-sweeps, unchanged parent code
    with HipSampler(p, mcmc=1, burnin=10 ** 8, thin=1, chains=chains, seed=42, draw_sink="none") as s:
        s.run(200)
        s.set_timing(True)
        ts = []
        for _ in range(REPS):
            settle()
            k0 = s.kernel_time()
            s.run(nd)
            s.synchronize()
            k1 = s.kernel_time()
            ts.append(((k1["sweep_ms"] - k0["sweep_ms"]) + (k1["hyper_ms"] - k0["hyper_ms"])) * 1e-3)
        info = s.launch_info()
    fit_s = float(np.median(ts))
    rec["sampler"] = dict(label=f"c2 sampler, {nd} sweeps, {chains} chains x {n} customers, no draws kept",
                          kernel_s=round(fit_s, 6), all_s=[round(t, 6) for t in ts], us_per_sweep=round(fit_s / nd * 1e6, 3),
                          customer_sweeps_per_s=round(n * chains * nd / fit_s, 1), persistent=info["persistent"],
                          layout=info["layout"])
    rate = time_score(full, f"{n} customers x {chains} x {nd} records, R = 1, summary sink", inner_sweeps=1, sink="summary")
    rec["rate"] = dict(rate, ratio_to_sampler=round(rate["kernel_s"] / fit_s, 3))
    rec["rate_full_sink"] = time_score(full, "the same, full sink", inner_sweeps=1, sink="full")
    rec["rate_R5"] = time_score(full, "the same, R = 5, summary sink", inner_sweeps=5, sink="summary")
    big = cdnow_tiled(args.scale)
    rec["scale"] = time_score(big, f"{args.scale} customers (CBS tiled) x {chains} x {nd} records, R = 1, summary sink",
                              inner_sweeps=1, sink="summary")
    # one and two workgroups on every CU (256 CUs x 256 lanes x 4 chains): one wave and two waves per SIMD
    for wgs_per_cu in (1, 2):
        m = 16384 * wgs_per_cu
        rec[f"probe_{wgs_per_cu}_workgroups_per_cu"] = time_score(
            cdnow_tiled(m), f"{m} customers x {chains} x {nd} records, R = 1, summary sink: {4 * m // 256} workgroups",
            inner_sweeps=1, sink="summary")
    if scratch is not None:
        scratch.close()

    # ---- c1: the level-2 posterior the bias measurement's two records are taken from
    abe = cdnow("abe")
    p1 = build_problem(abe, COVS, D=2)
    with HipSampler(p1, mcmc=2000, burnin=1000, thin=1, chains=chains, seed=7, draw_sink="summary") as s:
        s.run(3000)
        _, l2a, _ = s.read_draws(level1=False)
    flat = l2a.reshape(-1, l2a.shape[-1])
    rec["c1_level2"] = dict(note="Abe subset (2,357 customers), bivariate with first_sales_scaled, 4 x 2,000 draws after "
                                 "1,000 burn-in; records are beta.T.ravel() then Sigma's upper triangle",
                            mean=[float(v) for v in flat.mean(0)], sd=[float(v) for v in flat.std(0, ddof=1)])
    return rec


def bias_part(rec, chains=16, records=2000, n=64, inners=(1, 2, 5, 7, 8, 9, 10)):
    from tests import philox_sweep_ref as M
    from tests import score_ref as R
    from tests.helpers import cdnow
    mean, sd = np.array(rec["c1_level2"]["mean"]), np.array(rec["c1_level2"]["sd"])
    A, B = mean - 1.5 * sd, mean + 1.5 * sd
    sp = R.ScoreProblem(cdnow("abe", n), COVS, 2)
    for r in (A, B):
        assert np.linalg.eigvalsh(M.l2_unpack(r, 2, 2)[1]).min() > 0
    qa, qb = R.quadrature_means(sp, A), R.quadrature_means(sp, B)
    target = 0.5 * (qa[:, :2] + qb[:, :2])
    unit = 0.5 * (qa[:, 3:] + qb[:, 3:])
    sep = np.abs(qa[:, :2] - qb[:, :2]) / unit
    rows = np.tile(np.arange(n), chains)
    S, W, seed = 20, 50, 20250102
    table = []
    for inner in inners:
        unpacked = [M.l2_unpack(r, 2, 2) for r in (A, B)]
        lam0, mu0 = R.default_init(np.broadcast_to(A, (chains, 1, A.shape[0])), sp.X, 2, 2)
        lam, mu = lam0.ravel(), mu0.ravel()
        total = W + inner * records
        acc = np.zeros((2, chains * n))
        cache, t = {}, 1
        for d in range(-1, records):
            beta, Sigma = unpacked[max(d, 0) % 2]
            for _ in range(W if d < 0 else inner):
                if t not in cache:
                    cache.clear()
                    ts = np.arange(t, min(t + 64, total + 1))
                    parts = [R._variates_block(seed, c, ts, np.arange(n), S) for c in range(chains)]
                    for j, tt in enumerate(ts):
                        cache[int(tt)] = {k: np.concatenate([q[k][j] for q in parts], axis=-1) for k in parts[0]}
                r = sp.level1(lam, mu, beta, Sigma, cache[t], rows=rows)
                lam, mu = r["lam"], r["mu"]
                t += 1
            if d >= 0:
                acc[0] += r["ll"]
                acc[1] += r["lm"]
        got = (acc / records).reshape(2, chains, n).mean(axis=1).T          # [n][2]
        gap = np.abs(got - target) / unit
        table.append(dict(R=inner, worst_gap_sd=round(float(gap.max()), 4), mean_gap_sd=round(float(gap.mean()), 4),
                          worst_gap_log_lambda_sd=round(float(gap[:, 0].max()), 4),
                          worst_gap_log_mu_sd=round(float(gap[:, 1].max()), 4)))
        print(json.dumps(table[-1]), flush=True)
    rec["finite_R_bias"] = dict(
        note=f"float64 model (tests/score_ref.py), first {n} Abe customers, {chains} chains x {records} records alternating "
             "between the c1 level-2 mean - 1.5 sd and + 1.5 sd (elementwise), warm-up 50, 20 MH steps; gap = |pooled mean - "
             "average of the two quadratures| in units of the customer's posterior sd (mean of the two records'); the "
             "Monte Carlo error of a pooled mean is about 0.01 sd",
        separation_of_the_two_targets_sd=dict(worst=round(float(sep.max()), 3), mean=round(float(sep.mean()), 3)),
        table=table)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_c2.json"))
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--scale", type=int, default=1_000_000)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    ap.add_argument("--bias", action="store_true", help="the finite-R bias table on the CPU model (reads and extends --out)")
    ap.add_argument("--bias-inner", default="1,2,5,7,8,9,10", help="the inner_sweeps values of the bias table")
    args = ap.parse_args()
    if args.bias:
        with open(args.out) as f:
            rec = bias_part(json.load(f), inners=tuple(int(v) for v in args.bias_inner.split(",")))
    else:
        rec = gpu_part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

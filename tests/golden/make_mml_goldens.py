#!/usr/bin/env python3
"""Writes tests/golden/mml_exact.npz: the posterior moments of a customer's (log lambda, log mu) under one
level-2 record, and the log of the marginal likelihood, to (far beyond) double precision, for the cells
tests/test_mml_cpu.py holds the float64 model tests/mml_ref.py to.

    python tests/golden/make_mml_goldens.py [processes]
    python tests/golden/make_mml_goldens.py fit          (tests/golden/mml_fit.npz: see fit_main)

The integrals themselves, not the Gauss-Hermite rule under test: the composite Gauss-Legendre rule of
tests/golden/make_marginal_goldens.py (its nodes, its panel bound, 40-digit mpmath), with seven sums per
component instead of one: the integrand times 1, da, db, da^2, da db, db^2 ((da, db) = theta - m_i) and,
in the alive component, times e^(a - b) (1 - exp(-e^b t*)).  Every cell is integrated with panels of
width 1 and of width 1/2; the largest relative difference between the two is stored (``panel_gap``) and
asserted to be below GAP.

Cells: K = 2, the records ``marginal_ref.case_records(4, 2, 2, 41)`` against ten customers of
``marginal_ref.case_customers(600, 2, 17)`` — six edge archetypes (rows 0, 10, ..., 50) and four CDNOW
rows: 40 cells, columns as ``clv_mml_customers`` writes them (l, P(alive), E[da], E[db], E[da^2],
E[da db], E[db^2], E[X*(t*)]).

For the first IDENTITY_CELLS customers of record 0, l is also integrated at the record moved by +-h and
+-h/2 in each of (m_0, m_1, Sigma_00, Sigma_01, Sigma_11) (``shift_l`` [cell][parameter][4]: +h, -h,
+h/2, -h/2; ``shift_h``): the central differences Fisher's identity is checked against.
"""
from __future__ import annotations

import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from tests import marginal_ref as M  # noqa: E402
import make_marginal_goldens as G  # noqa: E402

K = 2
T_STAR = 39.0
ROWS = (0, 10, 20, 30, 40, 50, 1, 2, 3, 7)
N_REC = 4
IDENTITY_CELLS = 3
SHIFT_H = 2.0 ** -6
GAP = 1e-10
WIDTHS = (1.0, 0.5)
NQ = 7    # 1, da, db, da^2, da db, db^2, e^(a - b) (1 - exp(-e^b t*))


def component_sums(mp, gl, width, comp64, q, c, xa, xb, t, m0, m1, centre, t_star):
    """(H0, [NQ sums]) of one component: integral of exp(h - H0) f over theta, f the NQ factors."""
    a0, b0, L00, L10, L11 = (float(v) for v in centre[6 * q:6 * q + 5])
    A0, B0, l00, l10, l11 = (mp.mpf(v) for v in (a0, b0, L00, L10, L11))
    h0 = float(comp64.h(np.array([a0]), np.array([b0]))[0])
    H0 = M.mp_h(mp, c, xa, xb, t, m0, m1, mp.mpf(0), False, A0, B0)
    npan = int(round(2 * G.Z_MAX / width))
    mid = (np.arange(npan) + 0.5) * width - G.Z_MAX
    z1, z2 = (v.ravel() for v in np.meshgrid(mid, mid, indexing="ij"))
    one = np.ones_like(z1)
    pc = M.Component(comp64.c, comp64.xa * one, comp64.xb, comp64.t * one, comp64.m0 * one, comp64.m1 * one,
                     comp64.r0 * one, comp64.spend)
    hw = 0.5 * width
    bound = np.full(z1.shape, np.inf)
    for d1, d2 in ((0.0, 0.0), (-hw, -hw), (-hw, hw), (hw, -hw), (hw, hw)):
        p1, p2 = z1 + d1, z2 + d2
        a, b = a0 + L00 * p1, b0 + L10 * p1 + L11 * p2
        with np.errstate(all="ignore"):
            hp = pc.h(a, b)
            ga, gb = pc.derivs(a, b)[:2]
        g1, g2 = ga * L00 + gb * L10, gb * L11
        top = hp + np.maximum(g1 * (-hw - d1), g1 * (hw - d1)) + np.maximum(g2 * (-hw - d2), g2 * (hw - d2))
        bound = np.where(np.isnan(top), bound, np.minimum(bound, top))
    kept = (~(bound < h0 - G.DROP)).reshape(npan, npan)
    assert not kept[[0, -1], :].any() and not kept[:, [0, -1]].any(), "the integrand reaches the edge of the box"
    xs, ws = gl
    half = mp.mpf(width) / 2
    tot = [mp.mpf(0)] * NQ
    ts = mp.mpf(float(t_star))
    for i in range(npan):
        cols = np.nonzero(kept[i])[0]
        if not len(cols):
            continue
        for x1, w1 in zip(xs, ws):
            zz1 = mp.mpf(float(mid[i])) + half * x1
            av = A0 + l00 * zz1
            bb = B0 + l10 * zz1
            da = av - m0
            acc = [mp.mpf(0)] * NQ
            for j in cols:
                zc = mp.mpf(float(mid[j]))
                for x2, w2 in zip(xs, ws):
                    bv = bb + l11 * (zc + half * x2)
                    db = bv - m1
                    e = w2 * mp.exp(M.mp_h(mp, c, xa, xb, t, m0, m1, mp.mpf(0), False, av, bv) - H0)
                    acc[0] += e
                    acc[1] += e * da
                    acc[2] += e * db
                    acc[3] += e * da * da
                    acc[4] += e * da * db
                    acc[5] += e * db * db
                    if q == 1:
                        acc[6] += e * mp.exp(av - bv) * (-mp.expm1(-mp.exp(bv) * ts))
            for k in range(NQ):
                tot[k] += w1 * acc[k]
    fac = half * half * l00 * l11
    return H0, [v * fac for v in tot]


def cell(job):
    """(row [8], gap) of one (record, customer): l, P(alive), five moments, E[X*(t*)]."""
    import mpmath as mp
    mp.mp.dps = 40
    rec, covi, x, t_x, T_cal, t_star = job
    gl = G.gauss_legendre(mp, G.PANEL_NODES)
    c = M.mp_constants(mp, rec, 2, K, False, 1.0)
    cov1 = np.asarray(covi, dtype=np.float64).reshape(K - 1, 1)
    comps, m0, m1, _ = M.mp_customer(mp, rec, 2, K, cov1, 0, [x], [t_x], [T_cal], None)
    comps64 = M.components(rec, 2, K, cov1, [x], [t_x], [T_cal])
    _, cen = M.marginal_loglik(np.asarray(rec)[None], 2, K, cov1, [x], [t_x], [T_cal])
    rows = []
    for width in WIDTHS:
        try:
            parts = [component_sums(mp, gl, width, comps64[q], q, c, xa, xb, t, m0, m1, cen[0, 0], t_star)
                     for q, (xa, xb, t) in enumerate(comps)]
        except AssertionError as e:
            return None, str(e)
        H = max(p[0] for p in parts)
        sc = [mp.exp(p[0] - H) for p in parts]
        Z = sum(s * p[1][0] for s, p in zip(sc, parts))
        row = [H + mp.log(Z), sc[1] * parts[1][1][0] / Z]
        row += [sum(s * p[1][k] for s, p in zip(sc, parts)) / Z for k in range(1, 6)]
        row.append(sc[1] * parts[1][1][6] / Z)
        rows.append(row)
    a, b = rows
    scale = [max(1, abs(b[0])), 1, mp.sqrt(b[4]), mp.sqrt(b[6]), b[4], mp.sqrt(b[4] * b[6]), b[6], abs(b[7])]
    gap = max(float(abs(u - v) / s) for u, v, s in zip(a, b, scale))
    return [float(v) for v in b], gap


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    recs = M.case_records(N_REC, 2, K, 41)
    df, names = M.case_customers(600, K, 17)
    cov, x, t_x, T_cal, _ = M.case_arrays(df, names, False)
    rows = np.array(ROWS)
    jobs = [(recs[r], cov[:, i], int(x[i]), float(t_x[i]), float(T_cal[i]), T_STAR) for r in range(N_REC) for i in rows]
    n_main = len(jobs)
    for i in rows[:IDENTITY_CELLS]:
        for p in (0, K, 2 * K, 2 * K + 1, 2 * K + 2):
            for h in (SHIFT_H, -SHIFT_H, 0.5 * SHIFT_H, -0.5 * SHIFT_H):
                rec = recs[0].copy()
                rec[p] += h
                jobs.append((rec, cov[:, i], int(x[i]), float(t_x[i]), float(T_cal[i]), T_STAR))
    with multiprocessing.Pool(procs) as pool:
        res = []
        for k, r in enumerate(pool.imap(cell, jobs, chunksize=1)):
            res.append(r)
            print(f"cell {k + 1} of {len(jobs)}: gap {r[1]}", file=sys.stderr, flush=True)
    failed = [(k, g) for k, (v, g) in enumerate(res) if v is None]
    assert not failed, f"cells not integrated: {failed}"
    worst = max(g for _, g in res)
    assert worst < GAP, f"halving the panels moves a value by {worst:.3g}"
    exact = np.array([v for v, _ in res[:n_main]]).reshape(N_REC, len(rows), 8)
    shift = np.array([v[0] for v, _ in res[n_main:]]).reshape(IDENTITY_CELLS, 5, 4)
    np.savez(os.path.join(HERE, "mml_exact.npz"), exact=exact, level2=recs, rows=rows, cov=cov[:, rows], x=x[rows],
             t_x=t_x[rows], T_cal=T_cal[rows], t_star=np.float64(T_STAR), shift_l=shift, shift_h=np.float64(SHIFT_H),
             panel_gap=np.float64(worst))
    print(f"mml_exact.npz: {n_main} cells and {len(jobs) - n_main} shifted ones, the two panel widths agree to {worst:.3g}")


def fit_main():
    """tests/golden/mml_fit.npz: the float64 model tests/mml_ref.py fitted to the ``abe`` CBS (K = 1 and
    K = 2 with first_sales_scaled) and to the first FULL_ROWS rows of the full CBS (K = 2) by
    mle.minimize_bfgs_score from the default start: theta-hat, log L, max |score|, evaluations."""
    from mcmc_clv_model_amd import mle
    from tests import mml_ref as R
    from tests.helpers import cdnow
    out = {}
    for name, frame, K in (("abe_k1", cdnow("abe"), 1), ("abe_k2", cdnow("abe"), 2),
                           ("full_k2", cdnow("full", FULL_ROWS), 2)):
        x, t_x, T_cal = frame["x"].to_numpy(), frame["t_x"].to_numpy(float), frame["T_cal"].to_numpy(float)
        cov = np.ascontiguousarray(frame[["first_sales_scaled"]].to_numpy(float).T) if K > 1 else None
        res = mle.minimize_bfgs_score(R.objective(K, cov, x, t_x, T_cal), R.default_start(K, x, t_x, T_cal), 1e-7, 200)
        assert res.converged, (name, res.message, res.grad_norm)
        out[name + "_theta"], out[name + "_loglik"] = res.x, np.float64(-res.fun)
        out[name + "_score"], out[name + "_n_eval"] = np.float64(res.grad_norm), np.int64(res.n_eval)
        print(f"{name}: log L {-res.fun:.6f}, max |score| {res.grad_norm:.3g}, {res.n_eval} evaluations, "
              f"record {R.record_of(res.x, K)}", flush=True)
    np.savez(os.path.join(HERE, "mml_fit.npz"), full_rows=np.int64(FULL_ROWS), **out)


FULL_ROWS = 4096

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "fit":
        fit_main()
    else:
        main()

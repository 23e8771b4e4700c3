#!/usr/bin/env python3
"""Writes tests/golden/marginal_exact.npz: the marginal likelihood of DESIGN.md section 4k to (far
beyond) double precision, for the customers and level-2 records tests/test_marginal_cpu.py and
tests/test_gpu_marginal.py hold the quadrature to.

    python tests/golden/make_marginal_goldens.py [processes]

The integral itself, not the quadrature rule under test: per log-concave component (dropped out, alive;
tests/marginal_ref.py) a composite Gauss-Legendre rule (PANEL_NODES nodes per panel and dimension) in
mpmath at 40 digits over z in [-Z_MAX, Z_MAX]^2, theta = centre + L z with the float64 model's centre
and scale (any nearby centre gives the same integral).  A panel is left out only where a tangent
plane of h — an upper bound of a concave h everywhere; the lowest of those at the panel's middle and
four corners — stays below h(centre) - DROP on the whole panel (the bound is evaluated in float64; e^-DROP times the number of panels is below 1e-17 of
the integral).  Every cell is integrated with panels of width 1 and of width 1/2, and with halved panels again
(down to 1/8) while the last halving still moved the logarithm by 1e-15; the script asserts that the
last two agree to 1e-14, and the finest is stored.

Cases (all stored in the one file, keys prefixed by the case name):
    bi_k1    D = 2, K = 1: the edge customers (x = 0; t_x = T; t_x just under T; t_x << T; x = 40, 2,000
             and 20,000 on weekly and daily clocks) and CDNOW-like ones, against CDNOW-like records (chain
             medians of a c1-size oracle fit, tests/golden/envelope_c1_bi_k1.npz, one of them with both
             variances halved and rho = -0.4) and wide ones (Sigma_11 = 3, Sigma_22 = 6, rho = -0.24);
             ``bi_k1_family`` marks the records 0 = CDNOW-like, 1 = wide
    tri_k3   D = 3, K = 3 (chain medians of tests/golden/envelope_abe_tri_k3.npz): ``tri_k3_exact`` with
             the spend term, ``tri_k3_exact_tx`` without it (the leading block alone)
"""
from __future__ import annotations

import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import marginal_ref as M  # noqa: E402

PANEL_NODES = 10
Z_MAX = 100
DROP = 50.0
AGREE = 1e-14

BI_CUSTOMERS = [  # (x, t_x, T_cal)
    (0, 0.0, 39.0), (1, 39.0, 39.0), (1, 39.0 * (1.0 - 2.0 ** -40), 39.0), (1, 39.0e-9, 39.0), (3, 19.5, 39.0),
    (40, 2.0, 39.0), (40, 38.9, 39.0), (2000, 3649.0, 3650.0), (2000, 20.0, 39.0), (20000, 3649.0, 3650.0),
    (20000, 38.9, 39.0), (0, 0.0, 3650.0), (1, 3650.0, 3650.0), (0, 0.0, 0.01), (2, 30.43, 38.86),
    (1, 1.71, 38.86), (7, 29.43, 38.86), (0, 0.0, 27.0), (12, 35.2, 37.3), (5, 10.0, 39.0)]
TRI_CUSTOMERS = [  # (x, t_x, T_cal, log_s, c1, c2)
    (0, 0.0, 39.0, 0.0, 1.0, -0.3), (2, 30.0, 39.0, 3.2, 0.0, 0.8), (1, 39.0, 39.0, -12.0, 1.0, 0.1),
    (40, 2.0, 39.0, 14.0, 0.0, -1.0), (2000, 3649.0, 3650.0, 3.0, 1.0, 0.5), (7, 29.4, 38.9, 4.1, 0.0, 0.0)]
TRI_OMEGA2 = 0.8


def bi_records():
    med = np.load(os.path.join(HERE, "envelope_c1_bi_k1.npz"))["level2_median"]
    recs = [med[0], med[5], med[9]]
    tight = med[2].copy()
    tight[2], tight[4] = 0.5 * tight[2], 0.5 * tight[4]
    tight[3] = -0.4 * np.sqrt(tight[2] * tight[4])
    recs.append(tight)
    for b0, b1 in ((-3.5, -3.7), (-1.0, -6.0)):
        recs.append(np.array([b0, b1, 3.0, -0.24 * np.sqrt(18.0), 6.0]))
    return np.array(recs), np.array([0, 0, 0, 0, 1, 1])


def tri_records():
    return np.load(os.path.join(HERE, "envelope_abe_tri_k3.npz"))["level2_median"][:2].copy()


def gauss_legendre(mp, n):
    """The n-point rule on [-1, 1] at the working precision."""
    xs, ws = [], []
    for x0 in np.polynomial.legendre.leggauss(n)[0]:
        x = mp.mpf(float(x0))
        for _ in range(8):
            p0, p1 = mp.mpf(1), x
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            x = x - p1 / dp
        p0, p1 = mp.mpf(1), x
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        xs.append(x)
        ws.append(2 / ((1 - x * x) * dp * dp))
    return xs, ws


def component_integral(mp, gl, width, comp64, q, c, xa, xb, t, m0, m1, r0, spend, centre):
    """log of one component's integral with panels of ``width``; comp64: the float64 component of this
    one customer (for the panel bound), q its index in the centre row."""
    a0, b0, L00, L10, L11 = (float(v) for v in centre[6 * q:6 * q + 5])
    A0, B0, l00, l10, l11 = (mp.mpf(v) for v in (a0, b0, L00, L10, L11))
    h0 = float(comp64.h(np.array([a0]), np.array([b0]))[0])
    H0 = M.mp_h(mp, c, xa, xb, t, m0, m1, r0, spend, A0, B0)
    npan = int(round(2 * Z_MAX / width))
    mid = (np.arange(npan) + 0.5) * width - Z_MAX
    z1, z2 = (v.ravel() for v in np.meshgrid(mid, mid, indexing="ij"))
    one = np.ones_like(z1)
    pc = M.Component(comp64.c, comp64.xa * one, comp64.xb, comp64.t * one, comp64.m0 * one, comp64.m1 * one,
                     comp64.r0 * one, comp64.spend)
    hw = 0.5 * width
    bound = np.full(z1.shape, np.inf)
    for d1, d2 in ((0.0, 0.0), (-hw, -hw), (-hw, hw), (hw, -hw), (hw, hw)):   # the middle and the four corners
        p1, p2 = z1 + d1, z2 + d2
        a, b = a0 + L00 * p1, b0 + L10 * p1 + L11 * p2
        with np.errstate(all="ignore"):
            hp = pc.h(a, b)
            ga, gb = pc.derivs(a, b)[:2]
        g1, g2 = ga * L00 + gb * L10, gb * L11        # dh/dz at the anchor
        # the tangent plane's maximum over the panel [z - hw, z + hw]^2
        top = hp + np.maximum(g1 * (-hw - d1), g1 * (hw - d1)) + np.maximum(g2 * (-hw - d2), g2 * (hw - d2))
        bound = np.where(np.isnan(top), bound, np.minimum(bound, top))
    keep = ~(bound < h0 - DROP)
    assert not keep.reshape(npan, npan)[[0, -1], :].any() and not keep.reshape(npan, npan)[:, [0, -1]].any(), \
        "the integrand reaches the edge of the box"
    xs, ws = gl
    half = mp.mpf(width) / 2
    total = mp.mpf(0)
    kept = keep.reshape(npan, npan)
    for i in range(npan):
        cols = np.nonzero(kept[i])[0]
        if not len(cols):
            continue
        for x1, w1 in zip(xs, ws):
            zz1 = mp.mpf(float(mid[i])) + half * x1
            av = A0 + l00 * zz1
            bb = B0 + l10 * zz1
            acc = mp.mpf(0)
            for j in cols:
                zc = mp.mpf(float(mid[j]))
                for x2, w2 in zip(xs, ws):
                    bv = bb + l11 * (zc + half * x2)
                    acc += w2 * mp.exp(M.mp_h(mp, c, xa, xb, t, m0, m1, r0, spend, av, bv) - H0)
            total += w1 * acc
    return H0 + mp.log(total * half * half * l00 * l11)


def cell(job):
    """log of the marginal likelihood of one (record, customer) at 40 digits, and the two widths' gap."""
    import mpmath as mp
    mp.mp.dps = 40
    rec, D, K, cov, x, t_x, T_cal, log_s, omega2, centre = job
    spend = log_s is not None
    gl = gauss_legendre(mp, PANEL_NODES)
    c = M.mp_constants(mp, rec, D, K, spend, omega2)
    cov1 = None if cov is None else np.asarray(cov, dtype=np.float64).reshape(K - 1, 1)
    comps, m0, m1, r0 = M.mp_customer(mp, rec, D, K, cov1, 0, [x], [t_x], [T_cal], None if not spend else [log_s])
    comps64 = M.components(rec, D, K, cov1, [x], [t_x], [T_cal], [log_s] if spend else None, omega2)
    vals = []
    for width in (1.0, 0.5, 0.25, 0.125):
        try:
            parts = [component_integral(mp, gl, width, comps64[q], q, c, xa, xb, t, m0, m1, r0, spend, centre)
                     for q, (xa, xb, t) in enumerate(comps)]
        except AssertionError as e:  # reported by main with the cell's number
            return float("nan"), str(e)
        hi = max(parts)
        vals.append(hi + mp.log(sum(mp.exp(p - hi) for p in parts)))
        if len(vals) > 1 and abs(vals[-1] - vals[-2]) < AGREE / 10:   # halve the panels until it changes nothing
            break
    return float(vals[-1]), float(abs(vals[-1] - vals[-2]))


def case_jobs(level2, D, K, cov, x, t_x, T_cal, log_s, omega2):
    _, cen = M.marginal_loglik(level2, D, K, cov, x, t_x, T_cal, log_s, omega2)
    jobs = []
    for r in range(level2.shape[0]):
        for i in range(len(x)):
            jobs.append((level2[r], D, K, None if cov is None else cov[:, i], x[i], t_x[i], T_cal[i],
                         None if log_s is None else log_s[i], omega2, cen[r, i]))
    return jobs


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    out = {}
    bx = np.array([c[0] for c in BI_CUSTOMERS], dtype=np.int32)
    btx, bT = (np.array([c[k] for c in BI_CUSTOMERS], dtype=np.float64) for k in (1, 2))
    brec, fam = bi_records()
    tx_ = np.array([c[0] for c in TRI_CUSTOMERS], dtype=np.int32)
    ttx, tT, tls = (np.array([c[k] for c in TRI_CUSTOMERS], dtype=np.float64) for k in (1, 2, 3))
    tcov = np.array([[c[4] for c in TRI_CUSTOMERS], [c[5] for c in TRI_CUSTOMERS]], dtype=np.float64)
    trec = tri_records()
    sets = [("bi_k1_exact", case_jobs(brec, 2, 1, None, bx, btx, bT, None, 1.0), (len(brec), len(bx))),
            ("tri_k3_exact", case_jobs(trec, 3, 3, tcov, tx_, ttx, tT, tls, TRI_OMEGA2), (len(trec), len(tx_))),
            ("tri_k3_exact_tx", case_jobs(trec, 3, 3, tcov, tx_, ttx, tT, None, 1.0), (len(trec), len(tx_)))]
    with multiprocessing.Pool(procs) as pool:
        res = pool.map(cell, [j for _, jobs, _ in sets for j in jobs], chunksize=1)
    failed = [(k, g) for k, (_, g) in enumerate(res) if isinstance(g, str)]
    assert not failed, f"cells not integrated: {failed}"
    at, worst = 0, 0.0
    for name, jobs, shape in sets:
        part = res[at:at + len(jobs)]
        at += len(jobs)
        out[name] = np.array([v for v, _ in part]).reshape(shape)
        worst = max(worst, max(g for _, g in part))
    assert worst < AGREE, f"doubling the panels moves a value by {worst:.3g}"
    out.update(bi_k1_level2=brec, bi_k1_family=fam, bi_k1_x=bx, bi_k1_t_x=btx, bi_k1_T_cal=bT,
               tri_k3_level2=trec, tri_k3_x=tx_, tri_k3_t_x=ttx, tri_k3_T_cal=tT, tri_k3_log_s=tls,
               tri_k3_cov=tcov, tri_k3_omega2=np.float64(TRI_OMEGA2), panel_gap=np.float64(worst))
    np.savez(os.path.join(HERE, "marginal_exact.npz"), **out)
    print(f"marginal_exact.npz: {at} cells, the two panel widths agree to {worst:.3g}")


if __name__ == "__main__":
    main()

"""Float64 model of csrc/mml.hip — TEST INFRASTRUCTURE ONLY, plain numpy: the
posterior moments of a customer's (log lambda, log mu) under one level-2 record from the quadrature
of tests/marginal_ref.py, the mixing of the two components, the sums in the device's tree order and
the host algebra from the sums to the score of theta = (beta, log-Cholesky of Sigma).

Every operation is written in the order csrc/marginal_core.h and csrc/mml.hip have it.
"""
from __future__ import annotations

import numpy as np

from tests import marginal_ref as M
from tests.pnbd_ref import device_sum

ROW = 8          # l, P(alive), E[da], E[db], E[da da], E[da db], E[db db], E[X*(t*)]
BASE = 6         # sum w l, sum w, non-finite customers, sum w S (00, 01, 11)
SQRT2 = M.SQRT2


def component_moments(comp, tab, centre, t_star=None):
    """(log of the component's integral, mo [6][n]): marginal_ref.Component.integral with the five
    sums of the standardised coordinates next to s (and, ``t_star`` given, of g = e^(a - b)
    (1 - exp(-e^b t_star))), mapped to the component's E[da], E[db], E[da da], E[da db], E[db db], E[g]."""
    t, _, cw = tab
    a0, b0, L00, L10, L11 = centre[:5]
    m = np.full(a0.shape, -np.inf)
    s = np.zeros(a0.shape)
    su, sw, suu, suw, sww, sg = (np.zeros(a0.shape) for _ in range(6))
    for j in range(len(t)):
        tj = t[j]
        a = a0 + SQRT2 * (L00 * tj)
        lam = np.exp(a)
        for k in range(len(t)):
            wk = L10 * tj + L11 * t[k]
            b = b0 + SQRT2 * wk
            v = (cw[j] + cw[k]) + comp.h(a, b, lam)
            up = v > m
            e = np.exp(np.where(up, m - v, v - m))
            s = np.where(up, s * e + 1.0, s + e)
            su = np.where(up, su * e + tj, su + e * tj)
            sw = np.where(up, sw * e + wk, sw + e * wk)
            suu = np.where(up, suu * e + tj * tj, suu + e * (tj * tj))
            suw = np.where(up, suw * e + tj * wk, suw + e * (tj * wk))
            sww = np.where(up, sww * e + wk * wk, sww + e * (wk * wk))
            if t_star is not None:
                mu = np.exp(b)
                y = mu * t_star
                g = np.where(y > 0.0, (lam / mu) * -np.expm1(-y), lam * t_star)
                sg = np.where(up, sg * e + g, sg + e * g)
            m = np.where(up, v, m)
    U, W, UU, UW, WW = su / s, sw / s, suu / s, suw / s, sww / s
    ca, cb, k0 = a0 - comp.m0, b0 - comp.m1, SQRT2 * L00
    mo = [ca + k0 * U,
          cb + SQRT2 * W,
          (ca * ca + 2.0 * (ca * k0) * U) + (k0 * k0) * UU,
          ((ca * cb + (ca * SQRT2) * W) + (cb * k0) * U) + (k0 * SQRT2) * UW,
          (cb * cb + 2.0 * (cb * SQRT2) * W) + 2.0 * WW,
          sg / s if t_star is not None else np.zeros(a0.shape)]
    return np.log(2.0 * (L00 * L11)) + (m + np.log(s)), np.stack(mo)


def customers(record, K, cov, x, t_x, T_cal, nodes=M.DEFAULT_ORDER, t_star=0.0, centres=None, tables=None):
    """rows [n][8] as clv_mml_customers writes them; ``centres`` [n][12] given: the rule applied there
    (the device's own centres) instead of at the model's."""
    record = np.asarray(record, dtype=np.float64)
    tab = (tables or M.gh_tables())[nodes]
    with np.errstate(all="ignore"):
        comps = M.components(record, 2, K, cov, x, t_x, T_cal)
        parts = []
        for q, comp in enumerate(comps):
            ce = comp.centre() if centres is None else tuple(centres[:, 6 * q + p] for p in range(6))
            parts.append(component_moments(comp, tab, ce, float(t_star) if q == 1 else None))
        (iD, mD), (iA, mA) = parts
        hi, lo = np.maximum(iD, iA), np.minimum(iD, iA)
        l = hi + np.log1p(np.exp(lo - hi))
        wD, wA = np.exp(iD - l), np.exp(iA - l)
        rows = np.empty((len(l), ROW))
        rows[:, 0] = l
        rows[:, 1] = wA
        for k in range(5):
            rows[:, 2 + k] = wD * mD[k] + wA * mA[k]
        rows[:, 7] = wA * mA[5]
        rows[~(np.isfinite(iD) & np.isfinite(iA))] = np.nan
    return rows


def sums_of_rows(rows, K, cov, w=None):
    """(sums [2K + 6], n_nonfinite): the device's fixed-order sums of per-customer rows."""
    n = rows.shape[0]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        cols = [w * rows[:, 0], w, (~np.isfinite(rows[:, 0])).astype(np.float64), w * rows[:, 4], w * rows[:, 5],
                w * rows[:, 6]]
        for col in (2, 3):
            for k in range(K):
                d = np.ones(n) if k == 0 else cov[k - 1]
                cols.append((w * d) * rows[:, col])
        s = np.array([device_sum(c) for c in cols])
    return s, int(s[2])


def sigma_of(c):
    """(Sigma_00, Sigma_01, Sigma_11) of the log-Cholesky parameters c: Sigma = C C', C = [[e^c0, 0], [c1, e^c2]]."""
    e0, e2 = np.exp(c[0]), np.exp(c[2])
    return np.array([e0 * e0, e0 * c[1], c[1] * c[1] + e2 * e2])


def record_of(theta, K):
    """The level-2 record (beta [2][K], Sigma's triangle) of theta = (beta, c0, c1, c2)."""
    theta = np.asarray(theta, dtype=np.float64)
    return np.concatenate([theta[:2 * K], sigma_of(theta[2 * K:])])


def score_of_sums(sums, theta, K):
    """d sum w l / d theta from the 2K + 6 sums: d / d m = P E[(da, db)], d / d Sigma = P (S - W Sigma) P / 2,
    then the chain rule through Sigma = C C' (written with explicit 2 x 2 entries)."""
    theta = np.asarray(theta, dtype=np.float64)
    c = theta[2 * K:]
    s00, s01, s11 = sigma_of(c)
    det = s00 * s11 - s01 * s01
    P = np.array([[s11, -s01], [-s01, s00]]) / det
    W = sums[1]
    R = np.array([[sums[3] - W * s00, sums[4] - W * s01], [sums[4] - W * s01, sums[5] - W * s11]])
    G = 0.5 * (P @ R @ P)                              # d / d Sigma, the off-diagonal entry counted once per side
    C = np.array([[np.exp(c[0]), 0.0], [c[1], np.exp(c[2])]])
    GC = 2.0 * (G @ C)                                 # d / d C
    g = np.empty(2 * K + 3)
    for k in range(K):
        g[k], g[K + k] = P @ np.array([sums[BASE + k], sums[BASE + K + k]])
    g[2 * K:] = [GC[0, 0] * C[0, 0], GC[1, 0], GC[1, 1] * C[1, 1]]
    return g


def objective(K, cov, x, t_x, T_cal, w=None, nodes=M.DEFAULT_ORDER):
    """theta -> (-sum w l, -score) of the float64 model: what mle.minimize_bfgs_score takes."""
    tables = M.gh_tables()

    def f(theta):
        rows = customers(record_of(theta, K), K, cov, x, t_x, T_cal, nodes, tables=tables)
        sums, _ = sums_of_rows(rows, K, cov, w)
        return -sums[0], -score_of_sums(sums, theta, K)
    return f


def default_start(K, x, t_x, T_cal):
    """The fitter's default theta: the sampler's initial intercepts, no covariate effect, Sigma = I."""
    x, t_x, T_cal = (np.asarray(v, dtype=np.float64) for v in (x, t_x, T_cal))
    lam = x.mean() / np.mean(np.where(t_x == 0, T_cal, t_x))
    theta = np.zeros(2 * K + 3)
    theta[0] = np.log(lam)
    theta[K] = np.log(np.mean(1.0 / (t_x + 0.5 / lam)))
    return theta

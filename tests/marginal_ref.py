"""Float64 model of the marginal likelihood of csrc/marginal.hip — TEST
INFRASTRUCTURE ONLY, plain numpy, vectorised over records and customers — and its 40-digit mpmath
twin.

Per (level-2 record r, customer i) the customer's (log lambda, log mu) = (a, b) is integrated out of
the Pareto/NBD individual likelihood against N2((a, b); m_i, Sigma_12) of the record, times (spend)
N(log_s; m_3 + c (theta - m_12), v), c = Sigma_3,12 Sigma_12^-1, v = Sigma_33 - c Sigma_12,3 + omega2.
The likelihood is the sum of two log-concave components, each integrated on its own and the two joined
by logaddexp:

    dropped out   lambda^x mu / (lambda + mu) exp(-(lambda + mu) t_x)        (xa, xb, t) = (x, 1, t_x)
    alive         lambda^(x + 1) / (lambda + mu) exp(-(lambda + mu) T_cal)   (xa, xb, t) = (x + 1, 0, T_cal)

    h(a, b) = (((xa a + xb b) - log(lambda + mu)) - (lambda + mu) t) + gaussian(a, b)

Each component: NEWTON_STEPS damped Newton steps from the prior mean (a, b) = (m_0, m_1) (no early exit;
a step's larger coordinate is capped at STEP_CAP), then the order-Q Gauss-Hermite rule of
csrc/gauss_hermite.h centred there and scaled by the Cholesky factor L of the inverse negative Hessian,
the Q^2 terms carried through a running maximum in (j, k) order.  Every operation is written in the
order csrc/marginal.hip has it; nothing is contracted.
"""
from __future__ import annotations

import os
import re

import numpy as np

ORDERS = (8, 16, 24, 32)
DEFAULT_ORDER = 32
NEWTON_STEPS = 16
STEP_CAP = 2.0
STEP_DONE = 1e-9      # "steps used": the first step whose larger coordinate is below this
BLOCK = 256
LOG_2PI = float.fromhex("0x1.d67f1c864beb5p+0")   # log(2 pi)
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
N_CONST = 10          # P00 P01 P11 H00 H01 H11 c0 sc1 sc2 v   (cs follows: N_CONST + 1 doubles)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc_clv_model_amd", "csrc",
                      "gauss_hermite.h")


def gh_tables(path: str = HEADER):
    """{Q: (t, w, c)} parsed from csrc/gauss_hermite.h."""
    with open(path) as f:
        text = f.read()
    orders = [int(v) for v in re.search(r"CLV_GH_ORDERS \{([^}]*)\}", text).group(1).split(",")]
    cols = {}
    for key in "TWC":
        body = re.search(r"CLV_GH_%s_INIT \{(.*?)\n\}" % key, text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body)
        cols[key] = np.array([float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", body)])
    out, at = {}, 0
    for Q in orders:
        out[Q] = tuple(cols[key][at:at + Q] for key in "TWC")
        at += Q
    assert all(len(cols[key]) == at for key in "TWC")
    return out


def record_constants(rec, D, K, spend, omega2):
    """dict of the record's constants (NaN throughout where Sigma_12 is not positive definite or the
    spend variance is not positive)."""
    rec = np.asarray(rec, dtype=np.float64)
    sg = rec[D * K:]
    s00, s01, s11 = (sg[0], sg[1], sg[2]) if D == 2 else (sg[0], sg[1], sg[3])
    with np.errstate(all="ignore"):
        det = s00 * s11 - s01 * s01
        ok = (s00 > 0.0) and (det > 0.0)
        P00, P01, P11 = s11 / det, -(s01 / det), s00 / det
        c0 = -LOG_2PI - 0.5 * np.log(det)
        H00, H01, H11 = P00, P01, P11
        sc1 = sc2 = cs = 0.0
        v = 1.0
        if spend:
            s02, s12, s22 = sg[2], sg[4], sg[5]
            sc1 = (s02 * s11 - s12 * s01) / det
            sc2 = (s12 * s00 - s02 * s01) / det
            v = (s22 - (sc1 * s02 + sc2 * s12)) + omega2
            ok = ok and (v > 0.0)
            cs = -0.5 * (LOG_2PI + np.log(v))
            H00 = P00 + (sc1 * sc1) / v
            H01 = P01 + (sc1 * sc2) / v
            H11 = P11 + (sc2 * sc2) / v
    c = dict(P00=P00, P01=P01, P11=P11, H00=H00, H01=H01, H11=H11, c0=c0, sc1=sc1, sc2=sc2, v=v, cs=cs)
    if not ok:
        c = {k: np.nan for k in c}
    return c


def means(rec, D, K, cov, n, spend):
    """(m0, m1, m2) [n]: m_j = sum_k X_ik beta_kj, k ascending, X_i0 = 1 (m2 only with the spend term)."""
    rec = np.asarray(rec, dtype=np.float64)
    ms = []
    for j in range(3 if spend else 2):
        m = np.full(n, rec[j * K])
        for k in range(1, K):
            m = m + cov[k - 1] * rec[j * K + k]
        ms.append(m)
    return ms + [np.zeros(n)] * (3 - len(ms))


class Component:
    """One log-concave component of one record over n customers: the data (xa, xb, t), the means and
    the record's constants."""

    def __init__(self, c, xa, xb, t, m0, m1, r0, spend):
        self.c, self.xa, self.xb, self.t, self.m0, self.m1, self.r0, self.spend = c, xa, xb, t, m0, m1, r0, spend

    def h(self, a, b, lam=None):
        c = self.c
        da, db = a - self.m0, b - self.m1
        quad = (c["P00"] * da * da + 2.0 * c["P01"] * da * db) + c["P11"] * db * db
        if lam is None:
            lam = np.exp(a)
        mu = np.exp(b)
        ml = lam + mu
        lik = ((self.xa * a + self.xb * b) - np.log(ml)) - ml * self.t
        h = lik + (c["c0"] - 0.5 * quad)
        if self.spend:
            r = (self.r0 - c["sc1"] * da) - c["sc2"] * db
            h = h + (c["cs"] - (r * r) / (2.0 * c["v"]))
        return h

    def derivs(self, a, b):
        """(ga, gb, n00, n01, n11): the gradient and the negative Hessian of h."""
        c = self.c
        da, db = a - self.m0, b - self.m1
        lam, mu = np.exp(a), np.exp(b)
        ml = lam + mu
        q, qm = lam / ml, mu / ml
        ga = ((self.xa - q) - lam * self.t) - (c["P00"] * da + c["P01"] * db)
        gb = ((self.xb - qm) - mu * self.t) - (c["P01"] * da + c["P11"] * db)
        if self.spend:
            rv = ((self.r0 - c["sc1"] * da) - c["sc2"] * db) / c["v"]
            ga = ga + c["sc1"] * rv
            gb = gb + c["sc2"] * rv
        qq = q * qm
        n00 = (qq + lam * self.t) + c["H00"]
        n01 = c["H01"] - qq
        n11 = (qq + mu * self.t) + c["H11"]
        return ga, gb, n00, n01, n11

    def safe(self, n00, n01, n11):
        """The negative Hessian, or the gaussian part's alone where it is not positive definite."""
        c = self.c
        det = n00 * n11 - n01 * n01
        bad = ~(det > 0.0) & ~np.isnan(det)
        n00 = np.where(bad, c["H00"], n00)
        n01 = np.where(bad, c["H01"], n01)
        n11 = np.where(bad, c["H11"], n11)
        det = np.where(bad, c["H00"] * c["H11"] - c["H01"] * c["H01"], det)
        return n00, n01, n11, det

    def centre(self):
        """(a, b, L00, L10, L11, steps used) after NEWTON_STEPS capped Newton steps from (m0, m1)."""
        a, b = self.m0.copy(), self.m1.copy()
        used = np.full(a.shape, float(NEWTON_STEPS))
        for it in range(NEWTON_STEPS):
            ga, gb, n00, n01, n11 = self.derivs(a, b)
            n00, n01, n11, det = self.safe(n00, n01, n11)
            sa = (n11 * ga - n01 * gb) / det
            sb = (n00 * gb - n01 * ga) / det
            mx = np.maximum(np.abs(sa), np.abs(sb))
            over = mx > STEP_CAP
            scale = np.where(over, STEP_CAP / np.where(over, mx, 1.0), 1.0)
            sa = np.where(over, sa * scale, sa)
            sb = np.where(over, sb * scale, sb)
            a = a + sa
            b = b + sb
            used = np.where((mx < STEP_DONE) & (used == NEWTON_STEPS), float(it + 1), used)
        return (a, b) + self.factor(a, b) + (used,)

    def factor(self, a, b):
        """(L00, L10, L11): the Cholesky factor of the inverse negative Hessian at (a, b)."""
        _, _, n00, n01, n11 = self.derivs(a, b)
        n00, n01, n11, det = self.safe(n00, n01, n11)
        L00 = np.sqrt(n11 / det)
        L10 = -(n01 / det) / L00
        L11 = 1.0 / np.sqrt(n11)
        return L00, L10, L11

    def integral(self, tab, centre):
        """log of the component's integral by the rule tab = (t, w, c) at centre = (a, b, L00, L10, L11)."""
        t, _, cw = tab
        a0, b0, L00, L10, L11 = centre[:5]
        m = np.full(a0.shape, -np.inf)
        s = np.zeros(a0.shape)
        for j in range(len(t)):
            a = a0 + SQRT2 * (L00 * t[j])
            lam = np.exp(a)
            for k in range(len(t)):
                b = b0 + SQRT2 * (L10 * t[j] + L11 * t[k])
                v = (cw[j] + cw[k]) + self.h(a, b, lam)
                up = v > m
                e = np.exp(np.where(up, m - v, v - m))
                s = np.where(up, s * e + 1.0, s + e)
                m = np.where(up, v, m)
        return np.log(2.0 * (L00 * L11)) + (m + np.log(s))


def components(rec, D, K, cov, x, t_x, T_cal, log_s=None, omega2=1.0):
    """The (dropped-out, alive) components of one record over the customers."""
    x = np.asarray(x, dtype=np.float64)
    t_x, T_cal = np.asarray(t_x, dtype=np.float64), np.asarray(T_cal, dtype=np.float64)
    spend = log_s is not None
    c = record_constants(rec, D, K, spend, omega2)
    m0, m1, m2 = means(rec, D, K, cov, len(x), spend)
    r0 = (np.asarray(log_s, dtype=np.float64) - m2) if spend else np.zeros(len(x))
    return (Component(c, x, 1.0, t_x, m0, m1, r0, spend), Component(c, x + 1.0, 0.0, T_cal, m0, m1, r0, spend))


def join(iD, iA):
    """logaddexp of the two components; NaN where either is not finite."""
    hi, lo = np.maximum(iD, iA), np.minimum(iD, iA)
    out = hi + np.log1p(np.exp(lo - hi))
    return np.where(np.isfinite(iD) & np.isfinite(iA), out, np.nan)


def components_all(level2, D, K, cov, x, t_x, T_cal, log_s=None, omega2=1.0):
    """The two components over every (record, customer): the constants as [R][1] columns, the means
    [R][n] — the same operations as :func:`components` record by record, broadcast."""
    level2 = np.asarray(level2, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    t_x, T_cal = np.asarray(t_x, dtype=np.float64), np.asarray(T_cal, dtype=np.float64)
    spend = log_s is not None
    cs = [record_constants(rec, D, K, spend, omega2) for rec in level2]
    c = {k: np.array([ci[k] for ci in cs], dtype=np.float64)[:, None] for k in cs[0]}
    ms = [means(rec, D, K, cov, len(x), spend) for rec in level2]
    m0, m1, m2 = (np.stack([m[j] for m in ms]) for j in range(3))
    r0 = (np.asarray(log_s, dtype=np.float64) - m2) if spend else np.zeros(m0.shape)
    return (Component(c, x, 1.0, t_x, m0, m1, r0, spend), Component(c, x + 1.0, 0.0, T_cal, m0, m1, r0, spend))


def marginal_loglik(level2, D, K, cov, x, t_x, T_cal, log_s=None, omega2=1.0, nodes=DEFAULT_ORDER, centres=None,
                    tables=None):
    """(l_marg [R][n], centres [R][n][12]): per component (a, b, L00, L10, L11, steps used), the dropped-out
    component first.  ``centres`` given: the rule is applied there instead of at the model's own."""
    level2 = np.asarray(level2, dtype=np.float64)
    tab = (tables or gh_tables())[nodes]
    cen = np.empty((level2.shape[0], len(x), 12))
    parts = []
    with np.errstate(all="ignore"):
        for q, comp in enumerate(components_all(level2, D, K, cov, x, t_x, T_cal, log_s, omega2)):
            ce = comp.centre() if centres is None else tuple(centres[:, :, 6 * q + p] for p in range(6))
            cen[:, :, 6 * q:6 * q + 6] = np.stack(ce, axis=-1)
            parts.append(comp.integral(tab, ce))
        out = join(parts[0], parts[1])
    return out, cen


def model_centres(level2, D, K, cov, x, t_x, T_cal, log_s=None, omega2=1.0):
    """The centres [R][n][12] alone (the Newton iterations without the rule)."""
    level2 = np.asarray(level2, dtype=np.float64)
    cen = np.empty((level2.shape[0], len(x), 12))
    with np.errstate(all="ignore"):
        for q, comp in enumerate(components_all(level2, D, K, cov, x, t_x, T_cal, log_s, omega2)):
            cen[:, :, 6 * q:6 * q + 6] = np.stack(comp.centre(), axis=-1)
    return cen


def log_score(lm):
    """Per customer logsumexp_r l_marg - log R (the maximum, then the terms in record order)."""
    lm = np.asarray(lm, dtype=np.float64)
    m = lm.max(axis=0)
    s = np.zeros(lm.shape[1])
    for r in range(lm.shape[0]):
        s = s + np.exp(lm[r] - m)
    return (m + np.log(s)) - np.log(float(lm.shape[0]))


# ---------------------------------------------------------------------------------------------
# the 40-digit twin: the same rule at the model's own centre, every term in mpmath
# ---------------------------------------------------------------------------------------------
def mp_h(mp, c, xa, xb, t, m0, m1, r0, spend, a, b):
    """h(a, b) of one component of one customer in mpmath (c: record_constants in mpf)."""
    da, db = a - m0, b - m1
    quad = c["P00"] * da * da + 2 * c["P01"] * da * db + c["P11"] * db * db
    lam, mu = mp.exp(a), mp.exp(b)
    ml = lam + mu
    h = xa * a + xb * b - mp.log(ml) - ml * t + c["c0"] - quad / 2
    if spend:
        r = r0 - c["sc1"] * da - c["sc2"] * db
        h = h + c["cs"] - r * r / (2 * c["v"])
    return h


def mp_constants(mp, rec, D, K, spend, omega2):
    """record_constants from the record's doubles, in mpmath."""
    sg = [mp.mpf(float(v)) for v in np.asarray(rec)[D * K:]]
    s00, s01, s11 = (sg[0], sg[1], sg[2]) if D == 2 else (sg[0], sg[1], sg[3])
    det = s00 * s11 - s01 * s01
    c = dict(P00=s11 / det, P01=-s01 / det, P11=s00 / det, c0=-mp.log(2 * mp.pi) - mp.log(det) / 2, sc1=mp.mpf(0),
             sc2=mp.mpf(0), v=mp.mpf(1), cs=mp.mpf(0))
    if spend:
        s02, s12, s22 = sg[2], sg[4], sg[5]
        c["sc1"] = (s02 * s11 - s12 * s01) / det
        c["sc2"] = (s12 * s00 - s02 * s01) / det
        c["v"] = s22 - (c["sc1"] * s02 + c["sc2"] * s12) + mp.mpf(float(omega2))
        c["cs"] = -mp.log(2 * mp.pi * c["v"]) / 2
    return c


def mp_customer(mp, rec, D, K, cov, i, x, t_x, T_cal, log_s):
    """((xa, xb, t) of the two components, m0, m1, r0) of customer i in mpmath."""
    f = lambda v: mp.mpf(float(v))  # noqa: E731
    rec = np.asarray(rec)
    m = []
    for j in range(3 if log_s is not None else 2):
        acc = f(rec[j * K])
        for k in range(1, K):
            acc += f(cov[k - 1][i]) * f(rec[j * K + k])
        m.append(acc)
    r0 = (f(log_s[i]) - m[2]) if log_s is not None else mp.mpf(0)
    xi = f(x[i])
    return ((xi, mp.mpf(1), f(t_x[i])), (xi + 1, mp.mpf(0), f(T_cal[i]))), m[0], m[1], r0


def twin(level2, D, K, cov, x, t_x, T_cal, log_s, omega2, nodes, centres, cells):
    """The rule of order ``nodes`` at ``centres`` (the model's) with every term and the sums in 40
    digits, for the (record, customer) pairs ``cells``: a float array."""
    import mpmath as mp
    mp.mp.dps = 40
    tabs = _mp_rule(nodes)
    out = []
    for r, i in cells:
        c = mp_constants(mp, level2[r], D, K, log_s is not None, omega2)
        comps, m0, m1, r0 = mp_customer(mp, level2[r], D, K, cov, i, x, t_x, T_cal, log_s)
        tot = mp.mpf(0)
        for q, (xa, xb, t) in enumerate(comps):
            a0, b0, L00, L10, L11 = (mp.mpf(float(v)) for v in centres[r, i, 6 * q:6 * q + 5])
            acc = mp.mpf(0)
            for tj, wj in tabs:
                a = a0 + mp.sqrt(2) * L00 * tj
                for tk, wk in tabs:
                    b = b0 + mp.sqrt(2) * (L10 * tj + L11 * tk)
                    acc += wj * wk * mp.exp(tj * tj + tk * tk + mp_h(mp, c, xa, xb, t, m0, m1, r0, log_s is not None, a, b))
            tot += 2 * L00 * L11 * acc
        out.append(float(mp.log(tot)))
    return np.array(out)


def _mp_rule(Q):
    """The order-Q rule of csrc/gauss_hermite.h (its doubles, exactly) as mpmath (t, w) pairs."""
    import mpmath as mp
    t, w, _ = gh_tables()[Q]
    return [(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(t, w)]


# ---------------------------------------------------------------------------------------------
# the rounding unit and the cases the device is held to
# ---------------------------------------------------------------------------------------------
# The model's largest deviation from its twin, relative to max(1, |l_marg|) (the rounding of h grows
# with the size of its terms, x log lambda and (lambda + mu) t, which is the size of l_marg):
# measured by tests/test_marginal_cpu.py over the exact fixture's cells, recorded in DESIGN.md
# section 4k.  The device is held to 4 units against the model.
UNIT_REL = 1.6e-15


def unit_tol(lm):
    """4 units at the values lm."""
    return 4.0 * UNIT_REL * np.maximum(1.0, np.abs(lm))


def case_records(R, D, K, seed):
    """R CDNOW-like level-2 records [R][D K + D (D + 1) / 2]: intercepts near (-3.5, -3.6, 3.3), small
    covariate effects, Sigma = A A' of a jittered factor (Sigma_11 about 1.3, Sigma_22 about 3, Sigma_33
    about 0.5)."""
    rng = np.random.default_rng(seed)
    recs = np.empty((R, D * K + D * (D + 1) // 2))
    base = np.array([-3.5, -3.6, 3.3])[:D]
    sd = np.array([1.15, 1.75, 0.7])[:D]
    for r in range(R):
        beta = np.zeros((K, D))
        beta[0] = base + 0.05 * rng.standard_normal(D)
        beta[1:] = 0.15 * rng.standard_normal((K - 1, D))
        A = np.diag(sd * (1.0 + 0.05 * rng.standard_normal(D))) + np.tril(0.25 * rng.standard_normal((D, D)), -1)
        Sigma = A @ A.T
        recs[r] = np.concatenate([beta.T.ravel(), Sigma[np.triu_indices(D)]])
    return recs


def case_customers(N, K, seed):
    """(DataFrame with x, t_x, T_cal, log_s, c1 .. c{K-1}; covariate names): CDNOW's customers taken
    cyclically, every fifth row replaced by an edge archetype (tests/helpers.py: x = 0 on every span,
    t_x = T, t_x just under T, heavy buyers on weekly and daily clocks)."""
    from tests import helpers
    df = helpers.cdnow_tiled(N)[["x", "t_x", "T_cal", "log_s"]].copy()
    edge = helpers.edge_cbs(max(N, 41))
    for i in range(0, N, 5):
        j = (i // 5) % 41
        for col in ("x", "t_x", "T_cal", "log_s"):
            df.loc[i, col] = edge.loc[j, col]
    df["x"] = df["x"].astype(np.int64)
    names = [f"c{k}" for k in range(1, K)]
    if K > 1:
        df = helpers.with_covariates(df, K - 1, seed)
    return df, names


def case_arrays(df, names, spend):
    """(cov, x, t_x, T_cal, log_s) of a case frame as the C ABI takes them."""
    cov = np.ascontiguousarray(df[names].to_numpy(float).T) if names else None
    return (cov, np.ascontiguousarray(df["x"].to_numpy(), dtype=np.int32), np.ascontiguousarray(df["t_x"].to_numpy(float)),
            np.ascontiguousarray(df["T_cal"].to_numpy(float)),
            np.ascontiguousarray(df["log_s"].to_numpy(float)) if spend else None)

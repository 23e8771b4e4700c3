"""Models of the Pareto/NBD likelihood's second evaluation of I (csrc/pnbd.hip pnbd_si_quadrature, DESIGN.md
section 4o), on top of tests/pnbd_ref.py and tests/mle_ext_ref.py, which stay the models of everything else.

exact_*   mpmath at 40 digits: mpmath.quad of I = int_{t_x}^{T} (alpha+y)^-(r+x) (beta+y)^-(s+1) dy over panels
          that double from t_x (the integrand's scale there is min(alpha, beta) + t_x), and the gradient by
          quadrature of the differentiated integrand over the same panels.
model_*   float64 numpy restatement of the device algorithm: the path choice of the three modes, the panels
          in d = log((m + y) / (m + t_x)), the exponent shared by the integrand and its four gradient weights.

Two wrong variants for the power checks (``variant=``): "log_difference_width" takes the total width as
log(m + T) - log(m + t_x), "exchanged_exponents" gives p_m to the factor with the larger offset.
"""
from __future__ import annotations

import math

import numpy as np

from tests import mle_ext_ref as M
from tests import pnbd_ref as R

MODES = ("series", "auto", "quadrature")
Z_SWITCH = 0.9           # PNBD_Z_SWITCH
Q_SLOPE = 4.0            # PNBD_Q_SLOPE: a panel is at most Q_SLOPE / |d log integrand / dd| wide, and at most 1
Q_SPAN = 40.0            # PNBD_Q_SPAN: the panels may stop once the integrand is exp(-40) below its start
Q_PANEL_CAP = 4096       # PNBD_Q_PANEL_CAP
VARIANTS = (None, "log_difference_width", "exchanged_exponents")


# ---------------------------------------------------------------------------------------------
# exact (mpmath)
# ---------------------------------------------------------------------------------------------
def _panels(mp, tx, T, a, b):
    """Break points doubling from t_x: t_x + w 2^k with w = (min(alpha, beta) + t_x) / 8, then T."""
    w = (min(a, b) + tx) / 8
    pts = [tx]
    while tx + w < T and len(pts) < 400:
        pts.append(tx + w)
        w *= 2
    pts.append(T)
    return pts


def exact_parts(x, tx, T, params):
    """(log L, grad[4] with respect to log(r, alpha, s, beta), A, s I) as mpf; exact rationals of the floats."""
    mp = R._mp()
    r, a, s, b = (mp.mpf(float(v)) for v in params)
    x, tx, T = int(x), mp.mpf(float(tx)), mp.mpf(float(T))
    rx = r + x
    A = (a + T) ** (-rx) * (b + T) ** (-s)
    dA = [-mp.log(a + T), -rx / (a + T), -mp.log(b + T), -s / (b + T)]
    I, dI = mp.mpf(0), [mp.mpf(0)] * 4
    if tx < T:
        pts = _panels(mp, tx, T, a, b)
        # relative to the integrand at t_x, so that nothing underflows at x in the thousands
        l0 = -rx * mp.log(a + tx) - (s + 1) * mp.log(b + tx)

        def f(y):
            return mp.exp(-rx * mp.log(a + y) - (s + 1) * mp.log(b + y) - l0)
        q = mp.quad(f, pts)
        wts = (lambda y: -mp.log(a + y), lambda y: -rx / (a + y), lambda y: -mp.log(b + y), lambda y: -(s + 1) / (b + y))
        dI = [mp.quad(lambda y, w=w: f(y) * w(y), pts) / q for w in wts]
        dI[2] += 1 / s
        I = q * mp.exp(l0)
    den = A + s * I
    wA, wI = A / den, s * I / den
    logL = mp.loggamma(rx) - mp.loggamma(r) + r * mp.log(a) + s * mp.log(b) + mp.log(den)
    base = [mp.digamma(rx) - mp.digamma(r) + mp.log(a), r / a, mp.log(b), s / b]
    scale = [r, a, s, b]
    grad = [(base[j] + wA * dA[j] + wI * dI[j]) * scale[j] for j in range(4)]
    return logL, grad, A, s * I


def exact_customer(x, tx, T, params, t_star):
    """(log L, grad[4], P(alive), E[Y(t_star) | x, t_x, T], log(s I)) as mpf; log(s I) = -inf at t_x = T."""
    mp = R._mp()
    logL, grad, A, sI = exact_parts(x, tx, T, params)
    r, a, s, b = (mp.mpf(float(v)) for v in params)
    Tm = mp.mpf(float(T))
    pa = A / (A + sI)
    ell = mp.log((b + Tm + mp.mpf(float(t_star))) / (b + Tm))
    phi = ell if s == 1 else -mp.expm1(-(s - 1) * ell) / (s - 1)
    return logL, grad, pa, pa * (r + int(x)) * (b + Tm) / (a + Tm) * phi, (mp.log(sI) if sI > 0 else -mp.inf)


# ---------------------------------------------------------------------------------------------
# float64 model
# ---------------------------------------------------------------------------------------------
_GL = None


def _gl():
    global _GL
    if _GL is None:
        _GL = M.gauss_legendre_header()
    return _GL


def z_tx(tx, a, b):
    """z(t_x) = |alpha - beta| / (max(alpha, beta) + t_x) as pnbd_log_h forms it."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (np.where(a < b, b, a) + np.asarray(tx, np.float64))


def takes_quadrature(mode, tx, T, a, b):
    """The path of each customer: True where I comes from the quadrature."""
    if mode not in MODES:
        raise ValueError(f"integral must be one of {MODES}")
    has = np.asarray(tx, np.float64) < np.asarray(T, np.float64)
    if mode == "series":
        return np.zeros(has.shape, bool)
    if mode == "quadrature":
        return has
    return has & ~(z_tx(tx, a, b) <= Z_SWITCH)


def model_si_quadrature(x, tx, T, r, a, s, b, variant=None):
    """(log(s I), d log(s I) / d(r, alpha, s, beta) [4], panels) of one customer with t_x < T (scalars)."""
    X, W = _gl()
    x, tx, T, r, a, s, b = (float(v) for v in (x, tx, T, r, a, s, b))
    nan = (math.nan, [math.nan] * 4, 0)
    swap = a < b                                   # alpha is the smaller offset
    m, dl = (a if swap else b), abs(a - b)
    pm, pM = (r + x, s + 1.0) if swap else (s + 1.0, r + x)
    if variant == "exchanged_exponents":
        pm, pM = pM, pm
    e0 = m + tx
    eD = e0 + dl
    if not (e0 > 0.0 and math.isfinite(eD)):
        return nan
    q = e0 / eD
    if variant == "log_difference_width":
        D = math.log(m + T) - math.log(m + tx)
    else:
        D = math.log1p((T - tx) / e0)
    if not math.isfinite(D):
        return nan
    l0, lD = math.log(e0), math.log(eD)
    d, Q, Sd, SL, Sm, SM = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    panels = 0
    grew = True
    for _ in range(Q_PANEL_CAP):
        if not d < D:
            break
        em = math.expm1(d)
        E = (1.0 - pm) * d - pM * math.log1p(q * em)
        if E < -Q_SPAN and not grew:
            break
        rho = q * (em + 1.0) / (1.0 + q * em)
        slope = (1.0 - pm) - pM * rho
        hi = d + min(1.0, Q_SLOPE / abs(slope)) if slope != 0.0 else d + 1.0
        if not hi < D:
            hi = D
        mid, half = 0.5 * (d + hi), 0.5 * (hi - d)
        c, cd, cL, cm, cM = 0.0, 0.0, 0.0, 0.0, 0.0
        for j in range(len(X)):
            dj = mid + half * X[j]
            ej = math.expm1(dj)
            u = q * ej
            Lj = math.log1p(u)
            g = W[j] * math.exp((1.0 - pm) * dj - pM * Lj)
            c += g
            cd += g * dj
            cL += g * Lj
            cm += g / (e0 * (ej + 1.0))
            cM += g / (eD * (1.0 + u))
        nQ = Q + c * half
        grew = nQ != Q
        Q = nQ
        Sd += cd * half
        SL += cL * half
        Sm += cm * half
        SM += cM * half
        d = hi
        panels += 1
    if not Q > 0.0:
        return -math.inf, [0.0] * 4, panels
    lsi = math.log(s) + (((1.0 - pm) * l0 - pM * lD) + math.log(Q))
    lm, lM, im, iM = l0 + Sd / Q, lD + SL / Q, Sm / Q, SM / Q    # means of log(m+y), log(M+y), 1/(m+y), 1/(M+y)
    rx, s1 = r + x, s + 1.0
    if variant == "exchanged_exponents":
        swap = not swap
    if swap:
        dI = [-lm, -rx * im, -lM + 1.0 / s, -s1 * iM]
    else:
        dI = [-lM, -rx * iM, -lm + 1.0 / s, -s1 * im]
    return lsi, dI, panels


def model_customers_tail(x, tx, T, r, a, s, b, mode="auto", t_star=None, variant=None):
    """mle_ext_ref.model_customers_ab in the handle's mode: dict(logL, grad [n][4] with respect to
    log(r, alpha_i, s, beta_i), p_alive, ey, converged, quadrature, panels, log_sI).  A customer on the series
    path has the series model's values; on the quadrature path ``converged`` means a finite result and
    ``log_sI`` is log(s I) as the quadrature forms it (NaN on the series path, which does not expose it)."""
    x = np.asarray(x, np.float64)
    tx, T = np.asarray(tx, np.float64), np.asarray(T, np.float64)
    n = x.shape[0]
    a, b = np.broadcast_to(np.asarray(a, np.float64), (n,)), np.broadcast_to(np.asarray(b, np.float64), (n,))
    r, s = float(r), float(s)
    quad = takes_quadrature(mode, tx, T, a, b)
    out = dict(logL=np.zeros(n), grad=np.zeros((n, 4)), p_alive=np.zeros(n), converged=np.ones(n, bool),
               quadrature=quad, panels=np.zeros(n, np.int64), log_sI=np.full(n, np.nan))
    if t_star is not None:
        out["ey"] = np.zeros(n)
    k = np.flatnonzero(~quad)
    if k.size:
        ser = M.model_customers_ab(x[k], tx[k], T[k], r, a[k], s, b[k], t_star)
        for key in ("logL", "grad", "p_alive", "converged", "ey"):
            if key in ser:
                out[key][k] = ser[key]
    for i in np.flatnonzero(quad):
        xi, ai, bi, Ti = x[i], a[i], b[i], T[i]
        rx = r + xi
        dig = float(np.sum(1.0 / (r + np.arange(int(xi)))))
        laT, lbT = math.log(ai + Ti), math.log(bi + Ti)
        logA = -rx * laT - s * lbT
        dA = (-laT, -rx / (ai + Ti), -lbT, -s / (bi + Ti))
        logsI, dI, out["panels"][i] = model_si_quadrature(xi, tx[i], Ti, r, ai, s, bi, variant)
        out["log_sI"][i] = logsI
        mx = max(logA, logsI) if not math.isnan(logsI) else math.nan
        eA, eI = math.exp(logA - mx), math.exp(logsI - mx)
        den = eA + eI
        wA, wI = eA / den, eI / den
        out["logL"][i] = math.lgamma(rx) - math.lgamma(r) + r * math.log(ai) + s * math.log(bi) + (mx + math.log(den))
        base = (dig + math.log(ai), r / ai, math.log(bi), s / bi)
        scale = (r, ai, s, bi)
        out["grad"][i] = [(base[j] + wA * dA[j] + wI * dI[j]) * scale[j] for j in range(4)]
        out["p_alive"][i] = wA
        if t_star is not None:
            out["ey"][i] = wA * rx * (bi + Ti) / (ai + Ti) * float(R.phi(s - 1.0, np.log1p(float(t_star) / (bi + Ti))))
        fin = math.isfinite(out["logL"][i]) and np.isfinite(out["grad"][i]).all() and math.isfinite(wA)
        out["converged"][i] = fin
        if not fin:
            out["logL"][i] = out["p_alive"][i] = math.nan
            out["grad"][i] = math.nan
            if t_star is not None:
                out["ey"][i] = math.nan
    return out


def model_customers_cov_tail(x, tx, T, params, z1, z2, mode="auto", t_star=None):
    a, b = M.customer_scales(params, z1, z2)
    m = model_customers_tail(x, tx, T, params[0], a, params[2], b, mode, t_star)
    m["scores"] = M.theta_scores(m["grad"], z1, z2)
    m["alpha"], m["beta"] = a, b
    return m


def model_value_and_grad_cov_tail(x, tx, T, z1, z2, mode="auto", weights=None):
    """mle_ext_ref.model_value_and_grad_cov in the handle's mode (no penalty)."""
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    sw = w.sum()

    def f(theta):
        p = np.concatenate([np.exp(theta[:4]), theta[4:]])
        m = model_customers_cov_tail(x, tx, T, p, z1, z2, mode)
        return -(w * m["logL"]).sum() / sw, -(w[:, None] * m["scores"]).sum(0) / sw
    return f

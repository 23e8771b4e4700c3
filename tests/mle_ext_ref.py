"""Models of the classical baseline's extensions (csrc/pnbd.hip covariate kernels and DERT, csrc/gg.hip,
mcmc_clv_model_amd/mle.py), on top of tests/pnbd_ref.py.

exact_*   mpmath at 40 digits: the Pareto/NBD quadrature of pnbd_ref at each customer's own (r, alpha_i, s,
          beta_i) with the covariate gradient by the chain rule; the Hessian by mpmath.diff of that
          quadrature; the Gamma-Gamma likelihood from loggamma and digamma; the DERT integral by quadrature
          of the integral itself.  Only the golden maker and the CPU tests need mpmath.
model_*   float64 numpy restatements of the device algorithms.

theta = (log r, log alpha0, log s, log beta0, gamma1[K1], gamma2[K2]); z1 [K1][n], z2 [K2][n] (the device
layout); alpha_i = alpha0 exp(-gamma1' z1_i), beta_i = beta0 exp(-gamma2' z2_i) (Fader & Hardie 2007).
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from tests import pnbd_ref as R

HESSIAN_STEP = 2.0 ** -15


def _mp():
    return R._mp()


# ---------------------------------------------------------------------------------------------
# Pareto/NBD with covariates
# ---------------------------------------------------------------------------------------------
def split(params, k1, k2):
    p = np.asarray(params, np.float64)
    return p[:4], p[4:4 + k1], p[4 + k1:4 + k1 + k2]


def customer_scales(params, z1, z2):
    """(alpha_i, beta_i), the dot products accumulated column by column as the device does."""
    z1, z2 = np.asarray(z1, np.float64).reshape(-1, np.shape(z1)[-1]), np.asarray(z2, np.float64).reshape(-1, np.shape(z2)[-1])
    base, g1, g2 = split(params, z1.shape[0], z2.shape[0])
    e1, e2 = np.zeros(z1.shape[1]), np.zeros(z2.shape[1])
    for k in range(z1.shape[0]):
        e1 = e1 + g1[k] * z1[k]
    for k in range(z2.shape[0]):
        e2 = e2 + g2[k] * z2[k]
    return base[1] * np.exp(-e1), base[3] * np.exp(-e2)


def model_customers_ab(x, tx, T, r, a, s, b, t_star=None):
    """pnbd_ref.model_customers with per-customer alpha and beta arrays: dict(logL, grad [n][4] with
    respect to log(r, alpha_i, s, beta_i), p_alive, ey, converged)."""
    x = np.asarray(x, np.float64)
    tx, T = np.asarray(tx, np.float64), np.asarray(T, np.float64)
    n = x.shape[0]
    a, b = np.broadcast_to(np.asarray(a, np.float64), (n,)), np.broadcast_to(np.asarray(b, np.float64), (n,))
    r, s = float(r), float(s)
    rx = r + x
    lgr = np.array([math.lgamma(v) for v in rx]) - math.lgamma(r)
    dig = np.array([np.sum(1.0 / (r + np.arange(int(k)))) for k in x])
    laT, lbT = np.log(a + T), np.log(b + T)
    logA = -rx * laT - s * lbT
    dA = (-laT, -rx / (a + T), -lbT, -s / (b + T))
    has = tx < T
    logsI = np.full(n, -np.inf)
    dI = [np.zeros(n) for _ in range(4)]
    conv = np.ones(n, bool)
    if has.any():
        k = np.flatnonzero(has)
        h1, g1, _, c1 = R._log_h(tx[k], x[k], r, a[k], s, b[k])
        h2, g2, _, c2 = R._log_h(T[k], x[k], r, a[k], s, b[k])
        d = h2 - h1
        e = np.exp(d)
        om = -np.expm1(d)
        aa = r + s + x[k]
        ok = om > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            logsI[k] = np.where(ok, np.log(s) + h1 + np.log(om) - np.log(aa), -np.inf)
            for j in range(4):
                dj = (g1[j] - e * g2[j]) / om - 1.0 / aa * (j in (0, 2)) + (1.0 / s if j == 2 else 0.0)
                dI[j][k] = np.where(ok, dj, 0.0)
        conv[k] = c1 & c2
    mx = np.maximum(logA, logsI)
    eA, eI = np.exp(logA - mx), np.exp(logsI - mx)
    den = eA + eI
    wA, wI = eA / den, eI / den
    logL = lgr + r * np.log(a) + s * np.log(b) + (mx + np.log(den))
    base = (dig + np.log(a), r / a, np.log(b), s / b)
    scale = (r, a, s, b)
    grad = np.stack([(base[j] + wA * dA[j] + wI * dI[j]) * scale[j] for j in range(4)], axis=1)
    out = dict(logL=logL, grad=grad, p_alive=wA.copy(), converged=conv)
    if t_star is not None:
        out["ey"] = wA * rx * (b + T) / (a + T) * R.phi(s - 1.0, np.log1p(float(t_star) / (b + T)))
    for key in ("logL", "grad", "p_alive", "ey"):
        if key in out:
            out[key][~conv] = np.nan
    return out


def theta_scores(grad4, z1, z2):
    """[n][4 + K1 + K2] from the score with respect to log(r, alpha_i, s, beta_i): the chain rule."""
    z1, z2 = np.asarray(z1, np.float64), np.asarray(z2, np.float64)
    n = grad4.shape[0]
    return np.concatenate([grad4, -z1.reshape(-1, n).T * grad4[:, 1:2], -z2.reshape(-1, n).T * grad4[:, 3:4]], axis=1)


def model_customers_cov(x, tx, T, params, z1, z2, t_star=None):
    a, b = customer_scales(params, z1, z2)
    m = model_customers_ab(x, tx, T, params[0], a, params[2], b, t_star)
    m["scores"] = theta_scores(m["grad"], z1, z2)
    m["alpha"], m["beta"] = a, b
    return m


def model_gradient_cov(x, tx, T, z1, z2, weights=None):
    """theta -> d sum w log L / d theta of the float64 model."""
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)

    def g(theta):
        p = np.concatenate([np.exp(theta[:4]), theta[4:]])
        return (w[:, None] * model_customers_cov(x, tx, T, p, z1, z2)["scores"]).sum(0)
    return g


def model_value_and_grad_cov(x, tx, T, z1, z2, weights=None, penalizer_coef=0.0):
    """The covariate fitter's objective on theta: -sum w log L / sum w + pen (sum params^2 + sum gamma^2)."""
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    sw = w.sum()

    def f(theta):
        p = np.concatenate([np.exp(theta[:4]), theta[4:]])
        m = model_customers_cov(x, tx, T, p, z1, z2)
        val = -(w * m["logL"]).sum() / sw + penalizer_coef * (p ** 2).sum()
        g = -(w[:, None] * m["scores"]).sum(0) / sw
        g[:4] += 2.0 * penalizer_coef * p[:4] ** 2
        g[4:] += 2.0 * penalizer_coef * p[4:]
        return val, g
    return f


def central_hessian(grad, theta, step=HESSIAN_STEP):
    """mle.central_hessian, restated."""
    theta = np.asarray(theta, np.float64)
    P = theta.size
    H = np.empty((P, P))
    for j in range(P):
        e = np.zeros(P)
        e[j] = step
        up, dn = theta + e, theta - e
        H[:, j] = (grad(up) - grad(dn)) / (up[j] - dn[j])
    return 0.5 * (H + H.T)


def exact_customer_cov(x, tx, T, params, z1_i, z2_i, t_star):
    """(log L, P(alive), E[Y], grad[4 + K1 + K2] with respect to theta) of one customer as mpf."""
    mp = _mp()
    k1, k2 = len(z1_i), len(z2_i)
    base, g1, g2 = split(params, k1, k2)
    a = mp.mpf(float(base[1])) * mp.exp(-sum(mp.mpf(float(g)) * mp.mpf(float(z)) for g, z in zip(g1, z1_i)))
    b = mp.mpf(float(base[3])) * mp.exp(-sum(mp.mpf(float(g)) * mp.mpf(float(z)) for g, z in zip(g2, z2_i)))
    r, s = mp.mpf(float(base[0])), mp.mpf(float(base[2]))
    Tm = mp.mpf(float(T))
    logL, A, sI = R._exact_parts(mp, int(x), mp.mpf(float(tx)), Tm, r, a, s, b)
    p_alive = A / (A + sI)
    ell = mp.log((b + Tm + mp.mpf(float(t_star))) / (b + Tm))
    phi = ell if s == 1 else -mp.expm1(-(s - 1) * ell) / (s - 1)
    ey = p_alive * (r + int(x)) * (b + Tm) / (a + Tm) * phi
    p = [r, a, s, b]
    g4 = []
    for k in range(4):
        def f(v, k=k):
            q = list(p)
            q[k] = v
            return R._exact_parts(mp, int(x), mp.mpf(float(tx)), Tm, *q)[0]
        with mp.workdps(20):
            g4.append(mp.diff(f, p[k]) * p[k])
    grad = g4 + [-mp.mpf(float(z)) * g4[1] for z in z1_i] + [-mp.mpf(float(z)) * g4[3] for z in z2_i]
    return logL, p_alive, ey, grad


def exact_hessian_cov(x, tx, T, theta, z1, z2):
    """(H, H_abs): the Hessian of sum log L in theta and the sum over customers of the absolute values of
    their contributions (the scale of an error), as float64 arrays.  theta -> phi_i = (log r, log alpha_i, log s,
    log beta_i) is linear (log alpha_i = log alpha0 - gamma1' z1_i), so H = sum_i J_i' H_phi,i J_i with
    H_phi,i the 4 x 4 Hessian of customer i's quadrature log-likelihood by mpmath.diff."""
    mp = _mp()
    z1, z2 = np.asarray(z1, np.float64).reshape(-1, len(x)), np.asarray(z2, np.float64).reshape(-1, len(x))
    k1, k2 = z1.shape[0], z2.shape[0]
    P = 4 + k1 + k2
    th = [mp.mpf(float(v)) for v in theta]
    H, Habs = mp.zeros(P, P), mp.zeros(P, P)
    for i in range(len(x)):
        J = mp.zeros(4, P)
        for j in range(4):
            J[j, j] = 1
        for k in range(k1):
            J[1, 4 + k] = -mp.mpf(float(z1[k, i]))
        for k in range(k2):
            J[3, 4 + k1 + k] = -mp.mpf(float(z2[k, i]))
        ph = J * mp.matrix(th)
        xi, txm, Tm = int(x[i]), mp.mpf(float(tx[i])), mp.mpf(float(T[i]))

        def f(*v):
            return R._exact_parts(mp, xi, txm, Tm, *[mp.exp(t) for t in v])[0]
        Hp = mp.zeros(4, 4)
        for j in range(4):
            for k in range(j, 4):
                order = [0, 0, 0, 0]
                order[j] += 1
                order[k] += 1
                with mp.workdps(20):
                    Hp[j, k] = Hp[k, j] = mp.diff(f, tuple(ph), tuple(order))
        Hi = J.T * Hp * J
        H += Hi
        Habs += Hi.apply(abs)
    return tuple(np.array([[float(M[j, k]) for k in range(P)] for j in range(P)]) for M in (H, Habs))


# ---------------------------------------------------------------------------------------------
# chi-square survival function
# ---------------------------------------------------------------------------------------------
def exact_chi2_sf(x, df):
    mp = _mp()
    return mp.gammainc(mp.mpf(df) / 2, mp.mpf(float(x)) / 2, mp.inf, regularized=True)


# ---------------------------------------------------------------------------------------------
# Gamma-Gamma
# ---------------------------------------------------------------------------------------------
STIRLING_FROM = 32.0
PSI_SHIFT_TO = 10.0


def model_psi_tail(x):
    i2 = 1.0 / (x * x)
    return i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (
        1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 / 12.0))))))


def model_digamma(x):
    """psi(x), x > 0: upward shift to 10, then the asymptotic series (csrc/gg.hip gg_digamma)."""
    x = np.array(x, np.float64, copy=True).reshape(-1)
    shift = np.zeros_like(x)
    while True:
        k = x < PSI_SHIFT_TO
        if not k.any():
            break
        shift[k] += 1.0 / x[k]
        x[k] += 1.0
    return (np.log(x) - 0.5 / x - model_psi_tail(x)) - shift


def model_stirling(x):
    i = 1.0 / x
    i2 = i * i
    return i * (1.0 / 12.0 - i2 * (1.0 / 360.0 - i2 * (1.0 / 1260.0 - i2 * (1.0 / 1680.0 - i2 / 1188.0))))


def _lgamma(v):
    return np.array([math.lgamma(t) for t in np.asarray(v, np.float64).reshape(-1)])


def model_lgamma_diff(a, d, stable=True):
    """lnGamma(a + d) - lnGamma(a); ``stable=False`` is the two-lgamma form the device must not use."""
    a, d = (np.asarray(v, np.float64).reshape(-1) for v in np.broadcast_arrays(a, d))
    naive = _lgamma(a + d) - _lgamma(a)
    if not stable:
        return naive
    b = a + d
    with np.errstate(all="ignore"):
        st = ((a - 0.5) * np.log1p(d / a) - d) + d * np.log(b) + (model_stirling(b) - model_stirling(a))
    return np.where(a < STIRLING_FROM, naive, st)


def model_digamma_diff(a, d):
    a, d = (np.asarray(v, np.float64).reshape(-1) for v in np.broadcast_arrays(a, d))
    b = a + d
    st = np.log1p(d / a) + d / (2.0 * a * b) + (model_psi_tail(a) - model_psi_tail(b))
    return np.where(a < STIRLING_FROM, model_digamma(b) - model_digamma(a), st)


def model_gg_customers(n, m, params, stable=True):
    """dict(logL [N], grad [N][3] with respect to log(p, q, gamma)) of the float64 model."""
    n, m = np.asarray(n, np.float64).reshape(-1), np.asarray(m, np.float64).reshape(-1)
    p, q, g = (float(v) for v in params)
    a = p * n
    u = n * m / g
    l1, l2 = np.log1p(1.0 / u), np.log1p(u)
    logL = model_lgamma_diff(a, q, stable) - math.lgamma(q) - np.log(m) - a * l1 - q * l2
    grad = np.stack([a * (model_digamma_diff(a, q) - l1), q * (model_digamma_diff(np.full_like(a, q), a) - l2),
                     (q * u - a) / (1.0 + u)], axis=1)
    return dict(logL=logL, grad=grad)


def model_gg_value_and_grad(n, m, weights=None, penalizer_coef=0.0):
    w = np.ones(len(n)) if weights is None else np.asarray(weights, np.float64)
    sw = w.sum()

    def f(theta):
        p = np.exp(theta)
        c = model_gg_customers(n, m, p)
        return (-(w * c["logL"]).sum() / sw + penalizer_coef * (p ** 2).sum(),
                -(w[:, None] * c["grad"]).sum(0) / sw + 2.0 * penalizer_coef * p ** 2)
    return f


def model_gg_mean(n, m, params):
    p, q, g = (float(v) for v in params)
    n, m = np.asarray(n, np.float64), np.asarray(m, np.float64)
    den = p * n + q - 1.0
    with np.errstate(all="ignore"):
        return np.where(den > 0.0, p * (g + np.where(n == 0, 0.0, n * m)) / den, np.nan)


def exact_gg_customer(n, m, params):
    """(log L, grad[3] with respect to log(p, q, gamma), E[M | n, m]) as mpf."""
    mp = _mp()
    p, q, g = (mp.mpf(float(v)) for v in params)
    n, m = mp.mpf(int(n)), mp.mpf(float(m))
    a = p * n
    logL = (mp.loggamma(a + q) - mp.loggamma(a) - mp.loggamma(q) + q * mp.log(g) + (a - 1) * mp.log(m) + a * mp.log(n)
            - (a + q) * mp.log(g + n * m))
    gp = a * (mp.digamma(a + q) - mp.digamma(a) + mp.log(m) + mp.log(n) - mp.log(g + n * m))
    gq = q * (mp.digamma(a + q) - mp.digamma(q) + mp.log(g) - mp.log(g + n * m))
    gg = q - (a + q) * g / (g + n * m)
    return logL, [gp, gq, gg], p * (g + n * m) / (a + q - 1)


def exact_digamma(x):
    mp = _mp()
    return mp.digamma(mp.mpf(float(x)))


# ---------------------------------------------------------------------------------------------
# DERT
# ---------------------------------------------------------------------------------------------
U_SPLIT, D_SPAN = 4.0, 64.0


def gauss_legendre_header():
    """(x, w) of csrc/gauss_legendre.h: the doubles the device uses."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc_clv_model_amd", "csrc",
                        "gauss_legendre.h")
    with open(path) as f:
        text = f.read()
    x = text[text.index("CLV_GL_X_INIT"):text.index("CLV_GL_W_INIT")]
    w = text[text.index("CLV_GL_W_INIT"):]
    pat = r"-?0x[0-9a-f.]+p[+-]\d+"
    return (np.array([float.fromhex(t) for t in re.findall(pat, x)]),
            np.array([float.fromhex(t) for t in re.findall(pat, w)]))


def _gl16(lo, hi, f, X, W):
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    acc = 0.0
    for j in range(len(X)):
        acc += W[j] * f(mid + half * X[j])
    return acc * half


def model_dert_integral(s, B, delta, H):
    """J = int_0^H exp(-delta t) (B / (B + t))^s dt as csrc/pnbd.hip pnbd_dert_integral sums it (scalars)."""
    X, W = gauss_legendre_header()
    s, B, delta, H = float(s), float(B), float(delta), float(H)
    z, V = delta * B, H / B
    Y = math.inf if math.isinf(V) else math.log1p(V)
    yb = math.log(U_SPLIT / z) if 0.0 < z < U_SPLIT else (math.inf if z == 0.0 else 0.0)
    Yl = min(Y, yb)
    acc = 0.0
    if Yl > 0.0:
        npan = int(math.ceil(Yl / 0.5))
        wd = Yl / npan
        for k in range(npan):
            acc += _gl16(k * wd, Yl if k + 1 == npan else (k + 1) * wd,
                         lambda y: math.exp(-z * math.expm1(y) + (1.0 - s) * y), X, W)
    if Y > yb:
        d0 = U_SPLIT - z if z < U_SPLIT else 0.0
        d1 = min(z * V, d0 + D_SPAN)
        if d1 > d0:
            npan = int(math.ceil(d1 - d0))
            wd = (d1 - d0) / npan
            lin = 0.0
            for k in range(npan):
                lin += _gl16(d0 + k * wd, d1 if k + 1 == npan else d0 + (k + 1) * wd,
                             lambda d: math.exp(-d - s * math.log1p(d / z)), X, W)
            acc += lin / z
    return B * acc


def naive_dert_integral_inf(s, B, delta):
    """B e^z E_s(z) from the small-z series E_s(z) = Gamma(1 - s) z^(s-1) - sum_k (-z)^k / (k! (k + 1 - s)):
    what the device must not use (it cancels at s near an integer).  For the power check only."""
    z = delta * B
    tot = math.gamma(1.0 - s) * z ** (s - 1.0)
    term = 1.0
    for k in range(60):
        tot -= term / (k + 1.0 - s)
        term *= -z / (k + 1.0)
    return B * math.exp(z) * tot


def exact_dert_integral(s, B, delta, H):
    """mpmath quadrature of int_0^H exp(-delta t) (B / (B + t))^s dt, panels doubling from B / 64."""
    mp = _mp()
    s, B, d = mp.mpf(s), mp.mpf(B), mp.mpf(delta)
    Hm = mp.inf if math.isinf(float(H)) else mp.mpf(float(H))
    pts = [mp.mpf(0)]
    t = min(B, 1 / d if d > 0 else B) / 64
    while t < Hm and len(pts) < 80:
        pts.append(t)
        t *= 2
    pts.append(Hm)
    return mp.quad(lambda t: mp.exp(-d * t) * (B / (B + t)) ** s, pts)


def exact_dert_customer(x, tx, T, params4, delta, H):
    """(P(alive), DERT) of one customer at (r, alpha_i, s, beta_i) as mpf."""
    mp = _mp()
    r, a, s, b = (mp.mpf(float(v)) for v in params4)
    Tm = mp.mpf(float(T))
    _, A, sI = R._exact_parts(mp, int(x), mp.mpf(float(tx)), Tm, r, a, s, b)
    pa = A / (A + sI)
    return pa, pa * (r + int(x)) / (a + Tm) * exact_dert_integral(s, b + Tm, float(delta), H)


def model_dert_customers(x, tx, T, r, a, s, b, delta, H):
    m = model_customers_ab(x, tx, T, r, a, s, b)
    a, b = np.broadcast_to(a, np.shape(x)), np.broadcast_to(b, np.shape(x))
    J = np.array([model_dert_integral(s, b[i] + T[i], delta, H) for i in range(len(x))])
    return m["p_alive"], m["p_alive"] * (r + np.asarray(x, np.float64)) / (a + np.asarray(T, np.float64)) * J

"""Writes tests/golden/mle_ext_{cov,hessian,fit,gg,dert}.npz (a few KB each): inputs, exact values (mpmath,
tests/mle_ext_ref.py exact_*) and the measured error E_ref of the float64 numpy models, so the GPU tests
need neither mpmath nor a fit on the host.  Data only.

    python tests/golden/make_mle_ext_goldens.py [cov hessian fit gg dert]

Errors are relative to max(1, |value|); gradient sums and Hessian entries are scaled by max(1, sum_i
|term_i|).

mle_ext_cov      the 12 edge customers of pnbd_edge x 2 parameter sets (alpha0 < beta0 and swapped) with
                 K1 = 2, K2 = 1 and covariates that move alpha_i across beta_i within the frame.
mle_ext_hessian  a 24-row frame (the edge customers at two covariate values), a theta away from any optimum,
                 the exact Hessian, the scan of the central-difference step on the float64 model.
mle_ext_fit      the optima minimize_bfgs reaches with the numpy models: the covariate Pareto/NBD on abe with
                 first_sales_scaled on both processes (and its standard errors at HESSIAN_STEP), the
                 Gamma-Gamma on abe's spend observations.
mle_ext_gg       the Gamma-Gamma edge grid x 6 parameter sets, and a digamma grid.
mle_ext_dert     the DERT integral on s x z x H, and DERT end to end on the edge customers.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mle_ext_ref as M  # noqa: E402
from tests import pnbd_ref as R  # noqa: E402

T_STAR = 39.0
COV_PARAMS = np.array([
    # r, alpha0, s, beta0, gamma1 (two purchase columns, the second is all zeros), gamma2
    (0.8, 9.0, 1.7, 11.0, 0.9, 0.4, -0.6),     # alpha0 < beta0
    (0.8, 11.0, 1.7, 9.0, 0.9, 0.4, -0.6),     # swapped
])
HESS_THETA = np.array([np.log(0.9), np.log(7.0), np.log(1.3), np.log(9.0), 0.5, -0.4])
STEPS = 2.0 ** -np.arange(8, 25, 1.0)
INDEFINITE_THETA = np.array([np.log(20.0), np.log(0.05), np.log(8.0), np.log(300.0), 2.0, -2.0])   # far from any optimum


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def edge():
    e = np.load(os.path.join(HERE, "pnbd_edge.npz"))
    return e["x"], e["t_x"], e["T"]


def cov_frame(n):
    """z1 [2][n] (column 1 all zeros), z2 [1][n]: values in [-1, 1] that put alpha_i on both sides of beta_i."""
    z = np.linspace(-1.0, 1.0, n)
    return np.stack([z, np.zeros(n)]), (z[::-1] * 0.5)[None, :].copy()


def build_cov() -> dict:
    x, tx, T = edge()
    n, ns = len(x), len(COV_PARAMS)
    z1, z2 = cov_frame(n)
    P = COV_PARAMS.shape[1]
    out = dict(x=x, t_x=tx, T=T, z1=z1, z2=z2, params=COV_PARAMS, t_star=np.float64(T_STAR),
               logL=np.zeros((ns, n)), p_alive=np.zeros((ns, n)), ey=np.zeros((ns, n)), swap=np.zeros((ns, n), bool),
               grad_sum=np.zeros((ns, P)), grad_abs=np.zeros((ns, P)),
               eref_logL=np.zeros(ns), eref_p_alive=np.zeros(ns), eref_ey=np.zeros(ns), eref_grad=np.zeros(ns))
    for k, p in enumerate(COV_PARAMS):
        m = M.model_customers_cov(x, tx, T, p, z1, z2, T_STAR)
        assert m["converged"].all()
        out["swap"][k] = m["alpha"] < m["beta"]
        gs, ga = [0] * P, [0] * P
        for i in range(n):
            v = M.exact_customer_cov(x[i], tx[i], T[i], p, z1[:, i], z2[:, i], T_STAR)
            out["logL"][k, i], out["p_alive"][k, i], out["ey"][k, i] = (float(t) for t in v[:3])
            gs = [a + b for a, b in zip(gs, v[3])]
            ga = [a + abs(b) for a, b in zip(ga, v[3])]
        out["grad_sum"][k], out["grad_abs"][k] = [float(v) for v in gs], [float(v) for v in ga]
        for key in ("logL", "p_alive", "ey"):
            out["eref_" + key][k] = rel(m[key], out[key][k]).max()
        out["eref_grad"][k] = (np.abs(m["scores"].sum(0) - out["grad_sum"][k]) / np.maximum(1.0, out["grad_abs"][k])).max()
        assert out["swap"][k].any() and not out["swap"][k].all()      # both branches in one launch
    return out


def hessian_frame():
    x, tx, T = edge()
    x, tx, T = np.tile(x, 2), np.tile(tx, 2), np.tile(T, 2)
    z = np.repeat([-0.8, 0.7], 12)
    return x, tx, T, z[None, :].copy(), z[None, :].copy()


def build_hessian() -> dict:
    x, tx, T, z1, z2 = hessian_frame()
    H, Habs = M.exact_hessian_cov(x, tx, T, HESS_THETA, z1, z2)
    g = M.model_gradient_cov(x, tx, T, z1, z2)
    scale = np.maximum(1.0, Habs)
    scan = np.array([(np.abs(M.central_hessian(g, HESS_THETA, h) - H) / scale).max() for h in STEPS])
    eref = (np.abs(M.central_hessian(g, HESS_THETA, M.HESSIAN_STEP) - H) / scale).max()
    eig = np.linalg.eigvalsh(-M.central_hessian(g, INDEFINITE_THETA))
    assert eig.min() < -1.0 and eig.max() > 1.0               # indefinite by a margin no rounding closes
    return dict(x=x, t_x=tx, T=T, z1=z1, z2=z2, theta=HESS_THETA, hessian=H, hessian_abs=Habs, steps=STEPS,
                scan=scan, step=np.float64(M.HESSIAN_STEP), eref=np.float64(eref), indefinite_theta=INDEFINITE_THETA,
                indefinite_eig=eig)


def gg_rows(df):
    """The spend observation of the trivariate model: n = x + 1 transactions with mean sales / (x + 1)."""
    n = df["x"].to_numpy() + 1
    m = df["sales"].to_numpy() / n
    keep = m > 0
    return n[keep], m[keep]


def build_fit() -> dict:
    from mcmc_clv_model_amd.mle import GammaGammaFitter, ParetoNBDFitter, delta_standard_errors
    from tests.helpers import cdnow
    df = cdnow("abe")
    x, tx, T = df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy()
    z = df["first_sales_scaled"].to_numpy()[None, :].copy()
    names = ["r", "alpha", "s", "beta", "purchase:first_sales_scaled", "dropout:first_sales_scaled"]
    f = ParetoNBDFitter().fit_objective(M.model_value_and_grad_cov(x, tx, T, z, z), [1, 1, 1, 1, 0, 0], names=names)
    assert f.converged_
    p = f.params_.to_numpy()
    ll = float(M.model_customers_cov(x, tx, T, p, z, z)["logL"].sum())
    theta = np.concatenate([np.log(p[:4]), p[4:]])
    H = M.central_hessian(M.model_gradient_cov(x, tx, T, z, z), theta)
    se = delta_standard_errors(theta, np.linalg.inv(-H), 4)
    n, m = gg_rows(df)
    g = GammaGammaFitter().fit_objective(M.model_gg_value_and_grad(n, m), [1, 1, 1])
    assert g.converged_
    q = g.params_.to_numpy()
    return dict(cov_params=p, cov_logL=np.float64(ll), cov_hessian=H, cov_se=se, gg_params=q,
                gg_logL=np.float64(M.model_gg_customers(n, m, q)["logL"].sum()), gg_n=np.int64(len(n)))


GG_N = np.repeat([1, 2, 17, 2000], 4)
GG_M = np.tile([1e-3, 1.0, 35.0, 1e5], 4)
GG_PARAMS = np.array([
    (6.25, 3.74, 15.44),          # CDNOW-like (Fader & Hardie 2013)
    (0.05, 3.0, 10.0),            # p = 0.05
    (300.0, 200.0, 1e4),          # large: p n up to 6e5
    (2.0, 1.0 + 2.0 ** -20, 5.0),   # q just above 1: the conditional mean's denominator at n = 0
    (2.0, 3.0, 1e-6),             # gamma far below n m
    (2.0, 3.0, 1e8),              # gamma far above n m
])
GG_HEAVY = GG_N == 2000           # the heavy-buyer rows; the others are the easy ones


def build_gg() -> dict:
    ns, nc = len(GG_PARAMS), len(GG_N)
    out = dict(n=GG_N.astype(np.int32), m=GG_M, params=GG_PARAMS, heavy=GG_HEAVY, logL=np.zeros((ns, nc)),
               grad=np.zeros((ns, nc, 3)), mean=np.zeros((ns, nc)), eref_logL=np.zeros(ns), eref_grad=np.zeros(ns),
               eref_mean=np.zeros(ns), eref_logL_heavy=np.zeros(ns), eref_logL_easy=np.zeros(ns),
               eref_grad_heavy=np.zeros(ns), eref_grad_easy=np.zeros(ns))
    for k, p in enumerate(GG_PARAMS):
        for i in range(nc):
            v = M.exact_gg_customer(GG_N[i], GG_M[i], p)
            out["logL"][k, i], out["mean"][k, i] = float(v[0]), float(v[2])
            out["grad"][k, i] = [float(t) for t in v[1]]
        c = M.model_gg_customers(GG_N, GG_M, p)
        eL, eG = rel(c["logL"], out["logL"][k]), rel(c["grad"], out["grad"][k]).max(1)
        out["eref_logL"][k], out["eref_grad"][k] = eL.max(), eG.max()
        out["eref_mean"][k] = rel(M.model_gg_mean(GG_N, GG_M, p), out["mean"][k]).max()
        out["eref_logL_heavy"][k], out["eref_logL_easy"][k] = eL[GG_HEAVY].max(), eL[~GG_HEAVY].max()
        out["eref_grad_heavy"][k], out["eref_grad_easy"][k] = eG[GG_HEAVY].max(), eG[~GG_HEAVY].max()
    xs = np.concatenate([np.logspace(-3, 6, 46), [2.0 ** -40, 1e-300, 1.4616321449683622, 9.999999999, 10.0, 31.9, 32.0]])
    psi = np.array([float(M.exact_digamma(v)) for v in xs])
    out.update(psi_x=xs, psi=psi, eref_psi=np.float64(rel(M.model_digamma(xs), psi).max()))
    return out


DERT_S = np.array([0.3, 0.606, 1.0 - 2.0 ** -30, 1.0, 1.0 + 2.0 ** -30, 2.0, 2.5, 7.0])
DERT_Z = np.array([1e-4, 0.0137, 0.14, 1.0, 30.0])
DERT_H = np.array([np.inf, 1e-3, 52.0, 520.0])
DERT_B = 50.67                         # beta + T of a CDNOW customer; delta = z / B
DERT_CUST = np.array([(0.8, 5.0, 1.7, 14.0), (0.55, 10.58, 1.0, 11.67)])   # s = 1 exactly in the second
DERT_DELTA = float(np.log1p(0.15) / 52.0)


def build_dert() -> dict:
    s, z, H = (a.reshape(-1) for a in np.meshgrid(DERT_S, DERT_Z, DERT_H, indexing="ij"))
    B = np.full(s.shape, DERT_B)
    delta = z / B
    J = np.array([float(M.exact_dert_integral(*v)) for v in zip(s, B, delta, H)])
    mod = np.array([M.model_dert_integral(*v) for v in zip(s, B, delta, H)])
    err = rel(mod, J)
    integer = np.isin(s, [1.0, 2.0, 7.0]) | (np.abs(s - 1.0) < 1e-6)
    x, tx, T = edge()
    nc = len(x)
    dert = np.zeros((len(DERT_CUST), 2, nc))
    pal = np.zeros((len(DERT_CUST), nc))
    eref_c = np.zeros(len(DERT_CUST))
    for k, p in enumerate(DERT_CUST):
        for j, Hh in enumerate((np.inf, 52.0)):
            for i in range(nc):
                pa, d = M.exact_dert_customer(x[i], tx[i], T[i], p, DERT_DELTA, Hh)
                dert[k, j, i], pal[k, i] = float(d), float(pa)
            _, md = M.model_dert_customers(x, tx, T, p[0], p[1], p[2], p[3], DERT_DELTA, Hh)
            eref_c[k] = max(eref_c[k], rel(md, dert[k, j]).max())
    return dict(s=s, B=B, delta=delta, H=H, J=J, eref=np.float64(err.max()), eref_integer=np.float64(err[integer].max()),
                eref_easy=np.float64(err[~integer].max()), integer=integer, x=x, t_x=tx, T=T, cust_params=DERT_CUST,
                cust_delta=np.float64(DERT_DELTA), cust_H=np.array([np.inf, 52.0]), cust_dert=dert, cust_p_alive=pal,
                eref_cust=eref_c)


BUILDERS = dict(cov=build_cov, hessian=build_hessian, fit=build_fit, gg=build_gg, dert=build_dert)

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(BUILDERS)):
        out = BUILDERS[name]()
        path = os.path.join(HERE, f"mle_ext_{name}.npz")
        np.savez(path, **out)
        print(name, os.path.getsize(path), "bytes")
        for key in sorted(out):
            if key.startswith("eref") or key in ("scan", "steps", "cov_params", "cov_logL", "cov_se", "gg_params", "gg_logL"):
                print("  ", key, out[key])

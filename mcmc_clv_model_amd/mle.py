"""The classical Pareto/NBD fitted by maximum likelihood: the reference's MLE baseline.

Drop-in for what the reference uses of ``lifetimes`` (bivariate/analysis_abe.py:205-217, :426-438;
full_analysis.py:245, :437):

    from mcmc_clv_model_amd.mle import ParetoNBDFitter
    pnbd_mle = ParetoNBDFitter(penalizer_coef=0.0)
    pnbd_mle.fit(frequency=cbs["x"], recency=cbs["t_x"], T=cbs["T_cal"])
    pnbd_mle.conditional_expected_number_of_purchases_up_to_time(t_star, cbs["x"], cbs["t_x"], cbs["T_cal"])
    pnbd_mle.expected_number_of_purchases_up_to_time(rel_t)

The likelihood, its analytic gradient and the per-customer quantities are HIP kernels
(csrc/pnbd.hip, one lane per customer, fixed-order sums); the optimiser is a small numpy BFGS on
theta = log(r, alpha, s, beta).  There is no CPU fallback for the likelihood.  DESIGN.md §4e.

The rest of the classical baseline:

    pnbd_mle.fit(..., covariates=cbs[["first_sales_scaled"]], standard_errors=True)   # Fader & Hardie (2007)
    pnbd_mle.summary_; likelihood_ratio_test(plain_fit, pnbd_mle)
    gg = GammaGammaFitter().fit(frequency=n, monetary_value=m)                        # spend per transaction
    pnbd_mle.discounted_expected_transactions(cbs["x"], cbs["t_x"], cbs["T_cal"], discount_rate=0.15)
    classical_lifetime_value(pnbd_mle, gg, cbs, monetary_frequency=n, monetary_value=m)

alpha_i = alpha0 exp(-gamma1' z_i) and beta_i = beta0 exp(-gamma2' z_i) are formed on the device per
customer (the covariates stay in the handle); the Hessian is a central difference of the device
gradient; the Gamma-Gamma likelihood (csrc/gg.hip) and the DERT integral are HIP kernels too.
"""
from __future__ import annotations

import contextlib
import ctypes
import warnings
from types import SimpleNamespace
from typing import Callable, Optional

import numpy as np
import pandas as pd

from . import _lib
from ._lib import check, dptr

PARAM_NAMES = ("r", "alpha", "s", "beta")


# ---------------------------------------------------------------------------------------------
# Optimiser
# ---------------------------------------------------------------------------------------------
def minimize_bfgs(value_and_grad: Callable, theta0, tol: float = 1e-7, max_iter: int = 200):
    """BFGS with Armijo backtracking, numpy only.  ``value_and_grad(theta) -> (f, g)``; a
    non-finite f or g is a failed trial step and is backtracked.  Stops when max |g| <= tol.
    Returns a namespace: x, fun, grad, grad_norm, converged, n_iter, n_eval, message."""
    theta = np.array(theta0, np.float64)
    d = theta.size
    n_eval = 0

    def ev(t):
        nonlocal n_eval
        n_eval += 1
        f, g = value_and_grad(t)
        g = np.asarray(g, np.float64)
        return float(f), g, bool(np.isfinite(f) and np.isfinite(g).all())

    f, g, ok = ev(theta)
    res = SimpleNamespace(x=theta, fun=f, grad=g, grad_norm=float(np.max(np.abs(g))) if ok else np.inf,
                          converged=False, n_iter=0, n_eval=n_eval, message="")
    if not ok:
        res.message = "the objective is not finite at the starting point"
        return res
    H = np.eye(d)
    fresh = True                      # H is the identity: a failed line search has nothing to reset
    for it in range(1, max_iter + 1):
        if np.max(np.abs(g)) <= tol:
            res.converged, res.message = True, "gradient tolerance met"
            break
        p = -H @ g
        slope = float(g @ p)
        if not slope < 0.0:
            H, fresh = np.eye(d), True
            p, slope = -g, -float(g @ g)
        step = min(1.0, 1.0 / np.max(np.abs(p))) if fresh else 1.0
        found = False
        while step >= 1e-12:
            tn = theta + step * p
            fn, gn, okn = ev(tn)
            if okn and fn <= f + 1e-4 * step * slope:
                found = True
                break
            step *= 0.5
        res.n_iter = it
        if not found:
            if fresh:
                res.message = "line search failed along the steepest descent direction"
                break
            H, fresh = np.eye(d), True
            continue
        s, y = tn - theta, gn - g
        sy = float(s @ y)
        if sy > 1e-10 * np.sqrt(float(s @ s) * float(y @ y)):
            if fresh:
                H = np.eye(d) * (sy / float(y @ y))
            rho = 1.0 / sy
            V = np.eye(d) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
            fresh = False
        theta, f, g = tn, fn, gn
    else:
        if np.max(np.abs(g)) <= tol:
            res.converged, res.message = True, "gradient tolerance met"
        else:
            res.message = f"max_iter = {max_iter} iterations without meeting tol"
    res.x, res.fun, res.grad, res.grad_norm, res.n_eval = theta, f, g, float(np.max(np.abs(g))), n_eval
    return res


def minimize_bfgs_score(value_and_grad: Callable, theta0, tol: float = 1e-7, max_iter: int = 200, *,
                        curvature: float = 0.9, value_slack: float = 1e-3, max_line_steps: int = 30):
    """BFGS whose line search is decided by the score, for an objective whose gradient is not exactly
    the derivative of its value (the fixed-node score of a quadrature): along the
    direction p a step t is accepted when the directional derivative has shrunk,
    |g(theta + t p)' p| <= curvature |g(theta)' p| (the strong Wolfe curvature condition, which also makes
    the BFGS update positive definite); a positive derivative brackets the root and the next trial
    is the secant root of the derivative, a still steep negative one doubles the step.  The value is
    a sanity bound only: a trial that is not finite or whose value exceeds f + value_slack max(1, |f|)
    is too far and the step is halved towards the last good one.  Stops when max |g| <= tol: the
    result is the root of the score.  Same namespace as :func:`minimize_bfgs`."""
    theta = np.array(theta0, np.float64)
    d = theta.size
    n_eval = 0

    def ev(t):
        nonlocal n_eval
        n_eval += 1
        f, g = value_and_grad(t)
        g = np.asarray(g, np.float64)
        return float(f), g, bool(np.isfinite(f) and np.isfinite(g).all())

    f, g, ok = ev(theta)
    res = SimpleNamespace(x=theta, fun=f, grad=g, grad_norm=float(np.max(np.abs(g))) if ok else np.inf,
                          converged=False, n_iter=0, n_eval=n_eval, message="")
    if not ok:
        res.message = "the objective is not finite at the starting point"
        return res
    H = np.eye(d)
    fresh = True
    for it in range(1, max_iter + 1):
        if np.max(np.abs(g)) <= tol:
            res.converged, res.message = True, "score tolerance met"
            break
        p = -H @ g
        slope = float(g @ p)
        if not slope < 0.0:
            H, fresh = np.eye(d), True
            p, slope = -g, -float(g @ g)
        t = min(1.0, 1.0 / np.max(np.abs(p))) if fresh else 1.0
        lo, dlo, hi, dhi = 0.0, slope, None, None     # the derivative along p is negative at lo
        found = False
        for _ in range(max_line_steps):
            tn = theta + t * p
            fn, gn, okn = ev(tn)
            if not okn or fn > f + value_slack * max(1.0, abs(f)):
                hi, dhi = t, None
            else:
                dn = float(gn @ p)
                if abs(dn) <= curvature * abs(slope):
                    found = True
                    break
                if dn > 0.0:
                    hi, dhi = t, dn
                else:
                    lo, dlo = t, dn
            if hi is None:
                t = 2.0 * t
            elif dhi is None:
                t = 0.5 * (lo + hi)
            else:
                t = lo + (hi - lo) * (-dlo) / (dhi - dlo)
                t = min(max(t, lo + 0.1 * (hi - lo)), hi - 0.1 * (hi - lo))
        res.n_iter = it
        if not found:
            if fresh:
                res.message = "line search failed along the steepest descent direction"
                break
            H, fresh = np.eye(d), True
            continue
        s, y = tn - theta, gn - g
        sy = float(s @ y)
        if sy > 1e-10 * np.sqrt(float(s @ s) * float(y @ y)):
            if fresh:
                H = np.eye(d) * (sy / float(y @ y))
            rho = 1.0 / sy
            V = np.eye(d) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
            fresh = False
        theta, f, g = tn, fn, gn
    else:
        if np.max(np.abs(g)) <= tol:
            res.converged, res.message = True, "score tolerance met"
        else:
            res.message = f"max_iter = {max_iter} iterations without meeting tol"
    res.x, res.fun, res.grad, res.grad_norm, res.n_eval = theta, f, g, float(np.max(np.abs(g))), n_eval
    return res


# ---------------------------------------------------------------------------------------------
# Uncertainty of a fit: Hessian by central differences of the gradient, Wald summary, tests
# ---------------------------------------------------------------------------------------------
# The step of central_hessian on theta (logs of the positive parameters, coefficients as they are).
# The device gradient is good to about 1e-14 of sum |terms|, so rounding is about 1e-14 / h and
# truncation about h^2: tests/golden/make_mle_ext_goldens.py scans h against the exact Hessian
# (DESIGN.md §4m): the error is smallest, 2e-10 of sum |terms|, at 2^-15.
HESSIAN_STEP = 2.0 ** -15


def central_hessian(grad: Callable, theta, step: float = HESSIAN_STEP) -> np.ndarray:
    """The Jacobian of ``grad`` at theta by central differences, column j = (grad(theta + h e_j) -
    grad(theta - h e_j)) / 2h, then symmetrised: 2 P gradient evaluations."""
    theta = np.asarray(theta, np.float64).reshape(-1)
    h = float(step)
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError("step must be positive and finite")
    P = theta.size
    H = np.empty((P, P))
    for j in range(P):
        e = np.zeros(P)
        e[j] = h
        up, dn = theta + e, theta - e
        H[:, j] = (np.asarray(grad(up), np.float64) - np.asarray(grad(dn), np.float64)) / (up[j] - dn[j])
    return 0.5 * (H + H.T)


def chi2_sf(x, df: int) -> float:
    """P(chi2_df > x) from erfc and exp alone: Q(1/2, y) = erfc(sqrt y), Q(1, y) = exp(-y) and
    Q(a + 1, y) = Q(a, y) + y^a e^-y / Gamma(a + 1) with y = x / 2, a = df / 2: positive terms only."""
    import math
    df = int(df)
    if df < 1:
        raise ValueError("df must be a positive integer")
    x = float(x)
    if math.isnan(x):
        return float("nan")
    if x <= 0.0:
        return 1.0
    y = 0.5 * x
    if df % 2:
        a, q = 0.5, math.erfc(math.sqrt(y))
    else:
        a, q = 1.0, math.exp(-y)
    while a < 0.5 * df - 0.25:
        q += math.exp(a * math.log(y) - y - math.lgamma(a + 1.0))
        a += 1.0
    return min(q, 1.0)


def likelihood_ratio_test(restricted, full) -> dict:
    """2 (log L_full - log L_restricted) against chi2 with df = the difference in parameter counts.
    Both are fitted models (``log_likelihood_`` and ``params_``) of which ``restricted`` is nested in
    ``full``; returns dict(statistic, df, p_value)."""
    ll0, ll1 = float(restricted.log_likelihood_), float(full.log_likelihood_)
    df = len(full.params_) - len(restricted.params_)
    if df < 1:
        raise ValueError("the full model must have more parameters than the restricted one")
    stat = 2.0 * (ll1 - ll0)
    return dict(statistic=stat, df=int(df), p_value=chi2_sf(stat, df))


def delta_standard_errors(theta, cov_theta, n_log: int) -> np.ndarray:
    """Standard errors on the natural scale from the covariance of theta: exp(theta_j) se(theta_j)
    for the first n_log (log-scale) entries by the delta method, se(theta_j) for the rest."""
    theta = np.asarray(theta, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diag(np.asarray(cov_theta, np.float64)))
    out = se.copy()
    out[:n_log] = np.exp(theta[:n_log]) * se[:n_log]
    return out


_Z975 = 1.959963984540054          # the 0.975 quantile of the standard normal


def wald_summary(theta, cov_theta, names, n_log: int) -> pd.DataFrame:
    """estimate, se, z, p and the 95 % Wald interval per parameter.  The first n_log parameters are
    positive and theta holds their logs: their row is built on the log scale (z = theta / se(theta),
    which tests the parameter against 1; interval exp(theta -+ 1.96 se(theta))) and reports estimate
    and se on the natural scale (delta method).  The other rows are direct: z tests against 0."""
    import math
    theta = np.asarray(theta, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        se_t = np.sqrt(np.diag(np.asarray(cov_theta, np.float64)))
    est = theta.copy()
    est[:n_log] = np.exp(theta[:n_log])
    with np.errstate(invalid="ignore", divide="ignore"):
        z = theta / se_t
    p = np.array([math.erfc(abs(v) / math.sqrt(2.0)) if np.isfinite(v) else np.nan for v in z])
    lo, hi = theta - _Z975 * se_t, theta + _Z975 * se_t
    lo[:n_log], hi[:n_log] = np.exp(lo[:n_log]), np.exp(hi[:n_log])
    return pd.DataFrame(dict(estimate=est, se=delta_standard_errors(theta, cov_theta, n_log), z=z, p=p,
                             ci_lower=lo, ci_upper=hi), index=list(names))


class _WaldMixin:
    """What ParetoNBDFitter and GammaGammaFitter share: the optimiser half of fit(), and covariance_,
    standard_errors_ and summary_ from the Hessian of sum w log L in theta.  The ``_N_LOG`` leading
    parameters (``_NAMES``) are positive and optimised on their logs; a fitter adds
    ``_gradient(data)``, theta -> d sum w log L / d theta on the device."""
    _N_LOG = 0
    _NAMES = ()

    def _theta_names(self):
        names = list(self.params_.index)
        return [f"log {n}" for n in names[:self._N_LOG]] + names[self._N_LOG:]

    def _theta(self) -> np.ndarray:
        t = self.params_.to_numpy(dtype=np.float64).copy()
        t[:self._N_LOG] = np.log(t[:self._N_LOG])
        return t

    def _natural(self, theta) -> np.ndarray:
        """The parameters of theta: exp of its first _N_LOG entries, the rest as they are."""
        return np.concatenate([np.exp(theta[:self._N_LOG]), theta[self._N_LOG:]])

    def _fitted(self) -> np.ndarray:
        if self.params_ is None:
            raise RuntimeError("fit() has not been called")
        return self.params_.to_numpy(dtype=np.float64)

    def _fit_objective(self, value_and_grad: Callable, initial_params, tol: float, max_iter: int, names=None):
        """fit_objective of both fitters (their caller's caller gets the warning)."""
        names = list(self._NAMES if names is None else names)
        p0 = np.asarray(initial_params, np.float64).reshape(len(names))
        L = self._N_LOG
        res = minimize_bfgs(value_and_grad, np.concatenate([np.log(p0[:L]), p0[L:]]), tol, max_iter)
        self.params_ = pd.Series(self._natural(res.x), index=names)
        self.converged_ = bool(res.converged)
        self.n_iter_, self.n_eval_ = int(res.n_iter), int(res.n_eval)
        self.grad_norm_ = float(res.grad_norm)
        self.message_ = res.message
        if not res.converged:
            warnings.warn(f"{type(self).__name__} did not converge: {res.message} "
                          f"(max |gradient| = {res.grad_norm:.3g} after {res.n_eval} evaluations)", RuntimeWarning,
                          stacklevel=4)
        return self

    def _uncertainty(self, data, robust: bool, theta=None, step: float = HESSIAN_STEP):
        theta = self._theta() if theta is None else theta
        H = central_hessian(self._gradient(data), theta, step)
        return self._set_uncertainty(H, data.scores(self._natural(theta)) if robust else None, theta)

    def _set_uncertainty(self, H, scores=None, theta=None):
        """covariance_ = (-H)^-1 on theta, or the sandwich H^-1 (sum s_i s_i') H^-1 with ``scores``
        [N][P].  A -H that is not positive definite: NaN everywhere and one RuntimeWarning."""
        H = np.asarray(H, np.float64)
        P = H.shape[0]
        theta, names = self._theta() if theta is None else np.asarray(theta, np.float64), self._theta_names()
        cov = np.full((P, P), np.nan)
        ok = bool(np.isfinite(H).all())
        if ok:
            try:
                np.linalg.cholesky(-H)
            except np.linalg.LinAlgError:
                ok = False
        if ok:
            cov = np.linalg.inv(-H)
            if scores is not None:
                S = np.asarray(scores, np.float64)
                cov = cov @ (S.T @ S) @ cov
            cov = 0.5 * (cov + cov.T)
        else:
            warnings.warn(f"{type(self).__name__}: the Hessian of the log-likelihood is not negative definite "
                          "(a boundary or a fit that did not converge): the standard errors are NaN",
                          RuntimeWarning, stacklevel=3)
        self.hessian_ = H
        self.covariance_ = pd.DataFrame(cov, index=names, columns=names)
        self.standard_errors_ = pd.Series(delta_standard_errors(theta, cov, self._N_LOG), index=list(self.params_.index))
        self.summary_ = wald_summary(theta, cov, list(self.params_.index), self._N_LOG)
        return self


# ---------------------------------------------------------------------------------------------
# Device handle
# ---------------------------------------------------------------------------------------------
MAX_COVARIATES = 8
# How the likelihood's integral I is evaluated (clv_pnbd_set_integral): the series for every
# customer (the default; NaN and a count past its 2,048-term cap), the series up to z(t_x) = 0.9 and the
# quadrature of I itself past it, or the quadrature for every customer with t_x < T.
INTEGRAL_MODES = {"series": 0, "auto": 1, "quadrature": 2}


def integral_mode(integral) -> int:
    """The C enum of ``integral``; ValueError for anything but "series", "auto" and "quadrature"."""
    if not isinstance(integral, str) or integral not in INTEGRAL_MODES:
        raise ValueError(f"integral must be one of {tuple(INTEGRAL_MODES)}; got {integral!r}")
    return INTEGRAL_MODES[integral]


class _Handle:
    """A handle of the C library (``_h``, freed by the entry ``_DESTROY`` of ``_L``): closed by close(),
    on leaving its ``with`` block and when collected."""
    _DESTROY = ""

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._DESTROY)(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def covariate_matrix(cov, n: int, what: str = "covariates", names=None):
    """(z [K][n] C-contiguous float64, names) of an (n, K) array or DataFrame: the device layout, a
    covariate per row.  ValueError on a wrong shape, more than 8 columns or a non-finite value."""
    cols = None
    if isinstance(cov, pd.DataFrame):
        cols = [str(c) for c in cov.columns]
        a = cov.to_numpy(dtype=np.float64)
    else:
        a = np.asarray(cov, dtype=np.float64)
        if a.ndim == 1 and a.size == n and n > 0:
            a = a.reshape(n, 1)
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError(f"{what} must have shape (N, K) with N = {n} customers; got {a.shape}")
    K = a.shape[1]
    if K > MAX_COVARIATES:
        raise ValueError(f"{what}: at most {MAX_COVARIATES} columns per process; got {K}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite")
    if names is not None:
        names = [str(c) for c in names]
        if len(names) != K:
            raise ValueError(f"{what}: {len(names)} names for {K} columns")
    else:
        names = cols if cols is not None else [f"z{k}" for k in range(K)]
    return np.ascontiguousarray(a.T), names


def _cov_pair(covariates, covariates_dropout, n: int, names=None):
    """((z1, names1), (z2, names2)); the dropout process takes the purchase matrix unless it has its own."""
    z1, n1 = covariate_matrix(covariates, n, "covariates", names)
    if covariates_dropout is None:
        return (z1, n1), (z1, list(n1))
    same = not isinstance(covariates_dropout, pd.DataFrame) and names is not None and \
        np.ndim(covariates_dropout) == 2 and np.shape(covariates_dropout)[1] == len(n1)
    return (z1, n1), covariate_matrix(covariates_dropout, n, "covariates_dropout", names if same else None)


class PnbdData(_Handle):
    """The CBS columns resident on the device for the evaluations of a fit (clv_pnbd_create)."""
    _DESTROY = "clv_pnbd_destroy"

    def __init__(self, frequency, recency, T, weights=None, *, device: int = -1, covariates=None,
                 covariates_dropout=None, integral: str = "series"):
        mode = integral_mode(integral)    # ValueError before the library is loaded
        self.integral = "series"
        self.k1 = self.k2 = None          # None: no covariates in the handle
        cov = None
        if covariates is not None:
            cov = _cov_pair(covariates, covariates_dropout, int(np.asarray(frequency).reshape(-1).shape[0]))
        elif covariates_dropout is not None:
            raise ValueError("covariates_dropout without covariates: pass covariates with zero columns")
        L = _lib.lib()
        if _lib.device_count() < 1:
            raise _lib.ClvError("no HIP device visible; the Pareto/NBD likelihood has no CPU fallback")
        f = np.asarray(frequency)
        ff = np.asarray(f, np.float64)
        if f.size and not np.all(ff == np.round(ff)):
            raise ValueError("frequency must hold integer repeat counts")
        if f.size and (ff.max() > 2 ** 31 - 1 or ff.min() < -2 ** 31):
            raise ValueError("frequency exceeds int32")
        self.x = np.ascontiguousarray(f, dtype=np.int32).reshape(-1)
        self.t_x = np.ascontiguousarray(np.asarray(recency, np.float64).reshape(-1))
        self.T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1))
        self.n = int(self.x.shape[0])
        if self.t_x.shape[0] != self.n or self.T.shape[0] != self.n:
            raise ValueError("frequency, recency and T must have the same length")
        self.w = None
        if weights is not None:
            self.w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
            if self.w.shape[0] != self.n:
                raise ValueError("weights must have the length of frequency")
        self._L = L
        self._h = ctypes.c_void_p()
        check(L.clv_pnbd_create(int(device), self.n, self.x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                dptr(self.t_x), dptr(self.T), dptr(self.w), ctypes.byref(self._h)))
        try:
            if mode != INTEGRAL_MODES["series"]:
                self.set_integral(integral)
            if cov is not None:
                self.set_covariates(cov[0][0], cov[1][0])
        except Exception:
            self.close()
            raise

    def set_integral(self, integral: str):
        """How every later evaluation of this handle forms I: "series", "auto" or "quadrature"
        (clv_pnbd_set_integral)."""
        check(self._L.clv_pnbd_set_integral(self._h, integral_mode(integral)))
        self.integral = integral

    def set_covariates(self, z1, z2):
        """Covariates into the handle (clv_pnbd_set_covariates): z1 [K1][n] for the purchase process,
        z2 [K2][n] for the dropout process, a covariate per row."""
        z1 = np.ascontiguousarray(np.asarray(z1, np.float64).reshape(-1, self.n))
        z2 = np.ascontiguousarray(np.asarray(z2, np.float64).reshape(-1, self.n))
        check(self._L.clv_pnbd_set_covariates(self._h, z1.shape[0], dptr(z1) if z1.size else None, z2.shape[0],
                                              dptr(z2) if z2.size else None))
        self.k1, self.k2 = int(z1.shape[0]), int(z2.shape[0])
        self.z1, self.z2 = z1, z2

    def _params(self, params, cov: bool) -> np.ndarray:
        """params as a plain entry takes them (4) or, ``cov``, a covariate entry (4 + K1 + K2; a handle
        without covariates is given K1 = K2 = 0 first)."""
        if cov and self.k1 is None:
            self.set_covariates(np.empty((0, self.n)), np.empty((0, self.n)))
        k = self.k1 + self.k2 if cov else 0
        return np.ascontiguousarray(np.asarray(params, np.float64).reshape(4 + k))

    def _evaluate(self, params, cov: bool):
        """(sums, n_unconverged) of clv_pnbd_eval or, ``cov``, clv_pnbd_eval_cov."""
        p = self._params(params, cov)
        sums = np.empty(p.size + 2)
        nu = ctypes.c_int64(0)
        entry = self._L.clv_pnbd_eval_cov if cov else self._L.clv_pnbd_eval
        check(entry(self._h, dptr(p), dptr(sums), ctypes.byref(nu)))
        return sums, int(nu.value)

    def _per_customer(self, entry: str, width: int, params, cov: bool, *args) -> np.ndarray:
        """[n][width] of the per-customer entry ``entry(handle, params, *args, out)``."""
        p = self._params(params, cov)
        out = np.empty((self.n, width))
        check(getattr(self._L, entry)(self._h, dptr(p), *args, dptr(out)))
        return out

    def eval_cov(self, params):
        """(sums[6 + K1 + K2], n_unconverged) at params = (r, alpha0, s, beta0, gamma1, gamma2): the six
        sums of :meth:`eval`, then d sum w log L / d gamma1 and / d gamma2 (clv_pnbd_eval_cov).  A handle
        without covariates takes K1 = K2 = 0."""
        return self._evaluate(params, True)

    def customers_cov(self, params, t_star: float = 0.0) -> np.ndarray:
        """[n][7]: log L, P(alive), E[Y(t_star) | x, t_x, T, z] and the score with respect to
        log(r, alpha_i, s, beta_i) (clv_pnbd_customers_cov)."""
        return self._per_customer("clv_pnbd_customers_cov", 7, params, True, float(t_star))

    def scores(self, params) -> np.ndarray:
        """[n][4 + K1 + K2]: w_i d log L_i / d theta, theta = (log r, log alpha0, log s, log beta0,
        gamma1, gamma2), from the per-customer score of :meth:`customers_cov` by the chain rule."""
        g = self.customers_cov(params)[:, 3:7]
        s = np.concatenate([g, -self.z1.T * g[:, 1:2], -self.z2.T * g[:, 3:4]], axis=1)
        return s if self.w is None else s * self.w[:, None]

    def dert(self, params, delta: float, horizon: float) -> np.ndarray:
        """[n][2]: P(alive) and the discounted expected residual transactions (clv_pnbd_dert)."""
        return self._per_customer("clv_pnbd_dert", 2, params, self.k1 is not None, float(delta), float(horizon))

    def eval(self, params):
        """(sums[6], n_unconverged): sum w log L, its derivatives with respect to
        log(r, alpha, s, beta), sum w; customers whose series hit the term cap (sums[0] is NaN then; in
        the modes "auto" and "quadrature": customers with a result that is not finite)."""
        return self._evaluate(params, False)

    def customers(self, params, t_star: float = 0.0) -> np.ndarray:
        """[n][3]: log L, P(alive), E[Y(t_star) | x, t_x, T]."""
        return self._per_customer("clv_pnbd_customers", 3, params, False, float(t_star))


def phi(k: float, ell):
    """-expm1(-k ell) / k, and ell at k = 0."""
    ell = np.asarray(ell, np.float64)
    return ell.copy() if k == 0.0 else -np.expm1(-k * ell) / k


# ---------------------------------------------------------------------------------------------
# Fitter
# ---------------------------------------------------------------------------------------------
class ParetoNBDFitter(_WaldMixin):
    """Pareto/NBD by maximum likelihood (Schmittlein, Morrison & Colombo 1987; the likelihood as in
    Fader & Hardie 2005).  ``penalizer_coef`` adds penalizer_coef * sum(params^2) to the
    per-customer mean negative log-likelihood.

    With ``covariates`` the model is Fader & Hardie (2007)'s: alpha_i = alpha0 exp(-gamma1' z_i),
    beta_i = beta0 exp(-gamma2' z_i); ``params_`` then holds r, alpha (= alpha0), s, beta (= beta0),
    ``purchase:<name>`` per column of ``covariates`` and ``dropout:<name>`` per column of
    ``covariates_dropout`` (the same matrix unless given), and the penalty gains
    penalizer_coef * sum(gamma^2).

    ``integral`` is how every device evaluation of this fitter forms the likelihood's integral I
    (DESIGN.md §4o): "series" (the default: a customer past the series' term cap, z of about 0.98, is
    NaN and counted in ``n_unconverged_``), "auto" (the series with the same bits up to z(t_x) = 0.9, a
    quadrature of I itself past it: what a covariate that moves alpha_i / beta_i by orders of magnitude
    needs) or "quadrature" (the quadrature for every customer)."""
    _N_LOG = 4
    _NAMES = PARAM_NAMES

    def __init__(self, penalizer_coef: float = 0.0, *, integral: str = "series"):
        integral_mode(integral)
        self.integral = integral
        self.penalizer_coef = float(penalizer_coef)
        self.params_: Optional[pd.Series] = None
        self._device = -1
        self._k = None                # (K1, K2) of a covariate fit
        self._shared_dropout = True

    def _objective(self, data: PnbdData, cov: bool = False):
        """theta -> (penalised mean negative log-likelihood, its gradient) from clv_pnbd_eval, or ``cov``
        from clv_pnbd_eval_cov: the plain model is the covariate model without trailing coefficients."""
        pen = self.penalizer_coef
        evaluate = data.eval_cov if cov else data.eval

        def f(theta):
            with np.errstate(over="ignore"):
                p = self._natural(theta)
            if not (np.isfinite(p).all() and (p[:4] > 0.0).all()):
                return np.nan, np.full(theta.size, np.nan)
            sums, _ = evaluate(p)
            val = -sums[0] / sums[5] + pen * float((p ** 2).sum())
            g = -np.concatenate([sums[1:5], sums[6:]]) / sums[5]
            g[:4] += 2.0 * pen * p[:4] ** 2
            g[4:] += 2.0 * pen * p[4:]
            return val, g
        return f

    def _gradient(self, data: PnbdData):
        """theta -> d sum w log L / d theta on the device (the covariate entry point when the handle
        has covariates, clv_pnbd_eval otherwise)."""
        evaluate = data.eval if data.k1 is None else data.eval_cov

        def g(theta):
            s = evaluate(self._natural(theta))[0]
            return np.concatenate([s[1:5], s[6:]])
        return g

    def fit(self, frequency, recency, T, weights=None, initial_params=None, tol: float = 1e-7, max_iter: int = 200,
            *, device: int = -1, covariates=None, covariates_dropout=None, covariate_names=None,
            standard_errors: bool = False, robust: bool = False):
        """``covariates`` (N, K1) array or DataFrame for the purchase process, ``covariates_dropout``
        (N, K2) for the dropout process (default: the same matrix; K2 = 0 allowed), at most 8 columns
        each.  ``standard_errors=True`` fills covariance_, standard_errors_ and summary_ from 2 P more
        gradient evaluations (``robust=True``: the sandwich covariance)."""
        cov = covariates is not None
        names, k = list(PARAM_NAMES), None
        if cov:
            n = int(np.asarray(frequency).reshape(-1).shape[0])
            (z1, n1), (z2, n2) = _cov_pair(covariates, covariates_dropout, n, covariate_names)
            names += [f"purchase:{c}" for c in n1] + [f"dropout:{c}" for c in n2]
            k = (len(n1), len(n2))
        elif covariates_dropout is not None:
            raise ValueError("covariates_dropout without covariates: pass covariates with zero columns")
        P = len(names)
        p0 = None
        if initial_params is not None:
            p0 = np.asarray(initial_params, np.float64).reshape(-1 if cov else 4)
            if p0.size == 4:
                p0 = np.concatenate([p0, np.zeros(P - 4)])
            if p0.size != P or not (np.isfinite(p0).all() and (p0[:4] > 0.0).all()):
                raise ValueError("initial_params must be four positive finite numbers" +
                                 (f", or those and the {P - 4} finite covariate coefficients" if cov else ""))
        with PnbdData(frequency, recency, T, weights, device=device, integral=self.integral) as data:
            if cov:
                data.set_covariates(z1, z2)
            if p0 is None or not cov:
                # the plain fit; a covariate fit without initial_params starts from its optimum with
                # gamma = 0, so the nested fit can only gain, and leaves the warnings to its own stage
                with warnings.catch_warnings() if cov else contextlib.nullcontext():
                    if cov:
                        warnings.simplefilter("ignore", RuntimeWarning)
                    self.fit_objective(self._objective(data), np.ones(4) if p0 is None else p0, tol, max_iter)
            if cov:
                n_plain = 0
                if p0 is None:
                    p0, n_plain = np.concatenate([self.params_.to_numpy(), np.zeros(P - 4)]), self.n_eval_
                self.fit_objective(self._objective(data, True), p0, tol, max_iter, names=names)
                self.n_eval_ += n_plain
            sums, nu = data._evaluate(self.params_.to_numpy(), cov)
            self._k, self._shared_dropout = k, covariates_dropout is None
            if standard_errors:
                self._uncertainty(data, robust)
        self.log_likelihood_ = float(sums[0])
        self.n_unconverged_ = nu
        self._device = int(device)
        return self

    def _data(self, frequency, recency, T, weights, covariates, covariates_dropout) -> PnbdData:
        """The handle for a call after the fit; a covariate fit requires its covariates (ValueError
        before any device call), a plain fit refuses them."""
        if self._k is None:
            if covariates is not None or covariates_dropout is not None:
                raise ValueError("the model was fitted without covariates")
            return PnbdData(frequency, recency, T, weights, device=self._device, integral=self.integral)
        if covariates is None:
            raise ValueError("the model was fitted with covariates: pass covariates=")
        if np.shape(covariates)[0] != int(np.asarray(frequency).reshape(-1).shape[0]):
            raise ValueError("covariates must have one row per customer")
        z1, z2 = self._customer_matrices(covariates, covariates_dropout)
        data = PnbdData(frequency, recency, T, weights, device=self._device, integral=self.integral)
        try:
            data.set_covariates(z1, z2)
        except Exception:
            data.close()
            raise
        return data

    def hessian(self, frequency, recency, T, weights=None, *, covariates=None, covariates_dropout=None, theta=None,
                step: float = HESSIAN_STEP, robust: bool = False) -> np.ndarray:
        """The Hessian of sum w log L in theta = (log r, log alpha0, log s, log beta0, gamma1, gamma2)
        by central differences of the device gradient (2 P evaluations, symmetrised), at the fitted
        theta or at ``theta``.  Also sets covariance_, standard_errors_ and summary_ from it (NaN and
        one warning where -H is not positive definite).  On a model that was not fitted, ``theta`` is
        required and is adopted as its parameters."""
        if self.params_ is None and theta is not None:
            n = int(np.asarray(frequency).reshape(-1).shape[0])
            names = list(PARAM_NAMES)
            if covariates is not None:
                (_, n1), (_, n2) = _cov_pair(covariates, covariates_dropout, n)
                names += [f"purchase:{c}" for c in n1] + [f"dropout:{c}" for c in n2]
                self._k, self._shared_dropout = (len(n1), len(n2)), covariates_dropout is None
            t = np.asarray(theta, np.float64).reshape(-1)
            if t.size != len(names) or not np.isfinite(t).all():
                raise ValueError(f"theta must hold {len(names)} finite numbers")
            self.params_ = pd.Series(self._natural(t), index=names)
        theta = self._theta() if theta is None else np.asarray(theta, np.float64).reshape(-1)
        if theta.size != len(self._fitted()) or not np.isfinite(theta).all():
            raise ValueError(f"theta must hold {len(self._fitted())} finite numbers")
        with self._data(frequency, recency, T, weights, covariates, covariates_dropout) as data:
            self._uncertainty(data, robust, theta, step)
        return self.hessian_.copy()

    def scores(self, frequency, recency, T, weights=None, *, covariates=None, covariates_dropout=None) -> np.ndarray:
        """[N][P]: w_i d log L_i / d theta at the fitted parameters: the rows of the sandwich covariance."""
        with self._data(frequency, recency, T, weights, covariates, covariates_dropout) as data:
            return data.scores(self._fitted())

    def fit_objective(self, value_and_grad: Callable, initial_params, tol: float = 1e-7, max_iter: int = 200,
                      *, names=None):
        """The optimiser half of fit() for any ``value_and_grad(theta)``, theta = the logs of the first
        four parameters and the covariate coefficients as they are: sets params_, converged_, n_iter_,
        n_eval_, grad_norm_ and warns when tol was not met.  fit() calls it with the device objective;
        the CPU tests call it with the numpy model."""
        return self._fit_objective(value_and_grad, initial_params, tol, max_iter, names)

    def _customers(self, t, frequency, recency, T, covariates=None, covariates_dropout=None) -> np.ndarray:
        p = self._fitted()
        with self._data(frequency, recency, T, None, covariates, covariates_dropout) as data:
            return data.customers(p, t) if self._k is None else data.customers_cov(p, t)

    def conditional_expected_number_of_purchases_up_to_time(self, t, frequency, recency, T, *, covariates=None,
                                                            covariates_dropout=None) -> np.ndarray:
        """E[Y(t) | x, t_x, T] per customer (t a scalar); a covariate fit requires ``covariates``."""
        return self._customers(float(t), frequency, recency, T, covariates, covariates_dropout)[:, 2].copy()

    def conditional_probability_alive(self, frequency, recency, T, *, covariates=None,
                                      covariates_dropout=None) -> np.ndarray:
        return self._customers(0.0, frequency, recency, T, covariates, covariates_dropout)[:, 1].copy()

    def pointwise_log_likelihood(self, frequency, recency, T, *, covariates=None, covariates_dropout=None) -> np.ndarray:
        """log L per customer at the fitted parameters (column 0 of ``clv_pnbd_customers``): marginal
        over the gamma heterogeneity of lambda and mu."""
        return self._customers(0.0, frequency, recency, T, covariates, covariates_dropout)[:, 0].copy()

    def _dert(self, frequency, recency, T, discount_rate, periods_per_year, horizon, covariates,
              covariates_dropout) -> np.ndarray:
        from .analysis import ltv_params
        p = self._fitted()
        lp = ltv_params(discount_rate, periods_per_year, horizon)
        if np.isinf(lp["horizon"]) and lp["delta"] == 0.0:
            raise ValueError("an infinite horizon needs discount_rate > 0")
        with self._data(frequency, recency, T, None, covariates, covariates_dropout) as data:
            return data.dert(p, lp["delta"], lp["horizon"])

    def discounted_expected_transactions(self, frequency, recency, T, *, discount_rate=0.15, periods_per_year=52.0,
                                         horizon=None, covariates=None, covariates_dropout=None) -> np.ndarray:
        """DERT per customer (Fader, Hardie & Lee 2005): P(alive) (r + x) / (alpha + T) int_0^H exp(-delta t)
        ((beta + T) / (beta + T + t))^s dt, delta = log1p(discount_rate) / periods_per_year as
        ``analysis.ltv_params`` forms it for ``lifetime_value``; ``horizon`` in periods, None = infinite
        (which needs discount_rate > 0)."""
        return self._dert(frequency, recency, T, discount_rate, periods_per_year, horizon, covariates,
                          covariates_dropout)[:, 1].copy()

    def information_criteria(self, frequency, recency, T, *, covariates=None, covariates_dropout=None) -> dict:
        """The fitted model as an entry of ``analysis.compare_models`` beside the HB models'
        ``analysis.marginal_information_criteria`` (:func:`mle_information_criteria` of
        :meth:`pointwise_log_likelihood`).  The entry is IN-SAMPLE: elpd is the log-likelihood of the
        customers the four parameters were fitted to, with the AIC-style penalty p = 4 spread evenly
        (4 / N per customer) — no customer is left out, so it flatters the MLE by what four
        parameters can overfit N customers, and pareto_k is NaN.  A covariate fit is penalised by its
        4 + K1 + K2 parameters and reports them as ``n_params``."""
        ll = self.pointwise_log_likelihood(frequency, recency, T, covariates=covariates,
                                           covariates_dropout=covariates_dropout)
        out = mle_information_criteria(ll, n_params=len(self._fitted()))
        if self._k is not None:
            out["n_params"] = len(self._fitted())
        return out

    def expected_number_of_purchases_up_to_time(self, t, covariates=None, covariates_dropout=None):
        """E[X(t)] = r beta / alpha phi(s - 1, log((beta + t) / beta)), elementwise (host numpy).  With
        covariates (N rows): E[X(t) | z_i] at alpha_i, beta_i, one row per customer, shape (N,) + t.shape."""
        p = self._fitted()
        r, a, s, b = p[:4]
        t = np.asarray(t, np.float64)
        if self._k is None:
            if covariates is not None or covariates_dropout is not None:
                raise ValueError("the model was fitted without covariates")
            return r * b / a * phi(s - 1.0, np.log1p(t / b))
        if covariates is None:
            raise ValueError("the model was fitted with covariates: pass covariates=")
        ai, bi = self._customer_scales(covariates, covariates_dropout)
        shape = (-1,) + (1,) * t.ndim
        ai, bi = ai.reshape(shape), bi.reshape(shape)
        return r * bi / ai * phi(s - 1.0, np.log1p(t[None] / bi))

    def _customer_matrices(self, covariates, covariates_dropout):
        n = int(np.shape(covariates)[0])
        if covariates_dropout is None and not self._shared_dropout:
            if self._k[1] > 0:
                raise ValueError("the model was fitted with covariates_dropout: pass covariates_dropout=")
            covariates_dropout = np.empty((n, 0))
        (z1, _), (z2, _) = _cov_pair(covariates, covariates_dropout, n)
        if (z1.shape[0], z2.shape[0]) != self._k:
            raise ValueError(f"the model was fitted with {self._k[0]} purchase and {self._k[1]} dropout covariates; "
                             f"got {z1.shape[0]} and {z2.shape[0]}")
        return z1, z2

    def _customer_scales(self, covariates, covariates_dropout):
        """(alpha_i, beta_i) per customer at the fitted coefficients (host numpy)."""
        z1, z2 = self._customer_matrices(covariates, covariates_dropout)
        p = self._fitted()
        k1 = self._k[0]
        return p[1] * np.exp(-(p[4:4 + k1] @ z1)), p[3] * np.exp(-(p[4 + k1:] @ z2))


# ---------------------------------------------------------------------------------------------
# Gamma-Gamma spend model
# ---------------------------------------------------------------------------------------------
GG_PARAM_NAMES = ("p", "q", "gamma")


def _gg_columns(frequency, monetary_value, allow_zero: bool = False):
    """(n int32, m float64) validated on the host: integer n >= 1 and finite m > 0 (n = 0 rows pass
    with ``allow_zero``, whatever their m)."""
    f = np.asarray(frequency, np.float64).reshape(-1)
    m = np.asarray(monetary_value, np.float64).reshape(-1)
    if f.shape != m.shape:
        raise ValueError("frequency and monetary_value must have the same length")
    if f.size and not (np.isfinite(f).all() and np.all(f == np.round(f)) and f.max() <= 2 ** 31 - 1):
        raise ValueError("frequency must hold integer transaction counts")
    zero = f == 0
    if (f < 0).any() or (zero.any() and not allow_zero):
        raise ValueError("frequency must be >= 1: filter the customers without a transaction")
    bad = ~zero & ~((m > 0.0) & np.isfinite(m))
    if bad.any():
        raise ValueError("monetary_value must be > 0 and finite: filter the other customers")
    return np.ascontiguousarray(f, dtype=np.int32), np.ascontiguousarray(m)


class GgData(_Handle):
    """Frequency, mean spend and weights resident on the device for a Gamma-Gamma fit (clv_gg_create)."""
    _DESTROY = "clv_gg_destroy"

    def __init__(self, frequency, monetary_value, weights=None, *, device: int = -1):
        self.nn, self.m = _gg_columns(frequency, monetary_value)
        self.n = int(self.nn.shape[0])
        self.w = None
        if weights is not None:
            self.w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
            if self.w.shape[0] != self.n:
                raise ValueError("weights must have the length of frequency")
        L = _lib.lib()
        if _lib.device_count() < 1:
            raise _lib.ClvError("no HIP device visible; the Gamma-Gamma likelihood has no CPU fallback")
        self._L = L
        self._h = ctypes.c_void_p()
        check(L.clv_gg_create(int(device), self.n, self.nn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(self.m),
                              dptr(self.w), ctypes.byref(self._h)))

    def eval(self, params) -> np.ndarray:
        """sums[5]: sum w log L, its derivatives with respect to log(p, q, gamma), sum w."""
        p = np.ascontiguousarray(np.asarray(params, np.float64).reshape(3))
        sums = np.empty(5)
        check(self._L.clv_gg_eval(self._h, dptr(p), dptr(sums)))
        return sums

    def customers(self, params) -> np.ndarray:
        """[n][4]: log L and its gradient with respect to log(p, q, gamma)."""
        p = np.ascontiguousarray(np.asarray(params, np.float64).reshape(3))
        out = np.empty((self.n, 4))
        check(self._L.clv_gg_customers(self._h, dptr(p), dptr(out)))
        return out

    def scores(self, params) -> np.ndarray:
        s = self.customers(params)[:, 1:4]
        return s if self.w is None else s * self.w[:, None]


def device_digamma(x, *, device: int = -1) -> np.ndarray:
    """psi(x) for positive x as the Gamma-Gamma kernel computes it (clv_digamma)."""
    a = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1))
    L = _lib.lib()
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible")
    out = np.empty(a.shape[0])
    check(L.clv_digamma(int(device), a.shape[0], dptr(a), dptr(out)))
    return out.reshape(np.shape(x))


def device_dert_integral(s, B, delta, horizon, *, device: int = -1) -> np.ndarray:
    """J = int_0^H exp(-delta t) (B / (B + t))^s dt per row, as the DERT kernel integrates it
    (clv_dert_integral); horizon may be inf where delta > 0."""
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in np.broadcast_arrays(
        *(np.asarray(v, np.float64).reshape(-1) for v in (s, B, delta, horizon)))]
    L = _lib.lib()
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible")
    out = np.empty(a[0].shape[0])
    check(L.clv_dert_integral(int(device), a[0].shape[0], dptr(a[0]), dptr(a[1]), dptr(a[2]), dptr(a[3]), dptr(out)))
    return out


class GammaGammaFitter(_WaldMixin):
    """The Gamma-Gamma model of spend per transaction by maximum likelihood (Fader, Hardie & Lee 2005;
    Fader & Hardie 2013): mean spend m_i over n_i transactions, params_ = (p, q, gamma).
    ``penalizer_coef`` adds penalizer_coef * sum(params^2) to the per-customer mean negative
    log-likelihood.  The likelihood and its gradient are HIP kernels (csrc/gg.hip)."""
    _N_LOG = 3
    _NAMES = GG_PARAM_NAMES

    def __init__(self, penalizer_coef: float = 0.0):
        self.penalizer_coef = float(penalizer_coef)
        self.params_: Optional[pd.Series] = None
        self._device = -1

    def _objective(self, data: GgData):
        pen = self.penalizer_coef

        def f(theta):
            with np.errstate(over="ignore"):
                p = np.exp(theta)
            if not (np.isfinite(p).all() and (p > 0.0).all()):
                return np.nan, np.full(3, np.nan)
            sums = data.eval(p)
            return -sums[0] / sums[4] + pen * float((p ** 2).sum()), -sums[1:4] / sums[4] + 2.0 * pen * p ** 2
        return f

    def fit(self, frequency, monetary_value, weights=None, initial_params=None, tol: float = 1e-7, max_iter: int = 200,
            *, device: int = -1, standard_errors: bool = False, robust: bool = False):
        p0 = np.ones(3) if initial_params is None else np.asarray(initial_params, np.float64).reshape(3)
        if not (np.isfinite(p0).all() and (p0 > 0.0).all()):
            raise ValueError("initial_params must be three positive finite numbers")
        with GgData(frequency, monetary_value, weights, device=device) as data:
            self.fit_objective(self._objective(data), p0, tol, max_iter)
            sums = data.eval(self.params_.to_numpy())
            if standard_errors:
                self._uncertainty(data, robust)
        self.log_likelihood_ = float(sums[0])
        self._device = int(device)
        return self

    def fit_objective(self, value_and_grad: Callable, initial_params, tol: float = 1e-7, max_iter: int = 200):
        """The optimiser half of fit() for any ``value_and_grad(log params)``, as
        :meth:`ParetoNBDFitter.fit_objective`."""
        return self._fit_objective(value_and_grad, initial_params, tol, max_iter)

    @staticmethod
    def _gradient(data: GgData):
        return lambda theta: data.eval(np.exp(theta))[1:4]

    def hessian(self, frequency, monetary_value, weights=None, *, theta=None, step: float = HESSIAN_STEP,
                robust: bool = False) -> np.ndarray:
        """The Hessian of sum w log L in theta = log(p, q, gamma) by central differences of the device
        gradient; sets covariance_, standard_errors_ and summary_ as :meth:`ParetoNBDFitter.hessian`."""
        if self.params_ is None and theta is not None:
            self.params_ = pd.Series(np.exp(np.asarray(theta, np.float64).reshape(3)), index=list(GG_PARAM_NAMES))
        theta = self._theta() if theta is None else np.asarray(theta, np.float64).reshape(3)
        if not np.isfinite(theta).all():
            raise ValueError("theta must hold three finite numbers")
        with GgData(frequency, monetary_value, weights, device=self._device) as data:
            self._uncertainty(data, robust, theta, step)
        return self.hessian_.copy()

    def pointwise_log_likelihood(self, frequency, monetary_value) -> np.ndarray:
        with GgData(frequency, monetary_value, device=self._device) as data:
            return data.customers(self._fitted())[:, 0].copy()

    def conditional_expected_average_profit(self, frequency=None, monetary_value=None) -> np.ndarray:
        """E[M | n, m] = p (gamma + n m) / (p n + q - 1) per customer; a customer with n = 0 gets the
        population mean p gamma / (q - 1), which is also what no argument returns.  NaN where the
        denominator is not positive (q <= 1 at n = 0).  Host numpy: one division per customer."""
        p, q, g = self._fitted()
        if frequency is None:
            frequency, monetary_value = [0], [0.0]
        nn, m = _gg_columns(frequency, monetary_value, allow_zero=True)
        n = nn.astype(np.float64)
        nm = np.where(nn == 0, 0.0, n * np.where(nn == 0, 0.0, m))
        den = p * n + q - 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0.0, p * (g + nm) / den, np.nan)


def classical_lifetime_value(pnbd: ParetoNBDFitter, gg: GammaGammaFitter, cbs: pd.DataFrame, *, monetary_frequency,
                             monetary_value, discount_rate=0.15, periods_per_year=52.0, horizon=None, covariates=None,
                             covariates_dropout=None) -> pd.DataFrame:
    """The classical CLV of Fader, Hardie & Lee (2005) per customer of ``cbs`` (columns x, t_x, T_cal):
    p_alive and dert from the fitted Pareto/NBD (:meth:`ParetoNBDFitter.discounted_expected_transactions`),
    expected_spend from the fitted Gamma-Gamma at (monetary_frequency, monetary_value) — arrays or
    column names of ``cbs`` — and clv = dert * expected_spend.  The frame stands beside
    ``lifetime_value(draws)["customers"]``; the discount keywords are ``lifetime_value``'s."""
    for c in ("x", "t_x", "T_cal"):
        if c not in cbs.columns:
            raise ValueError(f"cbs missing required column {c!r}")
    mf = cbs[monetary_frequency] if isinstance(monetary_frequency, str) else monetary_frequency
    mv = cbs[monetary_value] if isinstance(monetary_value, str) else monetary_value
    spend = gg.conditional_expected_average_profit(mf, mv)
    if spend.shape[0] != len(cbs):
        raise ValueError("monetary_frequency and monetary_value must have one entry per customer of cbs")
    d = pnbd._dert(cbs["x"].to_numpy(), cbs["t_x"].to_numpy(np.float64), cbs["T_cal"].to_numpy(np.float64), discount_rate,
                   periods_per_year, horizon, covariates, covariates_dropout)
    return pd.DataFrame(dict(p_alive=d[:, 0], dert=d[:, 1], expected_spend=spend, clv=d[:, 1] * spend), index=cbs.index)


def mle_information_criteria(loglik, n_params: int = 4) -> dict:
    """An ``analysis.ic_frames``-shaped dict with ``"kind": "marginal"`` from the in-sample pointwise
    log-likelihood of a maximum-likelihood fit: per customer lppd = log L_i, p_waic = p_loo =
    n_params / N, elpd_waic = elpd_loo = log L_i - n_params / N, pareto_k and tail_len NaN; the totals
    as ic_frames forms them (elpd = log L - n_params), n_samples = 1."""
    from . import _lib
    from .analysis import ic_frames
    ll = np.asarray(loglik, np.float64).reshape(-1)
    n = ll.shape[0]
    if n < 1:
        raise ValueError("no customer")
    stats = np.full((n, len(_lib.IC_STATS)), np.nan)
    pen = float(n_params) / n
    for k, name in enumerate(_lib.IC_STATS):
        if name == "lppd":
            stats[:, k] = ll
        elif name in ("p_waic", "p_loo"):
            stats[:, k] = pen
        elif name in ("elpd_waic", "elpd_loo"):
            stats[:, k] = ll - pen
    out = ic_frames(stats, 2)             # the count only sets the k threshold, and every k is NaN
    for key in ("waic", "loo"):
        out[key]["n_samples"] = 1
        out[key]["warning"] = False    # no importance sampling, no pointwise variance: nothing to warn of
    out["kind"] = "marginal"
    return out


def pnbd_weekly_tracking(fitter: ParetoNBDFitter, birth_week, times, *, device: int = -1, covariates=None,
                         covariates_dropout=None) -> np.ndarray:
    """cum[j] = sum_i E[X(max(times[j] - birth_week[i], 0))]: the "Pareto/NBD (MLE)" curve of the
    reference's Figure 2 (bivariate/analysis_abe.py:434-438), summed on the device.  A covariate fit
    takes the customers' ``covariates`` and sums E[X(t) | z_i] (clv_pnbd_track_cov)."""
    cov = fitter._k is not None
    if not cov and (covariates is not None or covariates_dropout is not None):
        raise ValueError("the model was fitted without covariates")
    if cov and covariates is None:
        raise ValueError("the model was fitted with covariates: pass covariates=")
    b = np.ascontiguousarray(np.asarray(birth_week, np.float64).reshape(-1))
    t = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
    p = np.ascontiguousarray(fitter._fitted())
    zs = ()
    if cov:
        if np.shape(covariates)[0] != b.shape[0]:
            raise ValueError("covariates must have one row per birth_week entry")
        z1, z2 = fitter._customer_matrices(covariates, covariates_dropout)
        zs = (z1.shape[0], dptr(z1) if z1.size else None, z2.shape[0], dptr(z2) if z2.size else None)
    else:
        p = p.reshape(4)
    L = _lib.lib()
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible; the tracking kernel has no CPU fallback")
    out = np.empty(t.shape[0])
    track = L.clv_pnbd_track_cov if cov else L.clv_pnbd_track
    check(track(int(device), b.shape[0], dptr(b), dptr(t), t.shape[0], dptr(p), *zs, dptr(out)))
    return out


def mape_aggregate(actual, pred) -> float:
    """Abe (2009)'s time-series MAPE (utils/analysis_bi_helpers.py:29): the mean absolute deviation
    of the cumulative curves over the final cumulative actual, in percent."""
    a = np.cumsum(np.asarray(actual, np.float64))
    p = np.cumsum(np.asarray(pred, np.float64))
    return float(np.mean(np.abs(p - a)) / a[-1] * 100.0)


# ---------------------------------------------------------------------------------------------
# The log-normal Pareto/NBD by maximum marginal likelihood
# ---------------------------------------------------------------------------------------------
def log_cholesky_sigma(c) -> np.ndarray:
    """(Sigma_00, Sigma_01, Sigma_11) of c = (c0, c1, c2): Sigma = C C', C = [[e^c0, 0], [c1, e^c2]]."""
    c = np.asarray(c, np.float64)
    e0, e2 = np.exp(c[0]), np.exp(c[2])
    return np.array([e0 * e0, e0 * c[1], c[1] * c[1] + e2 * e2])


def sigma_log_cholesky(sigma) -> np.ndarray:
    """(c0, c1, c2) of a positive definite (Sigma_00, Sigma_01, Sigma_11) (ValueError otherwise)."""
    s00, s01, s11 = (float(v) for v in np.asarray(sigma, np.float64).reshape(3))
    if not (np.isfinite([s00, s01, s11]).all() and s00 > 0.0 and s00 * s11 - s01 * s01 > 0.0):
        raise ValueError("Sigma must be finite and positive definite")
    e0 = np.sqrt(s00)
    c1 = s01 / e0
    return np.array([np.log(e0), c1, 0.5 * np.log(s11 - c1 * c1)])


def mml_record(theta, K: int) -> np.ndarray:
    """The level-2 record (beta [2][K], then Sigma_00, Sigma_01, Sigma_11) of theta = (beta, c0, c1, c2)."""
    theta = np.asarray(theta, np.float64).reshape(2 * K + 3)
    return np.ascontiguousarray(np.concatenate([theta[:2 * K], log_cholesky_sigma(theta[2 * K:])]))


def mml_score(theta, K: int, sda, sdb, S, W) -> np.ndarray:
    """[2K + 3, ...]: the score of theta from moments by Fisher's identity and the chain rule.  ``sda``,
    ``sdb`` [K, ...] are (sums of w) d_k E[da] and d_k E[db], ``S`` [3, ...] of E[da da], E[da db], E[db db],
    ``W`` [...] the weight: the sums of clv_mml_eval, or per customer the rows of clv_mml_customers.
    d / d m = P E[(da, db)] and G = d / d Sigma = P (S - W Sigma) P / 2 with P = Sigma^-1; through
    Sigma = C C', d / d C = 2 G C, and the diagonal of C is e^c0, e^c2."""
    theta = np.asarray(theta, np.float64).reshape(2 * K + 3)
    c = theta[2 * K:]
    s00, s01, s11 = log_cholesky_sigma(c)
    det = s00 * s11 - s01 * s01
    P00, P01, P11 = s11 / det, -s01 / det, s00 / det
    sda, sdb, S, W = (np.asarray(v, np.float64) for v in (sda, sdb, S, W))
    R00, R01, R11 = S[0] - W * s00, S[1] - W * s01, S[2] - W * s11
    A00, A01 = P00 * R00 + P01 * R01, P00 * R01 + P01 * R11       # P R
    A10, A11 = P01 * R00 + P11 * R01, P01 * R01 + P11 * R11
    G00 = 0.5 * (A00 * P00 + A01 * P01)
    G01 = 0.5 * (A00 * P01 + A01 * P11)
    G11 = 0.5 * (A10 * P01 + A11 * P11)
    a, b = np.exp(c[0]), np.exp(c[2])
    out = np.empty((2 * K + 3,) + W.shape)
    out[:K] = P00 * sda + P01 * sdb
    out[K:2 * K] = P01 * sda + P11 * sdb
    out[2 * K] = 2.0 * (G00 * a + G01 * c[1]) * a
    out[2 * K + 1] = 2.0 * (G01 * a + G11 * c[1])
    out[2 * K + 2] = 2.0 * G11 * b * b
    return out


def mml_params(theta, K: int):
    """(params [2K + 4], J [2K + 4][2K + 3]): beta, Sigma_00, Sigma_01, Sigma_11 and the correlation
    rho = Sigma_01 / sqrt(Sigma_00 Sigma_11) of theta, and their Jacobian (the delta method's)."""
    theta = np.asarray(theta, np.float64).reshape(2 * K + 3)
    c0, c1, c2 = theta[2 * K:]
    e0, e2 = np.exp(c0), np.exp(c2)
    s00, s01, s11 = log_cholesky_sigma(theta[2 * K:])
    J = np.zeros((2 * K + 4, 2 * K + 3))
    J[:2 * K, :2 * K] = np.eye(2 * K)
    J[2 * K, 2 * K] = 2.0 * s00
    J[2 * K + 1, 2 * K:2 * K + 2] = [s01, e0]
    J[2 * K + 2, 2 * K + 1:] = [2.0 * c1, 2.0 * e2 * e2]
    J[2 * K + 3, 2 * K + 1:] = [e2 * e2 / s11 ** 1.5, -c1 * e2 * e2 / s11 ** 1.5]
    return np.concatenate([theta[:2 * K], [s00, s01, s11, c1 / np.sqrt(s11)]]), J


class MmlData(_Handle):
    """x, t_x, T, weights and the covariate rows resident on the device for the evaluations of a
    maximum-marginal-likelihood fit (clv_mml_create).  ``covariates``: (N, K - 1) or None."""
    _DESTROY = "clv_mml_destroy"

    def __init__(self, frequency, recency, T, weights=None, covariates=None, *, device: int = -1, check_finite=True):
        f = np.asarray(frequency)
        ff = np.asarray(f, np.float64)
        if f.size and not np.all(ff == np.round(ff)):
            raise ValueError("frequency must hold integer repeat counts")
        if f.size and (ff.max() > 2 ** 31 - 1 or ff.min() < -2 ** 31):
            raise ValueError("frequency exceeds int32")
        self.x = np.ascontiguousarray(f, dtype=np.int32).reshape(-1)
        self.t_x = np.ascontiguousarray(np.asarray(recency, np.float64).reshape(-1))
        self.T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1))
        self.n = int(self.x.shape[0])
        if self.t_x.shape[0] != self.n or self.T.shape[0] != self.n:
            raise ValueError("frequency, recency and T must have the same length")
        self.w = None
        if weights is not None:
            self.w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
            if self.w.shape[0] != self.n:
                raise ValueError("weights must have the length of frequency")
        self.cov = None
        if covariates is not None:
            if check_finite:
                self.cov = covariate_matrix(covariates, self.n)[0]
            else:
                self.cov = np.ascontiguousarray(np.asarray(covariates, np.float64).reshape(self.n, -1).T)
            if self.cov.shape[0] == 0:
                self.cov = None
        self.K = 1 if self.cov is None else 1 + int(self.cov.shape[0])
        L = _lib.lib()
        if _lib.device_count() < 1:
            raise _lib.ClvError("no HIP device visible; the marginal likelihood has no CPU fallback")
        self._L = L
        self._h = ctypes.c_void_p()
        check(L.clv_mml_create(int(device), self.n, self.x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                               dptr(self.t_x), dptr(self.T), dptr(self.w), self.K, dptr(self.cov), ctypes.byref(self._h)))

    def design(self) -> np.ndarray:
        """d [K][n]: the intercept row, then the covariate rows."""
        one = np.ones((1, self.n))
        return one if self.cov is None else np.concatenate([one, self.cov])

    def eval(self, record, nodes: int = 0, grid: Optional[int] = None):
        """(sums [2K + 6], n_nonfinite) of clv_mml_eval (``grid`` given: clv_debug_mml_eval)."""
        r = np.ascontiguousarray(np.asarray(record, np.float64).reshape(2 * self.K + 3))
        sums = np.empty(2 * self.K + 6)
        nn = ctypes.c_int64(0)
        if grid is None:
            check(self._L.clv_mml_eval(self._h, dptr(r), int(nodes), dptr(sums), ctypes.byref(nn)))
        else:
            check(self._L.clv_debug_mml_eval(self._h, dptr(r), int(nodes), int(grid), dptr(sums), ctypes.byref(nn)))
        return sums, int(nn.value)

    def customers(self, record, nodes: int = 0, t_star: float = 0.0) -> np.ndarray:
        """[n][8] of clv_mml_customers: the columns _lib.MML_ROW."""
        r = np.ascontiguousarray(np.asarray(record, np.float64).reshape(2 * self.K + 3))
        out = np.empty((self.n, len(_lib.MML_ROW)))
        check(self._L.clv_mml_customers(self._h, dptr(r), int(nodes), float(t_star), dptr(out)))
        return out

    def value_and_score(self, theta, nodes: int = 0):
        """(sum w l, its score in theta, n_nonfinite) at theta = (beta, c0, c1, c2)."""
        K = self.K
        sums, nn = self.eval(mml_record(theta, K), nodes)
        return sums[0], mml_score(theta, K, sums[6:6 + K], sums[6 + K:6 + 2 * K], sums[3:6], sums[1]), nn

    def scores(self, theta, nodes: int = 0) -> np.ndarray:
        """[n][2K + 3]: w_i d l_i / d theta from the rows of :meth:`customers`."""
        rows = self.customers(mml_record(theta, self.K), nodes)
        d = self.design()
        s = mml_score(theta, self.K, d * rows[:, 2], d * rows[:, 3], rows[:, 4:7].T, np.ones(self.n)).T
        return s if self.w is None else s * self.w[:, None]


class LogNormalParetoNBDFitter(_WaldMixin):
    """The Pareto/NBD with Abe (2009)'s log-normal heterogeneity, (log lambda_i, log mu_i) ~ N2(B' d_i, Sigma),
    fitted the classical way: (B, Sigma) maximise the marginal likelihood, the customers' own
    (lambda_i, mu_i) integrated out by the adaptive Gauss-Hermite rule of ``marginal_log_likelihood``
    (csrc/mml.hip).  The score comes from the posterior moments by Fisher's identity, at the
    quadrature's fixed nodes, and the estimate is the root of that score (:func:`minimize_bfgs_score`);
    ``log_likelihood_`` is the quadrature value there.  DESIGN.md §4n.

    theta = (beta in ``level_2`` order, c0, c1, c2) with Sigma = C C', C = [[e^c0, 0], [c1, e^c2]].
    ``params_`` holds beta (``purchase:intercept``, ``purchase:<covariate>`` ..., ``dropout:...``),
    Sigma_00, Sigma_01, Sigma_11 and rho; ``theta_`` the optimiser's parameters, on which ``covariance_``
    and ``hessian_`` stand; ``params_covariance_``, ``standard_errors_`` and ``summary_`` are the delta
    method's on ``params_``."""
    _N_LOG = 0
    SIGMA_NAMES = ("Sigma_00", "Sigma_01", "Sigma_11", "rho")

    def __init__(self):
        self.params_: Optional[pd.Series] = None
        self.theta_ = None
        self._device = -1
        self._K = 1
        self._nodes = 0
        self._names = []

    @staticmethod
    def _beta_names(names):
        cols = ["intercept"] + list(names)
        return [f"purchase:{c}" for c in cols] + [f"dropout:{c}" for c in cols]

    def _theta_names(self):
        return self._beta_names(self._names) + ["c0", "c1", "c2"]

    def _theta(self):
        return np.array(self.theta_, np.float64)

    def _require(self):
        if self.theta_ is None:
            raise RuntimeError("fit() has not been called")

    @staticmethod
    def default_start(K: int, frequency, recency, T) -> np.ndarray:
        """theta of the default start: the sampler's initial intercepts (log of mean x over the mean
        of t_x, T where t_x = 0; log of the mean of 1 / (t_x + 1 / (2 lambda))), no covariate effect, Sigma = I."""
        x, t_x, T = (np.asarray(v, np.float64).reshape(-1) for v in (frequency, recency, T))
        lam = x.mean() / np.mean(np.where(t_x == 0, T, t_x))
        theta = np.zeros(2 * K + 3)
        theta[0] = np.log(lam)
        theta[K] = np.log(np.mean(1.0 / (t_x + 0.5 / lam)))
        return theta

    def _adopt(self, theta):
        self.theta_ = np.array(theta, np.float64)
        p, _ = mml_params(self.theta_, self._K)
        self.params_ = pd.Series(p, index=self._beta_names(self._names) + list(self.SIGMA_NAMES))

    def fit(self, frequency, recency, T, weights=None, covariates=None, initial_params=None, tol: float = 1e-7,
            max_iter: int = 200, *, device: int = -1, covariate_names=None, standard_errors: bool = False,
            robust: bool = False, nodes: int = 32):
        """``covariates`` (N, K - 1) array or DataFrame (at most 8 columns); ``initial_params`` a level-2
        record (beta [2][K], Sigma_00, Sigma_01, Sigma_11).  ``tol`` bounds max |d sum w l / d theta|.
        ``standard_errors=True`` adds 2 P score evaluations (``robust=True``: the sandwich)."""
        from .analysis import marginal_nodes
        q = marginal_nodes(nodes)
        n = int(np.asarray(frequency).reshape(-1).shape[0])
        names = []
        if covariates is not None:
            names = covariate_matrix(covariates, n, "covariates", covariate_names)[1]
        K = 1 + len(names)
        if initial_params is None:
            theta0 = self.default_start(K, frequency, recency, T)
        else:
            r0 = np.asarray(initial_params, np.float64).reshape(-1)
            if r0.size != 2 * K + 3 or not np.isfinite(r0).all():
                raise ValueError(f"initial_params must be a level-2 record of {2 * K + 3} finite numbers")
            theta0 = np.concatenate([r0[:2 * K], sigma_log_cholesky(r0[2 * K:])])
        with MmlData(frequency, recency, T, weights, covariates if K > 1 else None, device=device) as data:
            def objective(theta):
                with np.errstate(over="ignore", invalid="ignore"):
                    v, g, nn = data.value_and_score(theta, q)
                if nn:
                    return np.nan, np.full(theta.size, np.nan)
                return -v, -g
            res = minimize_bfgs_score(objective, theta0, tol, max_iter)
            self._K, self._names, self._nodes, self._device = K, list(names), q, int(device)
            self._adopt(res.x)
            self.converged_ = bool(res.converged)
            self.n_iter_, self.n_eval_ = int(res.n_iter), int(res.n_eval)
            self.grad_norm_ = float(res.grad_norm)
            self.message_ = res.message
            if not res.converged:
                warnings.warn(f"{type(self).__name__} did not converge: {res.message} "
                              f"(max |score| = {res.grad_norm:.3g} after {res.n_eval} evaluations)", RuntimeWarning,
                              stacklevel=2)
            sums, nn = data.eval(mml_record(self.theta_, K), q)
            if standard_errors:
                self._uncertainty(data, robust)
        self.log_likelihood_ = float(sums[0])
        self.n_nonfinite_ = nn
        return self

    def _uncertainty(self, data, robust: bool, theta=None, step: float = HESSIAN_STEP):
        theta = self._theta() if theta is None else theta
        H = central_hessian(lambda t: data.value_and_score(t, self._nodes)[1], theta, step)
        return self._set_uncertainty(H, data.scores(theta, self._nodes) if robust else None, theta)

    def _set_uncertainty(self, H, scores=None, theta=None):
        theta = self._theta() if theta is None else np.asarray(theta, np.float64)
        keep, self.params_ = self.params_, pd.Series(theta, index=self._theta_names())
        try:
            super()._set_uncertainty(H, scores, theta)     # hessian_, covariance_ and the summary on theta
        finally:
            self.params_ = keep
        self.theta_summary_ = self.summary_
        p, J = mml_params(theta, self._K)
        pc = J @ self.covariance_.to_numpy() @ J.T
        names = list(self.params_.index)
        self.params_covariance_ = pd.DataFrame(pc, index=names, columns=names)
        self.standard_errors_ = pd.Series(delta_standard_errors(p, pc, 0), index=names)
        self.summary_ = wald_summary(p, pc, names, 0)
        return self

    def _data(self, frequency, recency, T, weights, covariates) -> MmlData:
        self._require()
        if self._K == 1 and covariates is not None:
            raise ValueError("the model was fitted without covariates")
        if self._K > 1:
            if covariates is None:
                raise ValueError("the model was fitted with covariates: pass covariates=")
            if np.ndim(covariates) == 2 and np.shape(covariates)[1] != self._K - 1:
                raise ValueError(f"the model was fitted with {self._K - 1} covariates")
        return MmlData(frequency, recency, T, weights, covariates, device=self._device)

    def _rows(self, t, frequency, recency, T, covariates) -> np.ndarray:
        with self._data(frequency, recency, T, None, covariates) as data:
            return data.customers(mml_record(self.theta_, self._K), self._nodes, float(t))

    def hessian(self, frequency, recency, T, weights=None, *, covariates=None, step: float = HESSIAN_STEP,
                robust: bool = False) -> np.ndarray:
        """The Jacobian of the score in theta by central differences (2 P evaluations, symmetrised) at
        the fitted theta; sets covariance_, standard_errors_ and summary_ from it."""
        with self._data(frequency, recency, T, weights, covariates) as data:
            self._uncertainty(data, robust, None, step)
        return self.hessian_.copy()

    def scores(self, frequency, recency, T, weights=None, *, covariates=None) -> np.ndarray:
        """[N][2K + 3]: w_i d l_i / d theta at the fitted theta: the rows of the sandwich covariance."""
        with self._data(frequency, recency, T, weights, covariates) as data:
            return data.scores(self.theta_, self._nodes)

    def pointwise_log_likelihood(self, frequency, recency, T, *, covariates=None) -> np.ndarray:
        """l_i per customer at the fitted (beta, Sigma): the bits of ``marginal_log_likelihood`` of
        :meth:`as_level2_record`."""
        return self._rows(0.0, frequency, recency, T, covariates)[:, 0].copy()

    def conditional_probability_alive(self, frequency, recency, T, *, covariates=None) -> np.ndarray:
        """The empirical-Bayes P(alive at T | x, t_x, T, theta-hat)."""
        return self._rows(0.0, frequency, recency, T, covariates)[:, 1].copy()

    def conditional_expected_number_of_purchases_up_to_time(self, t, frequency, recency, T, *,
                                                            covariates=None) -> np.ndarray:
        """E[X*(t) | x, t_x, T, theta-hat]: the expected purchases in (T, T + t] (t a scalar)."""
        return self._rows(float(t), frequency, recency, T, covariates)[:, 7].copy()

    def posterior_means(self, frequency, recency, T, *, covariates=None) -> pd.DataFrame:
        """Per customer the empirical-Bayes posterior mean and sd of log lambda_i and log mu_i, their
        correlation and P(alive)."""
        with self._data(frequency, recency, T, None, covariates) as data:
            rows = data.customers(mml_record(self.theta_, self._K), self._nodes, 0.0)
            d = data.design()
        K = self._K
        m0, m1 = self.theta_[:K] @ d, self.theta_[K:2 * K] @ d
        va = np.maximum(rows[:, 4] - rows[:, 2] ** 2, 0.0)
        vb = np.maximum(rows[:, 6] - rows[:, 3] ** 2, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            corr = (rows[:, 5] - rows[:, 2] * rows[:, 3]) / np.sqrt(va * vb)
        return pd.DataFrame(dict(log_lambda_mean=m0 + rows[:, 2], log_lambda_sd=np.sqrt(va), log_mu_mean=m1 + rows[:, 3],
                                 log_mu_sd=np.sqrt(vb), corr=corr, p_alive=rows[:, 1]))

    def information_criteria(self, frequency, recency, T, *, covariates=None) -> dict:
        """The fitted model as an entry of ``analysis.compare_models`` beside ``marginal_information_criteria``
        and ``ParetoNBDFitter.information_criteria``: in-sample, penalised by its 2K + 3 parameters
        (:func:`mle_information_criteria`), ``"kind": "marginal"``."""
        ll = self.pointwise_log_likelihood(frequency, recency, T, covariates=covariates)
        out = mle_information_criteria(ll, n_params=2 * self._K + 3)
        out["n_params"] = 2 * self._K + 3
        return out

    def as_level2_record(self) -> np.ndarray:
        """theta-hat in the ``level_2`` layout, [1 chain][1 draw][2K + 3]: what ``marginal_log_likelihood``,
        ``marginal_log_score`` and ``score_customers`` take as ``draws``."""
        self._require()
        return mml_record(self.theta_, self._K).reshape(1, 1, -1)

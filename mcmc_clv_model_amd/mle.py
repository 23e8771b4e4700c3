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
"""
from __future__ import annotations

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


# ---------------------------------------------------------------------------------------------
# Device handle
# ---------------------------------------------------------------------------------------------
def _params_array(params) -> np.ndarray:
    p = np.ascontiguousarray(np.asarray(params, np.float64).reshape(4))
    return p


class PnbdData:
    """The CBS columns resident on the device for the evaluations of a fit (clv_pnbd_create)."""

    def __init__(self, frequency, recency, T, weights=None, *, device: int = -1):
        L = _lib.lib()
        if _lib.device_count() < 1:
            raise _lib.ClvError("no HIP device visible; the Pareto/NBD likelihood has no CPU fallback")
        f = np.asarray(frequency)
        if f.size and not np.all(np.asarray(f, np.float64) == np.round(np.asarray(f, np.float64))):
            raise ValueError("frequency must hold integer repeat counts")
        if f.size and (np.asarray(f, np.float64).max() > 2 ** 31 - 1 or np.asarray(f, np.float64).min() < -2 ** 31):
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

    def eval(self, params):
        """(sums[6], n_unconverged): sum w log L, its derivatives with respect to
        log(r, alpha, s, beta), sum w; customers whose series hit the term cap (sums[0] is NaN then)."""
        p = _params_array(params)
        sums = np.empty(6)
        nu = ctypes.c_int64(0)
        check(self._L.clv_pnbd_eval(self._h, dptr(p), dptr(sums), ctypes.byref(nu)))
        return sums, int(nu.value)

    def customers(self, params, t_star: float = 0.0) -> np.ndarray:
        """[n][3]: log L, P(alive), E[Y(t_star) | x, t_x, T]."""
        p = _params_array(params)
        out = np.empty((self.n, 3))
        check(self._L.clv_pnbd_customers(self._h, dptr(p), float(t_star), dptr(out)))
        return out

    def close(self):
        if self._h:
            self._L.clv_pnbd_destroy(self._h)
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


def phi(k: float, ell):
    """-expm1(-k ell) / k, and ell at k = 0."""
    ell = np.asarray(ell, np.float64)
    return ell.copy() if k == 0.0 else -np.expm1(-k * ell) / k


# ---------------------------------------------------------------------------------------------
# Fitter
# ---------------------------------------------------------------------------------------------
class ParetoNBDFitter:
    """Pareto/NBD by maximum likelihood (Schmittlein, Morrison & Colombo 1987; the likelihood as in
    Fader & Hardie 2005).  ``penalizer_coef`` adds penalizer_coef * sum(params^2) to the
    per-customer mean negative log-likelihood."""

    def __init__(self, penalizer_coef: float = 0.0):
        self.penalizer_coef = float(penalizer_coef)
        self.params_: Optional[pd.Series] = None
        self._device = -1

    def _objective(self, data: PnbdData):
        pen = self.penalizer_coef

        def f(theta):
            with np.errstate(over="ignore"):
                p = np.exp(theta)
            if not (np.isfinite(p).all() and (p > 0.0).all()):
                return np.nan, np.full(4, np.nan)
            sums, _ = data.eval(p)
            val = -sums[0] / sums[5] + pen * float((p ** 2).sum())
            return val, -sums[1:5] / sums[5] + 2.0 * pen * p ** 2
        return f

    def fit(self, frequency, recency, T, weights=None, initial_params=None, tol: float = 1e-7, max_iter: int = 200,
            *, device: int = -1):
        p0 = np.ones(4) if initial_params is None else np.asarray(initial_params, np.float64).reshape(4)
        if not (np.isfinite(p0).all() and (p0 > 0.0).all()):
            raise ValueError("initial_params must be four positive finite numbers")
        with PnbdData(frequency, recency, T, weights, device=device) as data:
            self.fit_objective(self._objective(data), p0, tol, max_iter)
            sums, nu = data.eval(self.params_.to_numpy())
        self.log_likelihood_ = float(sums[0])
        self.n_unconverged_ = nu
        self._device = int(device)
        return self

    def fit_objective(self, value_and_grad: Callable, initial_params, tol: float = 1e-7, max_iter: int = 200):
        """The optimiser half of fit() for any ``value_and_grad(log params)``: sets params_,
        converged_, n_iter_, n_eval_, grad_norm_ and warns when tol was not met.  fit() calls it
        with the device objective; the CPU tests call it with the numpy model."""
        res = minimize_bfgs(value_and_grad, np.log(np.asarray(initial_params, np.float64).reshape(4)), tol, max_iter)
        self.params_ = pd.Series(np.exp(res.x), index=list(PARAM_NAMES))
        self.converged_ = bool(res.converged)
        self.n_iter_, self.n_eval_ = int(res.n_iter), int(res.n_eval)
        self.grad_norm_ = float(res.grad_norm)
        self.message_ = res.message
        if not res.converged:
            warnings.warn(f"ParetoNBDFitter did not converge: {res.message} "
                          f"(max |gradient| = {res.grad_norm:.3g} after {res.n_eval} evaluations)", RuntimeWarning,
                          stacklevel=3)
        return self

    def _fitted(self) -> np.ndarray:
        if self.params_ is None:
            raise RuntimeError("fit() has not been called")
        return self.params_.to_numpy(dtype=np.float64)

    def _customers(self, t, frequency, recency, T) -> np.ndarray:
        with PnbdData(frequency, recency, T, device=self._device) as data:
            return data.customers(self._fitted(), t)

    def conditional_expected_number_of_purchases_up_to_time(self, t, frequency, recency, T) -> np.ndarray:
        """E[Y(t) | x, t_x, T] per customer (t a scalar)."""
        return self._customers(float(t), frequency, recency, T)[:, 2].copy()

    def conditional_probability_alive(self, frequency, recency, T) -> np.ndarray:
        return self._customers(0.0, frequency, recency, T)[:, 1].copy()

    def pointwise_log_likelihood(self, frequency, recency, T) -> np.ndarray:
        """log L per customer at the fitted parameters (column 0 of ``clv_pnbd_customers``): marginal
        over the gamma heterogeneity of lambda and mu."""
        return self._customers(0.0, frequency, recency, T)[:, 0].copy()

    def information_criteria(self, frequency, recency, T) -> dict:
        """The fitted model as an entry of ``analysis.compare_models`` beside the HB models'
        ``analysis.marginal_information_criteria`` (:func:`mle_information_criteria` of
        :meth:`pointwise_log_likelihood`).  The entry is IN-SAMPLE: elpd is the log-likelihood of the
        customers the four parameters were fitted to, with the AIC-style penalty p = 4 spread evenly
        (4 / N per customer) — no customer is left out, so it flatters the MLE by what four
        parameters can overfit N customers, and pareto_k is NaN."""
        return mle_information_criteria(self.pointwise_log_likelihood(frequency, recency, T))

    def expected_number_of_purchases_up_to_time(self, t):
        """E[X(t)] = r beta / alpha phi(s - 1, log((beta + t) / beta)), elementwise (host numpy)."""
        r, a, s, b = self._fitted()
        return r * b / a * phi(s - 1.0, np.log1p(np.asarray(t, np.float64) / b))


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


def pnbd_weekly_tracking(fitter: ParetoNBDFitter, birth_week, times, *, device: int = -1) -> np.ndarray:
    """cum[j] = sum_i E[X(max(times[j] - birth_week[i], 0))]: the "Pareto/NBD (MLE)" curve of the
    reference's Figure 2 (bivariate/analysis_abe.py:434-438), summed on the device."""
    L = _lib.lib()
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible; the tracking kernel has no CPU fallback")
    b = np.ascontiguousarray(np.asarray(birth_week, np.float64).reshape(-1))
    t = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
    p = _params_array(fitter._fitted())
    out = np.empty(t.shape[0])
    check(L.clv_pnbd_track(int(device), b.shape[0], dptr(b), dptr(t), t.shape[0], dptr(p), dptr(out)))
    return out


def mape_aggregate(actual, pred) -> float:
    """Abe (2009)'s time-series MAPE (utils/analysis_bi_helpers.py:29): the mean absolute deviation
    of the cumulative curves over the final cumulative actual, in percent."""
    a = np.cumsum(np.asarray(actual, np.float64))
    p = np.cumsum(np.asarray(pred, np.float64))
    return float(np.mean(np.abs(p - a)) / a[-1] * 100.0)

"""Posterior analysis on the GPU, drop-in for the reference's helpers.

Reference functions mirrored (same names, arguments, defaults and return layout):

* ``draw_future_transactions`` — ``src/models/bivariate/mcmc.py:506-546`` (counts) and, as
  ``draw_future_transactions_rfm_m`` / ``trivariate.draw_future_transactions``,
  ``src/models/trivariate/mcmc.py:660-749`` (counts and lognormal spend totals).
* ``post_mean_lambdas``, ``post_mean_mus``, ``chain_total_loglik``, ``compute_table4`` —
  ``src/models/utils/analysis_bi_helpers.py:15-27, 52-72, 75-166``.
* ``posterior_weekly_tracking`` — the posterior-predictive weekly repeat-transaction curve of
  ``src/models/bivariate/analysis_abe.py:444-464`` (inline script code in the reference).

* ``summarize_level2``, ``extract_correlation`` — ``analysis_bi_helpers.py:6-13, 39-48`` (host only).
* ``level2_diagnostics``, ``level2_autocorr`` — what ``bivariate/analysis_abe.py:651-706`` asks of
  ArviZ (``az.summary``, ``az.plot_autocorr``) on the level-2 draws, and ``level1_diagnostics``, the
  same convergence check for every customer's parameters (``csrc/diag.hip``: split R-hat and mean
  ESS without rank normalisation, see :func:`level1_diagnostics`).
* ``level2_summary`` — the nine columns of ``az.summary`` (``analysis_abe.py:690-693``) with the
  rank-normalised ``ess_bulk``, ``ess_tail`` and ``r_hat``; ``level1_rank_diagnostics`` /
  ``level2_rank_diagnostics`` give every rank-normalised statistic (``clv_rank_diagnostics``).
* ``lifetime_value``, ``customer_equity``, ``lifetime_value_elasticities`` — what Abe (2015) derives
  from the level-1 draws and the reference leaves out: every customer's posterior lifetime value,
  the value of the customer base and the elasticity of CLV to the covariates (``csrc/ltv.hip``).
* ``pointwise_log_likelihood``, ``information_criteria``, ``psis_loo``, ``compare_models`` — what
  ``az.waic`` / ``az.loo`` / ``az.compare`` would give on the draws the reference wraps in
  ``az.from_dict`` and never compares: WAIC and PSIS-LOO per customer (``csrc/ic.hip``).
* ``score_customers`` — level-1 draws for customers outside the fit, from its level-2 draws
  (``csrc/score.hip``): bi:193-227, 268-339 and tri:306-333 run against stored (beta, Sigma) records.
* ``forecast``, ``forecast_pit``, ``compare_forecasts``, ``forecast_table`` — the holdout forecast the
  reference builds its draws for, in closed form (``csrc/forecast.hip``): every customer's predictive
  distribution of the holdout count, its out-of-sample scores, Table 2's disaggregate rows and
  Figure 3's conditional expectations from the posterior mean instead of a plug-in.
* ``posterior_predictive_check``, ``ppc_pit`` — the ``posterior_predictive`` group the reference's
  ``az.from_dict`` objects never get: the calibration data replicated per draw at the customer or at
  the population level (``csrc/ppc.hip``), the actual-vs-replicated frequency histogram, posterior
  predictive p-values and per-customer calibration PITs.
* ``marginal_log_likelihood``, ``marginal_information_criteria``, ``marginal_log_score`` — ``az.loo`` on a
  likelihood that is marginal over the customer's own (lambda, mu) (``csrc/marginal.hip``): one 2-D
  adaptive Gauss-Hermite quadrature per (customer, level-2 record), the statistics of ``csrc/ic.hip``.

The per-customer / per-draw work runs in ``csrc/analysis.hip`` through the C ABI (``clv_predict``,
``clv_track``, ``clv_level1_summary``, ``clv_chain_total_loglik``); the host only reshapes and
formats (pandas).  Random draws come from Philox streams keyed by ``seed`` (the reference uses
one numpy Generator), so simulated outputs match the reference in distribution; the statistics
(means, percentiles) are exact.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import numpy as np
import pandas as pd

from . import _lib
from ._lib import check, dptr
from .sampler import resolve_seed

__all__ = ["draw_future_transactions", "draw_future_transactions_rfm_m", "post_mean_lambdas", "post_mean_mus",
           "chain_total_loglik", "compute_table4", "level1_summary", "posterior_weekly_tracking",
           "level1_diagnostics", "level2_diagnostics", "level2_autocorr", "summarize_level2", "extract_correlation",
           "summary_rhat", "level1_rank_diagnostics", "level2_rank_diagnostics", "level2_summary",
           "lifetime_value", "customer_equity", "lifetime_value_elasticities",
           "pointwise_log_likelihood", "information_criteria", "psis_loo", "compare_models", "score_customers",
           "forecast", "forecast_pit", "compare_forecasts", "forecast_table", "posterior_predictive_check", "ppc_pit",
           "marginal_log_likelihood", "marginal_information_criteria", "marginal_log_score"]


def _stacked_level1(level1_chains) -> np.ndarray:
    if level1_chains is None:
        raise ValueError("level-1 draws are needed (run the sampler with draw_sink='full')")
    a = np.ascontiguousarray(np.concatenate(list(level1_chains), axis=0), dtype=np.float64)
    if a.ndim != 3 or a.shape[2] not in (4, 5):
        raise ValueError("level_1 draws must be (n_draws, n_customers, 4 or 5) per chain")
    return a


def _L():
    L = _lib.lib()
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible; the analysis kernels have no CPU fallback")
    return L


def _i64p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _predict(cbs, draws, T_star, seed, simulate_spend, sigma_s, device):
    L = _L()
    a = _stacked_level1(draws["level_1"])
    nd, n, w = a.shape
    T_cal = np.ascontiguousarray(cbs["T_cal"].to_numpy(float))
    if T_cal.shape[0] != n:
        raise ValueError("cbs and draws disagree on the number of customers")
    x = np.empty((nd, n), np.int64)
    spend = np.empty((nd, n), np.float64) if simulate_spend else None
    check(L.clv_predict(int(device), dptr(a), nd, n, w, dptr(T_cal), float(T_star), resolve_seed(seed),
                        1 if simulate_spend else 0, float(sigma_s), _i64p(x), dptr(spend) if spend is not None else None))
    return x, spend


def draw_future_transactions(cbs: pd.DataFrame, draws: Dict[str, Any], T_star: float = 39.0,
                             seed: Optional[int] = None, *, device: int = -1) -> np.ndarray:
    """Posterior-predictive transactions in (T_cal, T_cal + T_star] (bivariate/mcmc.py:506-546):
    x* ~ Poisson(lambda * tau*), tau* = T_star if alive else clip(tau - T_cal, 0, T_star).
    Returns int64 (n_draws_total, n_customers), chains stacked in order."""
    return _predict(cbs, draws, T_star, seed, False, 0.5, device)[0]


def draw_future_transactions_rfm_m(cbs: pd.DataFrame, draws: Dict[str, Any], T_star: float = 39.0, *,
                                   simulate_spend: bool = True, sigma_s: float = 0.50, seed: Optional[int] = None,
                                   device: int = -1):
    """RFM-M posterior predictive (trivariate/mcmc.py:660-749): counts as above and, with
    ``simulate_spend``, per-customer totals of x* lognormal(mean=eta, sigma=sigma_s) spends (eta is
    the level-1 column 4, passed as the log-mean like the reference). Returns ``x_future`` or
    ``(x_future, spend_future)``."""
    x, spend = _predict(cbs, draws, T_star, seed, simulate_spend, sigma_s, device)
    return (x, spend) if simulate_spend else x


def level1_summary(draws: Dict[str, Any], mu_cap: float = 0.05, *, device: int = -1) -> pd.DataFrame:
    """Per-customer posterior statistics computed on the GPU: means of lambda, mu, min(mu, mu_cap),
    z, tau (and eta), and numpy-'linear' 2.5 / 97.5 percentiles of lambda and mu.  A result of
    ``draw_sink="summary+pct"`` (no level-1 draws) carries them already, formed on the device at
    the end of the run (``draws["summary"]["level1"]``; mu_cap 0.05 only)."""
    if draws.get("level_1") is None and isinstance(draws.get("summary"), dict) and "level1" in draws["summary"]:
        if mu_cap != _lib.SUMMARY_MU_CAP:
            raise ValueError("a summary run's capped mean of mu uses mu_cap = 0.05")
        return draws["summary"]["level1"]
    L = _L()
    a = _stacked_level1(draws["level_1"])
    nd, n, w = a.shape
    out = np.empty((n, len(_lib.L1_STATS)), np.float64)
    check(L.clv_level1_summary(int(device), dptr(a), nd, n, w, float(mu_cap), dptr(out)))
    cols = list(_lib.L1_STATS if w == 5 else _lib.L1_STATS[:-1])
    return pd.DataFrame(out[:, :len(cols)], columns=cols)


def post_mean_lambdas(draws) -> np.ndarray:
    """analysis_bi_helpers.py:15-20 — per-customer posterior mean of lambda over all chains' draws."""
    return level1_summary(draws)["mean_lambda"].to_numpy()


def post_mean_mus(draws) -> np.ndarray:
    """analysis_bi_helpers.py:22-27 — per-customer posterior mean of mu over all chains' draws."""
    return level1_summary(draws)["mean_mu"].to_numpy()


def chain_total_loglik(level1_chains, cbs, *, device: int = -1) -> float:
    """analysis_bi_helpers.py:52-72 — mean over draws of the total log-likelihood
    sum_i [x log(lam) + (1-z) log(mu) - (lam+mu)(z T + (1-z) tau) - gammaln(x+1)]."""
    L = _L()
    a = _stacked_level1(level1_chains)
    nd, n, w = a.shape
    x = np.ascontiguousarray(cbs["x"].to_numpy(), dtype=np.int32)
    T_cal = np.ascontiguousarray(cbs["T_cal"].to_numpy(float))
    out = ctypes.c_double()
    check(L.clv_chain_total_loglik(int(device), dptr(a), nd, n, w, x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   dptr(T_cal), ctypes.byref(out)))
    return float(out.value)


def compute_table4(draws, xstar_draws=None) -> pd.DataFrame:
    """analysis_bi_helpers.py:75-166 — Table 4 of Abe (2009): customer-level statistics (per-customer
    reductions on the GPU), ranked by expected validation-period transactions, top/bottom 10 plus
    Ave/Min/Max rows, rounded like the paper.  ``xstar_draws`` is accepted and unused, as in the
    reference."""
    s = level1_summary(draws, mu_cap=0.05)
    mean_lambda = s["mean_lambda"].to_numpy()
    mean_mu = s["mean_mu_capped"].to_numpy()
    mean_z = s["mean_z"].to_numpy()
    t_star = 39
    mean_xstar = mean_z * (mean_lambda / mean_mu) * (1.0 - np.exp(-mean_mu * t_star))
    with np.errstate(divide="ignore"):
        mean_lifetime = np.where(mean_mu > 0, (1.0 / mean_mu) / 52.0, np.inf)
    surv_1yr = np.exp(-mean_mu * 52)
    df = pd.DataFrame({
        "Mean(λ)": mean_lambda,
        "2.5% tile λ": s["lambda_p025"].to_numpy(),
        "97.5% tile λ": s["lambda_p975"].to_numpy(),
        "Mean(μ)": mean_mu,
        "2.5% tile μ": s["mu_p025"].to_numpy(),
        "97.5% tile μ": s["mu_p975"].to_numpy(),
        "Mean exp lifetime (yrs)": mean_lifetime,
        "Survival rate (1yr)": surv_1yr,
        "P(alive at T_cal)": mean_z,
        "Exp # of trans in val period": mean_xstar,
    })
    df.index.name = "Customer ID"
    df_sorted = df.sort_values("Exp # of trans in val period", ascending=False).reset_index(drop=True)
    df_sorted.insert(0, "ID", df_sorted.index + 1)
    top10, bottom10 = df_sorted.iloc[:10], df_sorted.iloc[-10:]
    ave_row = df.mean().to_frame().T.assign(ID="Ave")
    min_row = df.min().to_frame().T.assign(ID="Min")
    max_row = df.max().to_frame().T.assign(ID="Max")
    out = pd.concat([top10, pd.DataFrame({"ID": ["…"]}), bottom10, ave_row, min_row, max_row],
                    ignore_index=True).set_index("ID")
    lam_cols = ["Mean(λ)", "2.5% tile λ", "97.5% tile λ"]
    mu_cols = ["Mean(μ)", "2.5% tile μ", "97.5% tile μ"]
    out[lam_cols] = out[lam_cols].round(3)
    out[mu_cols] = out[mu_cols].round(4)
    out["Mean exp lifetime (yrs)"] = out["Mean exp lifetime (yrs)"].round(2)
    out["Survival rate (1yr)"] = out["Survival rate (1yr)"].round(3)
    out["P(alive at T_cal)"] = out["P(alive at T_cal)"].round(3)
    out["Exp # of trans in val period"] = out["Exp # of trans in val period"].round(2)
    return out


def posterior_weekly_tracking(draws, birth_week, times, seed: Optional[int] = 0, *, device: int = -1) -> np.ndarray:
    """Posterior-predictive weekly repeat transactions (bivariate/analysis_abe.py:444-464): for every
    week t in ``times`` (ascending), the mean over all draws of the simulated transactions of the
    customers with birth_week < t <= birth_week + tau (rate lambda per unit time).  The reference
    draws one Poisson per customer and week; their sum is drawn here as one exact Poisson of the
    summed rate (same distribution).  Returns inc_hb_weekly (float64, len(times)); np.cumsum gives
    the tracking curve."""
    L = _L()
    a = _stacked_level1(draws["level_1"])
    nd, n, w = a.shape
    b = np.ascontiguousarray(np.asarray(birth_week, dtype=np.float64))
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float64))
    if b.shape[0] != n:
        raise ValueError("birth_week must have one entry per customer")
    out = np.empty(t.shape[0], np.float64)
    check(L.clv_track(int(device), dptr(a), nd, n, w, dptr(b), dptr(t), t.shape[0], resolve_seed(seed), dptr(out)))
    return out


# ---- customer lifetime value and customer equity (csrc/ltv.hip) --------------------------------
def ltv_params(discount_rate=0.15, periods_per_year=52.0, horizon=None, omega2=0.0) -> dict:
    """The scalars clv_lifetime_value takes, validated (ValueError) on the host: delta =
    log1p(discount_rate) / periods_per_year, horizon (None = infinite), value_scale = exp(omega2 / 2)."""
    r, ppy, w2 = float(discount_rate), float(periods_per_year), float(omega2)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError(f"discount_rate must be finite and >= 0 (got {discount_rate!r})")
    if not (np.isfinite(ppy) and ppy > 0.0):
        raise ValueError(f"periods_per_year must be finite and > 0 (got {periods_per_year!r})")
    if not np.isfinite(w2):
        raise ValueError(f"omega2 must be finite (got {omega2!r})")
    h = np.inf if horizon is None else float(horizon)
    if np.isnan(h) or h <= 0.0:
        raise ValueError(f"horizon must be > 0 or None for an infinite one (got {horizon!r})")
    with np.errstate(over="ignore"):
        scale = float(np.exp(w2 / 2.0))
    if not np.isfinite(scale):
        raise ValueError(f"exp(omega2 / 2) overflows (omega2 = {omega2!r})")
    return dict(delta=float(np.log1p(r) / ppy), horizon=h, value_scale=scale, periods_per_year=ppy)


def ltv_monetary(monetary, n: int, width: int) -> Optional[np.ndarray]:
    """The per-customer value per transaction of a width-4 (bivariate) run as a float64 [n] array."""
    if monetary is None:
        return None
    if width == 5:
        raise ValueError("monetary is for the bivariate model's draws: the trivariate model's value per "
                         "transaction is its eta column (scaled through omega2)")
    m = np.ascontiguousarray(np.asarray(monetary, dtype=np.float64))
    if m.shape != (n,):
        raise ValueError(f"monetary must have one entry per customer ({n}); got shape {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("monetary must be finite")
    return m


def ltv_frames(cust: np.ndarray, per_draw: np.ndarray, par: dict) -> dict:
    return dict(customers=pd.DataFrame(cust, columns=list(_lib.LTV_STATS)),
                draws=pd.DataFrame(per_draw, columns=list(_lib.LTV_DRAW_STATS)),
                delta=par["delta"], horizon=par["horizon"])


def lifetime_value(draws: Dict[str, Any], *, discount_rate: float = 0.15, periods_per_year: float = 52.0,
                   horizon: Optional[float] = None, monetary=None, omega2: float = 0.0,
                   device: int = -1) -> Dict[str, Any]:
    """Posterior customer lifetime value and customer equity from the level-1 draws, on the GPU
    (``csrc/ltv.hip``, ``clv_lifetime_value``): Abe (2015)'s ``CLV = eta lambda / (mu + delta)`` per
    draw and customer, summarised per customer over the draws and per draw over the customers.

    ``delta = log1p(discount_rate) / periods_per_year`` is the continuous discount rate per time unit
    of the data (15 % a year on weekly data: 0.0027); ``horizon`` (that unit; None = infinite) cuts
    the value at ``H``: ``value = lambda m (1 - exp(-(mu + delta) H)) / (mu + delta)``, the discounted
    expected value of a customer alive at time 0; ``residual = z value`` is what is left after
    ``T_cal``.  ``m``, the value per transaction, is ``eta exp(omega2 / 2)`` for the trivariate model
    (eta is the median of the log-normal spend, ``omega2`` the sampler's var(log_s): 0 keeps eta) and
    ``monetary`` (one entry per customer; default 1: discounted expected transactions, the DERT of
    Fader, Hardie & Lee 2005) for the bivariate one.

    Returns ``{"customers": DataFrame, one row per customer, columns _lib.LTV_STATS (mean, sd,
    2.5 / 50 / 97.5 percentiles of value and of residual, p_alive, lifetime_yrs = E[1 / (ppy mu)],
    survival_1yr = E[exp(-ppy mu)]), "draws": DataFrame, one row per stacked draw, columns
    _lib.LTV_DRAW_STATS (equity = sum of residual, value_total, n_alive, mu_share = mean over
    customers of mu / (mu + delta)), "delta": float, "horizon": float}``.  Unlike plugging posterior
    means into the formula (``compute_table4``) these are posterior means of the non-linear
    quantities, with intervals.  Arguments are checked before any device is touched."""
    par = ltv_params(discount_rate, periods_per_year, horizon, omega2)
    a = _stacked_level1(draws.get("level_1"))
    nd, n, w = a.shape
    m = ltv_monetary(monetary, n, w)
    L = _L()
    cust = np.empty((n, len(_lib.LTV_STATS)), np.float64)
    per_draw = np.empty((nd, len(_lib.LTV_DRAW_STATS)), np.float64)
    check(L.clv_lifetime_value(int(device), dptr(a), nd, n, w, dptr(m), par["delta"], par["horizon"],
                               par["value_scale"], par["periods_per_year"], dptr(cust), dptr(per_draw)))
    return ltv_frames(cust, per_draw, par)


def customer_equity(ltv: Dict[str, Any]) -> pd.DataFrame:
    """The value of the customer base: one row with mean, sd (ddof 1) and the 2.5 / 50 / 97.5
    percentiles over the draws of ``equity`` (the value left in the customers after T_cal) and, as
    ``value_total_*``, of ``value_total`` (the same customers, all alive at time 0).  Host numpy."""
    row = {}
    for col, pre in (("equity", ""), ("value_total", "value_total_")):
        v = ltv["draws"][col].to_numpy()
        p = np.percentile(v, [2.5, 50.0, 97.5])
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = v.std(ddof=1) if v.size > 1 else np.nan
        row.update({pre + "mean": v.mean(), pre + "sd": sd, pre + "p025": p[0], pre + "p50": p[1], pre + "p975": p[2]})
    return pd.DataFrame([row])


ELASTICITY_COMPONENTS = ("purchase_rate", "lifetime", "spend", "total")


def lifetime_value_elasticities(draws: Dict[str, Any], covariates, *, discount_rate: float = 0.15,
                                periods_per_year: float = 52.0, ltv: Optional[Dict[str, Any]] = None,
                                device: int = -1) -> pd.DataFrame:
    """Abe (2015)'s decomposition of the elasticity of CLV to each covariate, per draw s and covariate
    k (the intercept excluded): ``purchase_rate = beta_lambda,k``, ``lifetime = -beta_mu,k
    mu_share_s``, ``spend = beta_eta,k`` (0 for the bivariate model) and their ``total`` — d log CLV /
    d x_k of ``CLV = eta lambda / (mu + delta)`` averaged over the customers, which holds for the
    infinite horizon only.  beta comes from ``draws["level_2"]`` (rows ``[beta[:, 0] (K), beta[:, 1]
    (K), (beta[:, 2] (K)), Sigma's upper triangle]``, K = len(covariates) + 1), ``mu_share`` from
    ``ltv["draws"]`` (:func:`lifetime_value`, computed here on the GPU when ``ltv`` is not given).
    Returns a DataFrame indexed by (covariate, component) with mean, p025 and p975 over the draws."""
    covariates = list(covariates)
    K = len(covariates) + 1
    l2 = np.concatenate([np.asarray(c, dtype=np.float64) for c in draws["level_2"]], axis=0)
    if l2.ndim != 2:
        raise ValueError("level_2 draws must be (n_draws, n_params) per chain")
    D = {2 * K + 3: 2, 3 * K + 6: 3}.get(l2.shape[1])
    if D is None:
        raise ValueError(f"level_2 rows of width {l2.shape[1]} do not fit {len(covariates)} covariates plus the "
                         f"intercept (expected {2 * K + 3} or {3 * K + 6})")
    if ltv is None:
        ltv = lifetime_value(draws, discount_rate=discount_rate, periods_per_year=periods_per_year, device=device)
    if np.isfinite(ltv.get("horizon", np.inf)):
        raise ValueError("the elasticity decomposition holds for the infinite horizon: ltv was computed with "
                         f"horizon = {ltv['horizon']}")
    share = ltv["draws"]["mu_share"].to_numpy()
    if share.shape[0] != l2.shape[0]:
        raise ValueError(f"ltv has {share.shape[0]} draws, level_2 has {l2.shape[0]}")
    rows, index = [], []
    for k, name in enumerate(covariates, start=1):
        rate = l2[:, k]
        life = -l2[:, K + k] * share
        spend = l2[:, 2 * K + k] if D == 3 else np.zeros_like(rate)
        for comp, v in zip(ELASTICITY_COMPONENTS, (rate, life, spend, rate + life + spend)):
            p = np.percentile(v, [2.5, 97.5])
            rows.append((v.mean(), p[0], p[1]))
            index.append((name, comp))
    idx = pd.MultiIndex.from_arrays([[i[0] for i in index], [i[1] for i in index]], names=["covariate", "component"])
    return pd.DataFrame(rows, columns=["mean", "p025", "p975"], index=idx)


# ---- model comparison: WAIC and PSIS-LOO (csrc/ic.hip) -----------------------------------------
def ic_params(spend=False, omega2=None, reff=1.0, log_s=None) -> dict:
    """spend / omega2 / reff of the information criteria, validated (ValueError) on the host; the
    default omega2 of the spend term is var(log_s, ddof 1), the sampler's own."""
    spend = bool(spend)
    r = float(reff)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"reff must be finite and > 0 (got {reff!r})")
    w2 = 0.0
    if spend:
        if omega2 is None:
            if log_s is None or len(log_s) < 2:
                raise ValueError("spend=True needs omega2 or at least two customers' log_s for its default")
            omega2 = np.var(log_s, ddof=1)
        w2 = float(omega2)
        if not (np.isfinite(w2) and w2 > 0.0):
            raise ValueError(f"omega2 must be finite and > 0 (got {omega2!r})")
    elif omega2 is not None:
        raise ValueError("omega2 belongs to the spend term (spend=True)")
    return dict(spend=spend, omega2=w2, reff=r)


def _ic_shape(nd: int, n: int, w: int, spend: bool, reff: float) -> None:
    if nd < _lib.IC_MIN_DRAWS or nd > _lib.IC_MAX_DRAWS:
        raise ValueError(f"{nd} stacked draws: the information criteria take {_lib.IC_MIN_DRAWS} to "
                         f"{_lib.IC_MAX_DRAWS}")
    if n < 1:
        raise ValueError("no customer")
    if spend and w != 5:
        raise ValueError("spend=True needs the trivariate model's draws (the eta column)")
    if np.ceil(min(nd / 5.0, 3.0 * np.sqrt(nd / reff))) > _lib.IC_MAX_TAIL:
        raise ValueError(f"reff = {reff!r} gives a tail of more than {_lib.IC_MAX_TAIL} draws")


def _ic_data(cbs, n: int, spend: bool):
    """x (int32), t_x, T_cal and (spend) log_s of the CBS as contiguous arrays of n entries."""
    x = np.ascontiguousarray(cbs["x"].to_numpy(), dtype=np.int32)
    t_x = np.ascontiguousarray(cbs["t_x"].to_numpy(float))
    T_cal = np.ascontiguousarray(cbs["T_cal"].to_numpy(float))
    if not (x.shape[0] == t_x.shape[0] == T_cal.shape[0] == n):
        raise ValueError("cbs and draws disagree on the number of customers")
    log_s = None
    if spend:
        if "log_s" not in cbs:
            raise ValueError("spend=True needs a log_s column in cbs")
        log_s = np.ascontiguousarray(cbs["log_s"].to_numpy(float))
    return x, t_x, T_cal, log_s


def fixed_order_sum(v) -> float:
    """Sum of a per-customer column in the project's fixed order (csrc/pnbd.hip): zero-padded
    256-customer blocks by the tree (offsets 128 ... 1), then lane t adds the block partials t,
    t + 256, ... in turn and the lanes go through the same tree."""
    def tree(a):
        off = _lib.BLOCK // 2
        while off:
            a[:, :off] += a[:, off:2 * off]
            off >>= 1
        return a[:, 0]
    v = np.asarray(v, np.float64)
    nb = -(-len(v) // _lib.BLOCK)
    part = tree(np.pad(v, (0, nb * _lib.BLOCK - len(v))).reshape(nb, _lib.BLOCK))
    rows = np.pad(part, (0, -(-nb // _lib.BLOCK) * _lib.BLOCK - nb)).reshape(-1, _lib.BLOCK)
    acc = np.zeros(_lib.BLOCK)
    for row in rows:
        acc = acc + row
    return float(tree(acc[None])[0])


def bad_k_threshold(n_samples: int) -> float:
    """The Pareto k above which PSIS-LOO is not to be trusted: min(1 - 1 / log10(S), 0.7)."""
    return min(1.0 - 1.0 / np.log10(n_samples), 0.7)


def ic_frames(stats: np.ndarray, n_samples: int) -> dict:
    """The per-customer columns [n][len(_lib.IC_STATS)] as {"pointwise", "waic", "loo"}: the totals
    are formed here in float64 with :func:`fixed_order_sum` — elpd the sum of the per-customer
    values, se = sqrt(N var(., ddof 0)) (deviations from the mean, squares, the same sum), p the sum
    of the penalties, n_bad_k the customers with pareto_k above :func:`bad_k_threshold`, warning =
    any such customer (loo) or any p_waic > 0.4 (waic, as az.waic).  A NaN customer (a non-finite
    log-likelihood) makes the totals NaN."""
    pw = pd.DataFrame(stats, columns=list(_lib.IC_STATS))
    n = stats.shape[0]

    def total(col):
        v = pw[col].to_numpy()
        mean = fixed_order_sum(v) / n
        dev = v - mean
        return fixed_order_sum(v), float(np.sqrt(n * (fixed_order_sum(dev * dev) / n)))
    k = pw["pareto_k"].to_numpy()
    n_bad = int(np.count_nonzero(k > bad_k_threshold(n_samples)))
    rows = {}
    for name, ecol, pcol in (("waic", "elpd_waic", "p_waic"), ("loo", "elpd_loo", "p_loo")):
        elpd, se = total(ecol)
        warn = bool(n_bad > 0) if name == "loo" else bool(np.any(pw["p_waic"].to_numpy() > 0.4))
        rows[name] = pd.DataFrame([dict(elpd=elpd, se=se, p=fixed_order_sum(pw[pcol].to_numpy()),
                                        n_samples=int(n_samples), n_data_points=int(n),
                                        n_bad_k=n_bad if name == "loo" else 0, warning=warn)])
    return dict(pointwise=pw, waic=rows["waic"], loo=rows["loo"])


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def pointwise_log_likelihood(draws: Dict[str, Any], cbs: pd.DataFrame, *, spend: bool = False, omega2=None,
                             device: int = -1) -> np.ndarray:
    """The log-likelihood of every customer under every stacked draw, on the GPU (``csrc/ic.hip``,
    ``clv_pointwise_loglik``): float64 (n_draws_total, n_customers), chains stacked in order.  It is
    marginal over z and tau — the Pareto/NBD individual likelihood given the draw's (lambda, mu) —
    unlike the reference's ``log_likelihood`` and ``chain_total_loglik``, which condition on them.
    ``spend=True`` (trivariate draws) adds one observation of ``log_s ~ N(log eta, omega2)``;
    ``omega2`` defaults to ``var(cbs["log_s"], ddof=1)``, the sampler's.  ``spend=False`` on
    trivariate draws gives the transaction part alone, comparable with a bivariate fit."""
    a = _stacked_level1(draws.get("level_1"))
    nd, n, w = a.shape
    x, t_x, T_cal, log_s = _ic_data(cbs, n, spend)
    par = ic_params(spend, omega2, 1.0, log_s)
    _ic_shape(nd, n, w, par["spend"], 1.0)
    L = _L()
    out = np.empty((nd, n), np.float64)
    check(L.clv_pointwise_loglik(int(device), dptr(a), nd, n, w, _i32p(x), dptr(t_x), dptr(T_cal), dptr(log_s),
                                 par["omega2"], dptr(out)))
    return out


def information_criteria(draws: Dict[str, Any], cbs: pd.DataFrame, *, spend: bool = False, omega2=None,
                         reff: float = 1.0, device: int = -1) -> Dict[str, Any]:
    """WAIC and Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman & Gabry 2017) of a
    fit, per customer and in total, on the GPU (``csrc/ic.hip``, ``clv_information_criteria``): what
    ``az.waic`` and ``az.loo`` give on :func:`pointwise_log_likelihood`, without that matrix leaving
    the device.  ``reff`` is the relative efficiency of the draws (ESS / S; the rank diagnostics
    give ESS), which sets the tail length ``M = ceil(min(S / 5, 3 sqrt(S / reff)))``.

    Returns ``{"pointwise": DataFrame, one row per customer, columns _lib.IC_STATS (lppd, p_waic,
    elpd_waic, elpd_loo, p_loo, pareto_k — +inf where the tail had fewer than 5 distinct values or
    the fit failed and the raw weights were kept —, tail_len), "waic", "loo": one-row DataFrames
    elpd, se, p, n_samples, n_data_points, n_bad_k, warning}`` (:func:`ic_frames`); compare fits of
    the same customers with :func:`compare_models`.  Arguments are checked before any device is
    touched."""
    a = _stacked_level1(draws.get("level_1"))
    nd, n, w = a.shape
    x, t_x, T_cal, log_s = _ic_data(cbs, n, spend)
    par = ic_params(spend, omega2, reff, log_s)
    _ic_shape(nd, n, w, par["spend"], par["reff"])
    L = _L()
    out = np.empty((n, len(_lib.IC_STATS)), np.float64)
    check(L.clv_information_criteria(int(device), dptr(a), nd, n, w, _i32p(x), dptr(t_x), dptr(T_cal), dptr(log_s),
                                     par["omega2"], par["reff"], dptr(out)))
    return ic_frames(out, nd)


_SCORE_SINKS = {"full": _lib.SINK_FULL, "summary": _lib.SINK_SUMMARY}


def score_level2(draws) -> np.ndarray:
    """The level-2 records of a fit as one C-contiguous float64 array [chain][draw][width]: ``draws``
    is a drop-in's return value (its ``level_2`` list, one (n_draws, width) array per chain) or such
    a list / array itself."""
    l2 = draws.get("level_2") if isinstance(draws, dict) else draws
    if l2 is None:
        raise ValueError("level-2 records are needed (draws['level_2'])")
    try:
        a = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in l2]))
    except ValueError as e:
        raise ValueError(f"level_2 must be one (n_draws, width) array per chain, all alike: {e}") from None
    if a.ndim != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("level_2 must be one (n_draws, width) array per chain, at least one record each")
    return a


def score_problem(cbs_new: pd.DataFrame, covariates, width: int):
    """(D, K, x int32, t_x, T_cal, cov (K-1, N) or None, log_s or None) of the new customers' CBS for
    records of ``width`` doubles: K = 1 + len(covariates), D from width = D K + D (D + 1) / 2."""
    covariates = list(covariates or [])
    K = 1 + len(covariates)
    if K > _lib.MAX_K:
        raise ValueError(f"at most {_lib.MAX_K - 1} covariates are supported (got {K - 1})")
    D = {2 * K + 3: 2, 3 * K + 6: 3}.get(int(width))
    if D is None:
        raise ValueError(f"level-2 records of {width} doubles match neither the bivariate ({2 * K + 3}) nor the "
                         f"trivariate ({3 * K + 6}) model with {K - 1} covariates")
    for col in ["x", "t_x", "T_cal"] + covariates + (["log_s"] if D == 3 else []):
        if col not in cbs_new:
            raise ValueError(f"cbs_new has no column {col!r}")
    n = len(cbs_new)
    if n < 1:
        raise ValueError("no customer to score")
    xv = cbs_new["x"].to_numpy()
    if np.any(xv < 0) or np.any(xv > np.iinfo(np.int32).max) or np.any(xv != np.round(xv)):
        raise ValueError("x must hold non-negative integer counts")
    x = np.ascontiguousarray(xv, dtype=np.int32)
    t_x = np.ascontiguousarray(cbs_new["t_x"].to_numpy(float))
    T_cal = np.ascontiguousarray(cbs_new["T_cal"].to_numpy(float))
    cov = np.ascontiguousarray(cbs_new[covariates].to_numpy(float).T) if covariates else None
    log_s = np.ascontiguousarray(cbs_new["log_s"].to_numpy(float)) if D == 3 else None
    return D, K, x, t_x, T_cal, cov, log_s


def score_init(level2: np.ndarray, D: int, K: int, cov, n: int, init):
    """The shadow chains' start state [chain][N]: ``init=(lam, mu)`` checked and broadcast, or the
    default lambda_0 = exp(x_i' beta_{c,0}[:, 0]), mu_0 = exp(x_i' beta_{c,0}[:, 1]) from each chain's
    first record — per customer, whoever else is in the batch (the reference's init_state, bi:367-370,
    uses batch means instead)."""
    C = level2.shape[0]
    if init is None:
        X = np.ones((n, K))
        if K > 1:
            X[:, 1:] = cov.T
        beta0 = level2[:, 0, :D * K].reshape(C, D, K)          # beta.T.ravel(): [d][k]
        lam = np.exp(np.einsum("nk,ck->cn", X, beta0[:, 0]))
        mu = np.exp(np.einsum("nk,ck->cn", X, beta0[:, 1]))
    else:
        try:
            lam, mu = (np.broadcast_to(np.asarray(v, dtype=np.float64), (C, n)) for v in init)
        except ValueError:
            raise ValueError(f"init must be (lam, mu), each shaped ({C}, {n})") from None
    lam, mu = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(mu, dtype=np.float64)
    tiny = np.finfo(np.float64).tiny
    if not (np.isfinite(lam).all() and np.isfinite(mu).all() and (lam >= tiny).all() and (mu >= tiny).all()):
        raise ValueError("init must be finite and > 0")
    return lam, mu


def score_options(inner_sweeps, warmup, n_mh_steps, sink, customer_offset, sweep_first, n_draws, n) -> dict:
    """The scoring options validated on the host (ValueError)."""
    if sink not in _SCORE_SINKS:
        raise ValueError(f"sink must be one of {sorted(_SCORE_SINKS)}")
    R, W, S = int(inner_sweeps), int(warmup), int(n_mh_steps)
    off, t0 = int(customer_offset), int(sweep_first)
    if R < 1:
        raise ValueError("inner_sweeps must be >= 1")
    if W < 0 or S < 0:
        raise ValueError("warmup and n_mh_steps must be >= 0")
    if off < 0 or off + n > 1 << 32:
        raise ValueError("customer_offset + N must fit in 32 bits")
    if t0 < 1 or t0 + W + R * n_draws - 1 > (1 << 32) - 1:
        raise ValueError("the inner-sweep numbers sweep_first .. sweep_first + warmup + inner_sweeps * n_draws - 1 "
                         "must lie in 1 .. 2^32 - 1")
    return dict(inner=R, warmup=W, S=S, sink=_SCORE_SINKS[sink], offset=off, sweep_first=t0)


def score_outputs(sink: str, C: int, nd: int, n: int, D: int):
    """(level1 or None, sums or None) host buffers of a scoring call."""
    if sink == "full":
        try:
            return np.empty((C, nd, n, D + 2), np.float64), None
        except MemoryError:
            raise MemoryError(f"the full sink's {C} x {nd} x {n} x {D + 2} level-1 draws do not fit in host memory; "
                              "use sink=\"summary\"") from None
    return None, np.empty((C, _lib.N_SUM_STATS, n), np.float64)


def score_check(rc: int) -> None:
    if rc == -4:  # CLV_ENOMEM: the message names sink="summary"
        raise MemoryError(_lib.lib().clv_last_error().decode(errors="replace"))
    check(rc)


def score_result(sink: str, level2: np.ndarray, l1, sums, lam, mu, D: int, opts: dict) -> Dict[str, Any]:
    """The return value of :func:`score_customers`."""
    C, nd = level2.shape[:2]
    state = dict(lam=lam, mu=mu, next_sweep=opts["sweep_first"] + opts["warmup"] + opts["inner"] * nd)
    if sink == "full":
        return dict(level_1=[l1[c] for c in range(C)], level_2=[level2[c] for c in range(C)], state=state)
    names = [s for s in _lib.SUM_STATS if D == 3 or "eta" not in s]
    tot = sums.sum(axis=0) / float(C * nd)                      # pooled over chains
    keep = ("lambda", "mu", "z", "log_lambda", "log_mu", "tau", "eta", "mu_capped")
    means = pd.DataFrame({f"mean_{k}": tot[_lib.SUM_STATS.index(k)] for k in keep if k in names})
    return dict(level_1=None, level_2=[level2[c] for c in range(C)], state=state,
                summary=dict(sums={k: sums[:, _lib.SUM_STATS.index(k)] for k in names}, n_draws=nd, means=means))


def score_customers(draws, cbs_new: pd.DataFrame, covariates=None, *, inner_sweeps: int = 10, warmup: int = 50,
                    n_mh_steps: int = 20, seed: Optional[int] = 0, omega2=None, sink: str = "full", init=None,
                    customer_offset: int = 0, chain_first: int = 0, sweep_first: int = 1,
                    device: int = -1) -> Dict[str, Any]:
    """Score customers who were not in the fit from its level-2 draws, on the GPU (``csrc/score.hip``,
    ``clv_score_customers``).  Given (beta, Sigma) customers are conditionally independent, so

        p(theta_i | y_i, fit) = integral p(theta_i | y_i, beta, Sigma) p(beta, Sigma | fit) d(beta, Sigma):

    for every chain c of ``draws["level_2"]`` and every row i of ``cbs_new`` (columns x, t_x, T_cal, the
    ``covariates`` and, for a trivariate fit, log_s) one shadow chain runs the level-1 half of the sweep
    (draw_z, draw_tau, ``n_mh_steps`` MH steps, draw_eta: bi:193-227, 268-339; tri:306-333) against that
    chain's records: ``warmup`` inner sweeps against record 0, then ``inner_sweeps`` against each record
    in turn, the state after the last being that record's draw.  The variates are a function of
    (seed, chain_first + c, customer_offset + i, inner-sweep number) alone, so the result does not
    depend on how the customers are batched: shard a customer base with ``customer_offset``.

    (beta, Sigma) is held fixed during a record's inner sweeps (a two-stage, "cut" analysis).  If all
    records of a chain are equal the scheme is exactly invariant for any ``inner_sweeps``; when they
    vary, theta enters record d distributed for record d - 1, a bias that fades as ``inner_sweeps``
    grows and as the level-2 posterior narrows.  Measured with records that
    alternate between two values three level-2 posterior sd apart, the worst customer's posterior
    mean is off by 0.34 of its posterior sd at ``inner_sweeps=1``, 0.14 at 5 and 0.035 at the
    default 10; a fit's own consecutive records are far closer than that.

    ``sink="full"`` returns a dict shaped like the drop-ins': ``level_1`` a list of (n_draws, N, D + 2)
    arrays (lambda, mu, tau, z, [eta]), ``level_2`` the input's, ``state`` the final (lam, mu) and the
    next inner-sweep number — so lifetime_value, draw_future_transactions, information_criteria,
    level1_summary and level1_diagnostics work on it unchanged.  ``sink="summary"`` keeps nothing per
    record: ``summary`` holds the per-chain sums ([chain][N] per statistic), the record count and a
    frame of posterior means pooled over chains (lambda, mu, z, log lambda, log mu, tau, eta, mu capped
    at 0.05) — the way to score millions of customers against thousands of records.  A full sink that
    does not fit in memory raises MemoryError naming ``sink="summary"``.

    ``init=(lam, mu)`` ([chain][N]) overrides the default start exp(x_i' beta_{c,0}); with the
    returned ``state``, ``warmup=0`` and ``sweep_first=state["next_sweep"]`` a call on further records
    continues this one exactly.  ``omega2`` (trivariate) defaults to var(cbs_new["log_s"], ddof=1).
    Arguments are checked before any device is touched."""
    level2 = score_level2(draws)
    C, nd, width = level2.shape
    D, K, x, t_x, T_cal, cov, log_s = score_problem(cbs_new, covariates, width)
    n = x.shape[0]
    opts = score_options(inner_sweeps, warmup, n_mh_steps, sink, customer_offset, sweep_first, nd, n)
    w2 = 1.0
    if D == 3:
        if omega2 is None:
            if n < 2:
                raise ValueError("omega2 is needed: its default is var(cbs_new['log_s'], ddof=1) of at least two customers")
            omega2 = np.var(log_s, ddof=1)
        w2 = float(omega2)
        if not (np.isfinite(w2) and w2 > 0.0):
            raise ValueError(f"omega2 must be finite and > 0 (got {omega2!r})")
    elif omega2 is not None:
        raise ValueError("omega2 belongs to the trivariate model")
    if int(chain_first) < 0:
        raise ValueError("chain_first must be >= 0")
    lam0, mu0 = score_init(level2, D, K, cov, n, init)
    L = _L()
    l1, sums = score_outputs(sink, C, nd, n, D)
    lam, mu = np.empty((C, n)), np.empty((C, n))
    score_check(L.clv_score_customers(int(device), D, K, C, nd, dptr(level2), n, _i32p(x), dptr(t_x), dptr(T_cal),
                                      dptr(cov), dptr(log_s), w2, opts["S"], opts["warmup"], opts["inner"],
                                      resolve_seed(seed), int(chain_first), opts["offset"], opts["sweep_first"],
                                      dptr(lam0), dptr(mu0), opts["sink"], dptr(l1), dptr(sums), dptr(lam), dptr(mu)))
    return score_result(sink, level2, l1, sums, lam, mu, D, opts)


def psis_loo(log_lik, *, reff: float = 1.0, device: int = -1) -> Dict[str, Any]:
    """:func:`information_criteria` of any pointwise log-likelihood matrix (n_draws, n_observations)
    (``clv_psis_loo``)."""
    ll = np.ascontiguousarray(np.asarray(log_lik, dtype=np.float64))
    if ll.ndim != 2:
        raise ValueError("log_lik must be (n_draws, n_observations)")
    par = ic_params(False, None, reff)
    _ic_shape(ll.shape[0], ll.shape[1], 4, False, par["reff"])
    L = _L()
    out = np.empty((ll.shape[1], len(_lib.IC_STATS)), np.float64)
    check(L.clv_psis_loo(int(device), dptr(ll), ll.shape[0], ll.shape[1], par["reff"], dptr(out)))
    return ic_frames(out, ll.shape[0])


def compare_models(models: Dict[str, Dict[str, Any]], criterion: str = "loo") -> pd.DataFrame:
    """Rank fits of the same customers by ``criterion`` ("loo" or "waic"), as ``az.compare`` does:
    one row per model, best first, with rank, elpd, p, ``elpd_diff`` = the best model's elpd minus
    this one's, ``dse = sqrt(N var(elpd_i - elpd_best,i, ddof 0))`` — the standard error of that
    difference from the paired per-customer values — se, n_bad_k and warning.  Host numpy on the
    frames of :func:`information_criteria`; ValueError on unequal customer counts.  Entries of
    :func:`marginal_information_criteria` (and ``ParetoNBDFitter.information_criteria``) carry
    ``"kind": "marginal"``; entries without the key are conditional, and a mix of the two kinds is
    refused with a ValueError that names both: their pointwise terms are different likelihoods."""
    if criterion not in ("loo", "waic"):
        raise ValueError(f"criterion must be 'loo' or 'waic' (got {criterion!r})")
    if not models:
        raise ValueError("no model to compare")
    kinds = {k: m.get("kind", "conditional") for k, m in models.items()}
    if len(set(kinds.values())) > 1:
        groups = {kind: sorted(k for k in kinds if kinds[k] == kind) for kind in sorted(set(kinds.values()))}
        raise ValueError("marginal and conditional criteria are not comparable (the pointwise terms are different "
                         f"likelihoods): {groups}")
    col = "elpd_" + criterion
    point = {k: m["pointwise"][col].to_numpy() for k, m in models.items()}
    sizes = {len(v) for v in point.values()}
    if len(sizes) != 1:
        raise ValueError(f"the models were fitted to different numbers of customers: {sorted(sizes)}")
    n = sizes.pop()
    order = sorted(models, key=lambda k: -float(models[k][criterion]["elpd"].iloc[0]))
    best = order[0]
    rows = []
    for r, k in enumerate(order):
        tot = models[k][criterion].iloc[0]
        diff = point[best] - point[k]
        rows.append(dict(rank=r, elpd=float(tot["elpd"]), p=float(tot["p"]),
                         elpd_diff=float(models[best][criterion]["elpd"].iloc[0]) - float(tot["elpd"]),
                         dse=float(np.sqrt(n * np.var(diff))), se=float(tot["se"]), n_bad_k=int(tot["n_bad_k"]),
                         warning=bool(tot["warning"])))
    return pd.DataFrame(rows, index=pd.Index(order, name="model"))


# ---- the marginal likelihood and marginal WAIC / PSIS-LOO (csrc/marginal.hip) ------------------
def marginal_nodes(nodes) -> int:
    """``nodes`` of the marginal-likelihood functions as the C ABI's argument: None or 0 the default
    order, else one of _lib.MARGINAL_ORDERS (ValueError)."""
    if nodes is None:
        return 0
    q = int(nodes)
    if q != nodes or q not in (0,) + tuple(_lib.MARGINAL_ORDERS):
        raise ValueError(f"nodes must be None or one of {_lib.MARGINAL_ORDERS} (got {nodes!r})")
    return q


def marginal_problem(draws, cbs: pd.DataFrame, covariates, spend: bool, omega2):
    """(level2 [R][width], D, K, x, t_x, T_cal, cov, log_s or None, omega2) of a marginal-likelihood
    call: the chains' records stacked in order, the columns :func:`score_problem` takes (log_s only
    with ``spend=True``), validated on the host (ValueError)."""
    l2 = score_level2(draws)
    level2 = np.ascontiguousarray(l2.reshape(-1, l2.shape[2]))
    spend = bool(spend)
    covariates = list(covariates or [])
    K = 1 + len(covariates)
    D = {2 * K + 3: 2, 3 * K + 6: 3}.get(int(level2.shape[1]))
    if spend and D == 2:
        raise ValueError("spend=True needs the trivariate model's records")
    frame = cbs if (D != 3 or "log_s" in cbs) else cbs.assign(log_s=0.0)   # the column is read with spend only
    D, K, x, t_x, T_cal, cov, log_s = score_problem(frame, covariates, level2.shape[1])
    if spend and "log_s" not in cbs:
        raise ValueError("spend=True needs a log_s column in cbs")
    w2 = 1.0
    if spend:
        if omega2 is None:
            if len(log_s) < 2:
                raise ValueError("spend=True needs omega2 or at least two customers' log_s for its default")
            omega2 = np.var(log_s, ddof=1)
        w2 = float(omega2)
        if not (np.isfinite(w2) and w2 > 0.0):
            raise ValueError(f"omega2 must be finite and > 0 (got {omega2!r})")
    elif omega2 is not None:
        raise ValueError("omega2 belongs to the spend term (spend=True)")
    if level2.shape[0] > _lib.MARGINAL_MAX_RECORDS:
        raise ValueError(f"{level2.shape[0]} level-2 records: the marginal likelihood takes at most "
                         f"{_lib.MARGINAL_MAX_RECORDS}")
    return level2, D, K, x, t_x, T_cal, cov, (log_s if spend else None), w2


def marginal_log_likelihood(draws, cbs: pd.DataFrame, covariates=None, *, spend: bool = False, omega2=None,
                            nodes=None, device: int = -1) -> np.ndarray:
    """The log of the marginal likelihood of every customer under every level-2 record, on the GPU
    (``csrc/marginal.hip``, ``clv_marginal_loglik``): float64 (R, N), R the records of all chains
    stacked in order — the layout of :func:`pointwise_log_likelihood`, so :func:`psis_loo` reads it.

        p(y_i | beta, Sigma) = int int L(x_i, t_x,i, T_i | lambda, mu) N2((log lambda, log mu); beta' d_i, Sigma_12)

    The customer's own (lambda, mu) is integrated out against the record's population distribution,
    so no level-1 draws are needed and ``cbs`` may hold the fit's own customers or new ones (the
    columns :func:`score_customers` takes: x, t_x, T_cal, the ``covariates``).  ``spend=True``
    (trivariate records, a log_s column) multiplies in one observation log_s ~ N(log eta, omega2) with
    eta integrated out analytically; ``omega2`` defaults to ``var(cbs["log_s"], ddof=1)``.
    ``spend=False`` on trivariate records reads the transaction block alone, comparable with a
    bivariate fit.

    ``nodes``: the points per dimension of the adaptive Gauss-Hermite rule, one of 8, 16, 24, 32
    (None: the default, _lib.MARGINAL_DEFAULT_NODES).  DESIGN.md section 4k records the quadrature
    error each order reaches against the exact integral: the default, 32, is the smallest order within
    1e-6 of it on every customer of the fixture under CDNOW-like population distributions (24 reaches
    2.9e-6); under much wider ones (Sigma_11 = 3, Sigma_22 = 6) no supported order reaches 1e-6 on
    every edge customer (32 reaches 1.2e-5).
    A record whose Sigma_12 is not positive definite gives NaN in its row; a non-finite t_x or T_cal
    in that customer's column.  Arguments are checked before any device is touched."""
    level2, D, K, x, t_x, T_cal, cov, log_s, w2 = marginal_problem(draws, cbs, covariates, spend, omega2)
    q = marginal_nodes(nodes)
    L = _L()
    out = np.empty((level2.shape[0], x.shape[0]), np.float64)
    check(L.clv_marginal_loglik(int(device), dptr(level2), D, K, dptr(cov), level2.shape[0], x.shape[0], _i32p(x),
                                dptr(t_x), dptr(T_cal), dptr(log_s), w2, q, dptr(out)))
    return out


def marginal_frames(stats: np.ndarray, n_samples: int) -> dict:
    """:func:`ic_frames` of marginal criteria: the same dict plus ``"kind": "marginal"``."""
    out = ic_frames(stats, n_samples)
    out["kind"] = "marginal"
    return out


def marginal_information_criteria(draws, cbs: pd.DataFrame, covariates=None, *, spend: bool = False, omega2=None,
                                  reff: float = 1.0, nodes=None, device: int = -1) -> Dict[str, Any]:
    """WAIC and PSIS-LOO of a fit from the marginal likelihood (:func:`marginal_log_likelihood`)
    instead of the likelihood conditional on each customer's own (lambda, mu), on the GPU
    (``clv_marginal_information_criteria``: the matrix never leaves the device; the same bits as
    :func:`psis_loo` of it).  With one observation and one parameter pair per customer the conditional
    importance ratios of :func:`information_criteria` have no usable tail (Vehtari et al. 2017,
    section 2.4; Merkle, Furr & Rabe-Hesketh 2019); leaving a customer out of the marginal
    likelihood perturbs only the posterior of (beta, Sigma).

    Returns the dict of :func:`ic_frames` plus ``"kind": "marginal"``, which :func:`compare_models`
    takes as it is — among marginal entries only (``ParetoNBDFitter.information_criteria`` is one)."""
    level2, D, K, x, t_x, T_cal, cov, log_s, w2 = marginal_problem(draws, cbs, covariates, spend, omega2)
    q = marginal_nodes(nodes)
    par = ic_params(False, None, reff)
    R, n = level2.shape[0], x.shape[0]
    _ic_shape(R, n, 4, False, par["reff"])
    L = _L()
    out = np.empty((n, len(_lib.IC_STATS)), np.float64)
    check(L.clv_marginal_information_criteria(int(device), dptr(level2), D, K, dptr(cov), R, n, _i32p(x), dptr(t_x),
                                              dptr(T_cal), dptr(log_s), w2, q, par["reff"], dptr(out)))
    return marginal_frames(out, R)


def marginal_log_score(draws, cbs_new: pd.DataFrame, covariates=None, *, spend: bool = False, omega2=None,
                       nodes=None, device: int = -1) -> Dict[str, Any]:
    """The out-of-sample log score of customers the fit has not seen, without running any MH: per
    customer ``log_score = logsumexp_r l_marg[r] - log R`` over the R level-2 records (the maximum
    over the records, then the terms added in record order) — the log of the posterior predictive
    density of that customer's (x, t_x [, log_s]) — and in total with its standard error
    ``sqrt(N var(., ddof 0))``, both through :func:`fixed_order_sum`.

    Returns ``{"pointwise": DataFrame(log_score), "total": one-row DataFrame (log_score, se,
    n_records, n_customers)}``."""
    lm = marginal_log_likelihood(draws, cbs_new, covariates, spend=spend, omega2=omega2, nodes=nodes, device=device)
    R, n = lm.shape
    m = lm.max(axis=0)
    acc = np.zeros(n)
    for r in range(R):
        acc = acc + np.exp(lm[r] - m)
    score = (m + np.log(acc)) - np.log(float(R))
    total = fixed_order_sum(score)
    dev = score - total / n
    se = float(np.sqrt(n * (fixed_order_sum(dev * dev) / n)))
    return dict(pointwise=pd.DataFrame(dict(log_score=score)),
                total=pd.DataFrame([dict(log_score=total, se=se, n_records=int(R), n_customers=int(n))]))


# ---- the closed-form holdout forecast and its scores (csrc/forecast.hip) ---------------------
def forecast_params(T_star=39.0, x_star=None, k_max=None, pmf=False, cbs=None, n: Optional[int] = None) -> dict:
    """T_star / x_star / k_max of :func:`forecast`, validated (ValueError) on the host.  ``x_star`` may
    name a column of ``cbs``; ``k_max=None`` gives ``64 ceil((max(63, max x*) + 1) / 64)``."""
    t = float(T_star)
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"T_star must be finite and > 0 (got {T_star!r})")
    xs = None
    if x_star is not None:
        if isinstance(x_star, str):
            if cbs is None or x_star not in cbs:
                raise ValueError(f"x_star names the column {x_star!r}, which cbs does not have")
            x_star = cbs[x_star].to_numpy()
        v = np.asarray(x_star)
        if v.ndim != 1 or (n is not None and v.shape[0] != n):
            raise ValueError("x_star must hold one count per customer")
        if v.size and (not np.all(np.isfinite(v)) or np.any(v < 0) or np.any(v != np.floor(v))):
            raise ValueError("x_star must hold non-negative whole numbers")
        if v.size and v.max() >= _lib.FC_MAX_K:
            raise ValueError(f"x_star reaches {int(v.max())}: the forecast covers counts below {_lib.FC_MAX_K}")
        xs = np.ascontiguousarray(v, dtype=np.int32)
    if k_max is None:
        top = 63 if xs is None or xs.size == 0 else max(63, int(xs.max()))
        k_max = 64 * -(-(top + 1) // 64)
    if int(k_max) != k_max or not 1 <= int(k_max) <= _lib.FC_MAX_K:
        raise ValueError(f"k_max must be a whole number in [1, {_lib.FC_MAX_K}] (got {k_max!r})")
    k_max = int(k_max)
    if xs is not None and xs.size and int(xs.max()) >= k_max:
        raise ValueError(f"x_star reaches {int(xs.max())}, outside [0, k_max = {k_max})")
    return dict(T_star=t, x_star=xs, k_max=k_max, pmf=bool(pmf))


def forecast_frames(stats: np.ndarray, pmf: Optional[np.ndarray], n_samples: int, has_x_star: bool) -> dict:
    """The per-customer columns [n][len(_lib.FC_STATS)] as {"pointwise", "scores", "frequency",
    "pmf"}.  ``scores`` (one row, sums by :func:`fixed_order_sum`): log_score = the sum of the
    customers' log scores, se = sqrt(N var(., ddof 0)), rps = the mean ranked probability score,
    coverage_90 = the share of customers with q05 <= x* <= q95, n_samples, n_data_points; the score
    columns are NaN without x_star.  ``frequency`` (with the pmf only): the expected number of
    customers with k purchases, k = 0 ... k_max - 1, and a last entry ">=k_max" from the tail
    masses."""
    pw = pd.DataFrame(stats, columns=list(_lib.FC_STATS))
    n = stats.shape[0]
    row = dict(log_score=np.nan, se=np.nan, rps=np.nan, coverage_90=np.nan)
    if has_x_star:
        ls = pw["log_score"].to_numpy()
        tot = fixed_order_sum(ls)
        dev = ls - tot / n
        # q05 <= x* is F(x*) >= 0.05, x* <= q95 is F(x* - 1) < 0.95
        lo = np.where(pw["pit_hi"].to_numpy() >= 0.05, 1.0, 0.0)
        hi = np.where(pw["pit_lo"].to_numpy() < 0.95, 1.0, 0.0)
        row = dict(log_score=tot, se=float(np.sqrt(n * (fixed_order_sum(dev * dev) / n))),
                   rps=fixed_order_sum(pw["rps"].to_numpy()) / n, coverage_90=fixed_order_sum(lo * hi) / n)
    row.update(n_samples=int(n_samples), n_data_points=int(n))
    freq = None
    if pmf is not None:
        vals = [fixed_order_sum(pmf[:, k]) for k in range(pmf.shape[1])]
        vals.append(fixed_order_sum(pw["tail_mass"].to_numpy()))
        freq = pd.Series(vals, index=pd.Index(list(range(pmf.shape[1])) + [f">={pmf.shape[1]}"], name="x_star"),
                         name="expected_customers")
    return dict(pointwise=pw, scores=pd.DataFrame([row]), frequency=freq, pmf=pmf)


def forecast(draws: Dict[str, Any], cbs: pd.DataFrame, T_star: float = 39.0, *, x_star=None, k_max=None,
             pmf: bool = False, device: int = -1) -> Dict[str, Any]:
    """The posterior predictive distribution of every customer's number of purchases in the
    ``T_star`` periods after calibration, in closed form, on the GPU (``csrc/forecast.hip``,
    ``clv_forecast``): given a draw's (lambda, mu) the count is marginal over z and tau — a customer
    alive at T_cal may still drop out during the holdout, unlike in
    :func:`draw_future_transactions`, which restates the reference's simulation (there a customer
    whose sampled z is 1 buys for the whole of T_star) — and the distribution is the mean over the
    draws, not a sample.  ``x_star`` (an array, or the name of a CBS column) adds the scores of the
    realised counts; ``k_max`` is the number of counts covered (default
    ``64 ceil((max(63, max x*) + 1) / 64)``, at most 4096); ``pmf=True`` also returns the
    (n_customers, k_max) distribution.

    Returns ``{"pointwise": DataFrame, one row per customer, columns _lib.FC_STATS (xstar_mean,
    p_alive, p_zero, q05, q50, q95, tail_mass; log_score, pit_lo, pit_hi, rps with x_star),
    "scores", "frequency", "pmf"}`` (:func:`forecast_frames`; "frequency" needs the pmf and is None
    without it).  Arguments are checked before any device is touched."""
    a = _stacked_level1(draws.get("level_1"))
    nd, n, w = a.shape
    x, t_x, T_cal, _ = _ic_data(cbs, n, False)
    par = forecast_params(T_star, x_star, k_max, pmf, cbs, n)
    L = _L()
    out = np.empty((n, len(_lib.FC_STATS)), np.float64)
    dist = np.empty((n, par["k_max"]), np.float64) if par["pmf"] else None
    xs = par["x_star"]
    check(L.clv_forecast(int(device), dptr(a), nd, n, w, _i32p(x), dptr(t_x), dptr(T_cal), par["T_star"],
                         par["k_max"], None if xs is None else _i32p(xs), dptr(out), dptr(dist)))
    return forecast_frames(out, dist, nd, xs is not None)


def forecast_pit(fc: Dict[str, Any], bins: int = 10, seed: int = 0) -> pd.Series:
    """The randomised probability integral transform histogram of a scored :func:`forecast`:
    u_i = pit_lo + v_i (pit_hi - pit_lo) with v_i uniform (numpy's default_rng(seed)), counted in
    ``bins`` equal bins of [0, 1].  A calibrated forecast gives a flat histogram.  Host numpy."""
    pw = fc["pointwise"]
    lo, hi = pw["pit_lo"].to_numpy(), pw["pit_hi"].to_numpy()
    if int(bins) < 1:
        raise ValueError("bins must be >= 1")
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("the forecast carries no PIT values (it was made without x_star, or a customer is NaN)")
    u = lo + np.random.default_rng(seed).random(len(lo)) * (hi - lo)
    counts, edges = np.histogram(np.clip(u, 0.0, 1.0), bins=int(bins), range=(0.0, 1.0))
    return pd.Series(counts, index=pd.Index(edges[:-1], name="pit_bin_left"), name="customers")


def compare_forecasts(forecasts: Dict[str, Dict[str, Any]]) -> pd.DataFrame:
    """Rank forecasts of the same customers' holdout counts by their total log score, best first:
    rank, log_score, ``diff`` = the best forecast's log score minus this one's,
    ``dse = sqrt(N var(log_score_i - log_score_best,i, ddof 0))`` from the paired per-customer
    values, se and rps (:func:`compare_models` for the out-of-sample score)."""
    if not forecasts:
        raise ValueError("no forecast to compare")
    point = {k: f["pointwise"]["log_score"].to_numpy() for k, f in forecasts.items()}
    sizes = {len(v) for v in point.values()}
    if len(sizes) != 1:
        raise ValueError(f"the forecasts cover different numbers of customers: {sorted(sizes)}")
    if any(np.isnan(v).all() for v in point.values()):
        raise ValueError("a forecast carries no log score (it was made without x_star)")
    n = sizes.pop()
    total = {k: float(f["scores"]["log_score"].iloc[0]) for k, f in forecasts.items()}
    order = sorted(forecasts, key=lambda k: -total[k])
    best = order[0]
    rows = []
    for r, k in enumerate(order):
        sc = forecasts[k]["scores"].iloc[0]
        diff = point[best] - point[k]
        rows.append(dict(rank=r, log_score=total[k], diff=total[best] - total[k],
                         dse=float(np.sqrt(n * np.var(diff))), se=float(sc["se"]), rps=float(sc["rps"])))
    return pd.DataFrame(rows, index=pd.Index(order, name="model"))


def forecast_table(fc: Dict[str, Any], cbs: pd.DataFrame, pool_from: int = 7) -> Dict[str, Any]:
    """Table 2's disaggregate rows and Figure 3's data from the posterior mean forecast
    (``xstar_mean``) and the realised ``cbs["x_star"]``: ``{"metrics": one-row DataFrame correlation
    (Pearson) and mse, "by_frequency": DataFrame indexed by calibration x (0 ... pool_from - 1 and
    "7+" pooled) with n, actual = mean x_star, predicted = mean xstar_mean}``
    (analysis_abe.py compute_metrics and its conditional-expectation figure).  Host numpy."""
    if "x_star" not in cbs or "x" not in cbs:
        raise ValueError("cbs needs the columns x and x_star")
    pred = fc["pointwise"]["xstar_mean"].to_numpy()
    act = cbs["x_star"].to_numpy(float)
    x = cbs["x"].to_numpy()
    if not (len(pred) == len(act) == len(x)):
        raise ValueError("cbs and the forecast disagree on the number of customers")
    corr = float(np.corrcoef(act, pred)[0, 1]) if len(act) > 1 else float("nan")
    metrics = pd.DataFrame([dict(correlation=corr, mse=float(np.mean((act - pred) ** 2)))])
    rows, labels = [], []
    for k in range(int(pool_from) + 1):
        sel = x >= pool_from if k == pool_from else x == k
        if not sel.any():
            continue
        labels.append(f"{pool_from}+" if k == pool_from else str(k))
        rows.append(dict(n=int(sel.sum()), actual=float(act[sel].mean()), predicted=float(pred[sel].mean())))
    return dict(metrics=metrics, by_frequency=pd.DataFrame(rows, index=pd.Index(labels, name="x")))


# ---- posterior predictive checks of the calibration data (csrc/ppc.hip) ----------------------
PPC_STATISTICS = ("share_zero", "total_x", "max_x", "var_x", "mean_recency")


def ppc_params(level="customer", k_hist=None, seed=0, replicates=False, customer_offset=0, x=None,
               n: Optional[int] = None) -> dict:
    """level / k_hist / seed / customer_offset of :func:`posterior_predictive_check`, validated
    (ValueError) on the host.  ``k_hist=None`` gives ``max(8, min(int(x.max()) + 1, 256))`` (8 without
    ``x``)."""
    if level not in _lib.PPC_LEVELS:
        raise ValueError(f"level must be one of {sorted(_lib.PPC_LEVELS)} (got {level!r})")
    if k_hist is None:
        k_hist = 8 if x is None or len(x) == 0 else max(8, min(int(np.max(x)) + 1, 256))
    if isinstance(k_hist, bool) or int(k_hist) != k_hist or not 1 <= int(k_hist) <= _lib.PPC_MAX_K:
        raise ValueError(f"k_hist must be a whole number in [1, {_lib.PPC_MAX_K}] (got {k_hist!r})")
    off = int(customer_offset)
    if off < 0 or off + int(n or 0) > 1 << 32:
        raise ValueError("customer_offset + N must fit in 32 bits")
    return dict(level=level, k_hist=int(k_hist), seed=resolve_seed(seed), replicates=bool(replicates),
                customer_offset=off)


def _ppc_data(cbs: pd.DataFrame):
    """x (int32), t_x, T_cal of the calibration CBS, checked."""
    for col in ("x", "t_x", "T_cal"):
        if col not in cbs:
            raise ValueError(f"cbs has no column {col!r}")
    if len(cbs) < 1:
        raise ValueError("no customer")
    xv = cbs["x"].to_numpy()
    if np.any(xv < 0) or np.any(xv > np.iinfo(np.int32).max) or np.any(xv != np.round(xv)):
        raise ValueError("x must hold non-negative integer counts")
    return (np.ascontiguousarray(xv, dtype=np.int32), np.ascontiguousarray(cbs["t_x"].to_numpy(float)),
            np.ascontiguousarray(cbs["T_cal"].to_numpy(float)))


def ppc_outputs(nd: int, n: int, k_hist: int, replicates: bool):
    """(customers, draws_int, draws_f, x_rep or None, t_x_rep or None) host buffers of a check."""
    return (np.empty((n, len(_lib.PPC_STATS)), np.float64),
            np.empty((nd, k_hist + 1 + len(_lib.PPC_DRAW_INTS)), np.int64),
            np.empty((nd, len(_lib.PPC_DRAW_FLOATS)), np.float64),
            np.empty((nd, n), np.int64) if replicates else None,
            np.empty((nd, n), np.float64) if replicates else None)


def _ppc_statistics(n: int, n_zero, sum_x, sum_x2, max_x, sum_tx) -> dict:
    """The test statistics of one data set (or, vectorised, of every replicate) from its sums:
    share_zero = n_zero / n, total_x, max_x, var_x = sum_x2 / n - (sum_x / n)^2 (ddof 0),
    mean_recency = sum_tx / (n - n_zero), NaN when nobody repeats."""
    n_zero, sum_x, sum_x2 = (np.asarray(v, dtype=np.float64) for v in (n_zero, sum_x, sum_x2))
    rep = n - n_zero
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.where(rep > 0, np.asarray(sum_tx, dtype=np.float64) / np.where(rep > 0, rep, 1.0), np.nan)
    mean = sum_x / n
    return dict(share_zero=n_zero / n, total_x=sum_x, max_x=np.asarray(max_x, dtype=np.float64),
                var_x=sum_x2 / n - mean * mean, mean_recency=rec)


def ppc_frames(cust: np.ndarray, draws_int: np.ndarray, draws_f: np.ndarray, x, t_x, k_hist: int, level: str,
               seed: int, x_rep=None, t_x_rep=None) -> Dict[str, Any]:
    """The outputs of ``clv_ppc`` as the return value of :func:`posterior_predictive_check`; ``x`` and
    ``t_x`` are the observed calibration data, from which ``observed`` is computed by the replicates'
    own definitions (the recency sum by :func:`fixed_order_sum`)."""
    x = np.asarray(x, dtype=np.int64)
    n, nd = len(x), draws_int.shape[0]
    hist = draws_int[:, :k_hist + 1]
    ints = {k: draws_int[:, k_hist + 1 + j] for j, k in enumerate(_lib.PPC_DRAW_INTS)}
    sum_tx = draws_f[:, _lib.PPC_DRAW_FLOATS.index("sum_tx")]
    rep = _ppc_statistics(n, hist[:, 0], ints["sum_x"], ints["sum_x2"], ints["max_x"], sum_tx)
    draws = pd.DataFrame(dict(n_zero=hist[:, 0], total_x=ints["sum_x"], max_x=ints["max_x"], n_alive=ints["n_alive"],
                              var_x=rep["var_x"], mean_recency=rep["mean_recency"]))
    obs_hist = np.bincount(np.minimum(x, k_hist), minlength=k_hist + 1)
    pct = np.percentile(hist, [5.0, 50.0, 95.0], axis=0)
    freq = pd.DataFrame(dict(observed=obs_hist, rep_mean=hist.mean(axis=0), rep_p05=pct[0], rep_p50=pct[1],
                             rep_p95=pct[2]),
                        index=pd.Index(list(range(k_hist)) + [f"{k_hist}+"], name="x"))
    obs = _ppc_statistics(n, int(np.count_nonzero(x == 0)), int(x.sum()), int((x * x).sum()), int(x.max()),
                          fixed_order_sum(np.asarray(t_x, dtype=np.float64)))
    rows = []
    for name in PPC_STATISTICS:
        r, o = np.asarray(rep[name], dtype=np.float64), float(obs[name])
        ok = ~np.isnan(r)
        m = int(ok.sum())
        if m == 0 or np.isnan(o):
            rows.append(dict(observed=o, rep_mean=np.nan, rep_sd=np.nan, p_value=np.nan, p_mid=np.nan))
            continue
        gt, eq = np.count_nonzero(r[ok] > o), np.count_nonzero(r[ok] == o)
        rows.append(dict(observed=o, rep_mean=float(r[ok].mean()), rep_sd=float(r[ok].std(ddof=1)) if m > 1 else np.nan,
                         p_value=(gt + eq) / m, p_mid=(gt + 0.5 * eq) / m))
    out = dict(customers=pd.DataFrame(cust, columns=list(_lib.PPC_STATS)), frequency=freq, draws=draws,
               statistics=pd.DataFrame(rows, index=pd.Index(list(PPC_STATISTICS), name="statistic")),
               level=level, n_samples=int(nd), seed=int(seed))
    if x_rep is not None:
        out["x_rep"], out["t_x_rep"] = x_rep, t_x_rep
    return out


def posterior_predictive_check(draws: Dict[str, Any], cbs: pd.DataFrame, covariates=None, *, level: str = "customer",
                               k_hist=None, seed: Optional[int] = 0, replicates: bool = False,
                               customer_offset: int = 0, device: int = -1) -> Dict[str, Any]:
    """Posterior predictive checks of the calibration data, on the GPU (``csrc/ppc.hip``, ``clv_ppc``):
    for every stacked draw one replicate (x_rep, t_x_rep) of every customer's (x, t_x) on (0, T_cal] —
    a lifetime tau ~ Exp(mu), x_rep ~ Poisson(lambda min(tau, T_cal)) purchases and the last of them
    — and what the replicated data sets look like next to the observed one.

    ``level="customer"`` replicates each customer from their own level-1 draws (lambda_i, mu_i): a
    check of the Poisson / exponential individual model.  ``level="population"`` is the mixed
    replicate: for each level-2 record (beta, Sigma) of ``draws["level_2"]`` a new
    (lambda, mu) ~ LogNormal(beta' d_i, Sigma) for every customer's covariates d_i (``covariates``: the
    fit's covariate columns of ``cbs``) — a check of the log-normal heterogeneity and the covariate
    regression, which level-1 draws, adapting to each customer's own data, cannot give.

    Returns a dict: ``customers`` (one row per customer, columns _lib.PPC_STATS: x_rep_mean, p_x_lt =
    P(x_rep < x), p_x_eq, p_zero, tx_rep_mean, p_tx_le = P(t_x_rep <= t_x), p_alive_rep);
    ``frequency`` (index 0 ... k_hist - 1 and "{k_hist}+": the observed number of customers with that
    many repeat purchases and the mean, 5 / 50 / 95 % points of the replicated numbers over the
    draws); ``draws`` (one row per replicated data set: n_zero, total_x, max_x, n_alive, var_x,
    mean_recency = sum t_x_rep / (n - n_zero), NaN when nobody repeats); ``statistics`` (one row per
    test statistic share_zero, total_x, max_x, var_x (ddof 0), mean_recency: observed, rep_mean,
    rep_sd, p_value = P(T_rep >= T_obs), p_mid = P(>) + P(=) / 2, over the replicates where the
    statistic is defined); ``level``, ``n_samples``, ``seed``; and with ``replicates=True`` the
    (n_draws, n) arrays ``x_rep`` (int64) and ``t_x_rep``.  ``k_hist`` defaults to
    ``max(8, min(max x + 1, 256))``, at most 4096.  The variates are a function of (seed,
    customer_offset + i, stacked draw) alone: shard a customer base with ``customer_offset`` (the
    per-draw integer columns of the shards add up).  Arguments are checked before any device is
    touched."""
    if level not in _lib.PPC_LEVELS:
        raise ValueError(f"level must be one of {sorted(_lib.PPC_LEVELS)} (got {level!r})")
    l1 = l2 = cov = None
    w = D = K = 0
    if level == "customer":
        x, t_x, T_cal = _ppc_data(cbs)
        l1 = _stacked_level1(draws.get("level_1") if isinstance(draws, dict) else draws)
        nd, n, w = l1.shape
        if n != x.shape[0]:
            raise ValueError("cbs and draws disagree on the number of customers")
    else:
        rec = score_level2(draws)
        l2 = np.ascontiguousarray(rec.reshape(-1, rec.shape[2]))
        D, K, x, t_x, T_cal, cov, _ = score_problem(cbs, covariates, rec.shape[2])
        nd, n = l2.shape[0], x.shape[0]
    par = ppc_params(level, k_hist, seed, replicates, customer_offset, x, n)
    L = _L()
    cust, di, df, xr, tr = ppc_outputs(nd, n, par["k_hist"], par["replicates"])
    check(L.clv_ppc(int(device), _lib.PPC_LEVELS[level], dptr(l1), int(w), dptr(l2), int(D), int(K), dptr(cov), nd, n,
                    _i32p(x), dptr(t_x), dptr(T_cal), par["k_hist"], par["seed"], par["customer_offset"], dptr(cust),
                    _i64p(di), dptr(df), None if xr is None else _i64p(xr), dptr(tr)))
    return ppc_frames(cust, di, df, x, t_x, par["k_hist"], level, par["seed"], xr, tr)


def ppc_pit(ppc: Dict[str, Any], bins: int = 10, seed: int = 0) -> pd.Series:
    """The randomised probability integral transform histogram of the calibration counts under a
    :func:`posterior_predictive_check`: u_i = p_x_lt + v_i p_x_eq with v_i uniform (numpy's
    default_rng(seed)), counted in ``bins`` equal bins of [0, 1].  A model that replicates the
    customers' counts gives a flat histogram.  Host numpy."""
    cu = ppc["customers"]
    lo, eq = cu["p_x_lt"].to_numpy(), cu["p_x_eq"].to_numpy()
    if int(bins) < 1:
        raise ValueError("bins must be >= 1")
    if np.isnan(lo).any() or np.isnan(eq).any():
        raise ValueError("the check carries no PIT values (a customer is NaN)")
    u = lo + np.random.default_rng(seed).random(len(lo)) * eq
    counts, edges = np.histogram(np.clip(u, 0.0, 1.0), bins=int(bins), range=(0.0, 1.0))
    return pd.Series(counts, index=pd.Index(edges[:-1], name="pit_bin_left"), name="customers")


# ---- convergence diagnostics (csrc/diag.hip) -------------------------------------------------
LEVEL1_PARAMS = ("lambda", "mu", "tau", "z", "eta")


def level1_log_mask(log_columns, width: int) -> int:
    """Bit i set = level-1 column i (lambda, mu, tau, z[, eta]) is logged before the statistics."""
    names = LEVEL1_PARAMS[:width]
    mask = 0
    for c in log_columns or ():
        if c not in names:
            raise ValueError(f"log_columns entries must be among {names} (got {c!r})")
        mask |= 1 << names.index(c)
    return mask


def level1_diagnostics_frame(stats: np.ndarray, n: int, width: int, log_mask: int) -> pd.DataFrame:
    """[n * width][6] statistics -> one row per customer, columns f"{stat}_{param}"."""
    a = np.asarray(stats).reshape(n, width, len(_lib.DIAG_STATS))
    cols = {}
    for j, nm in enumerate(LEVEL1_PARAMS[:width]):
        pname = f"log_{nm}" if (log_mask >> j) & 1 else nm
        for k, st in enumerate(_lib.DIAG_STATS):
            cols[f"{st}_{pname}"] = a[:, j, k]
    return pd.DataFrame(cols)


def level2_diagnostics_frame(stats: np.ndarray, param_names=None) -> pd.DataFrame:
    a = np.asarray(stats)
    names = list(param_names) if param_names is not None else [f"level_2[{i}]" for i in range(a.shape[0])]
    if len(names) != a.shape[0]:
        raise ValueError(f"param_names has {len(names)} entries for {a.shape[0]} level-2 parameters")
    return pd.DataFrame(a, columns=list(_lib.DIAG_STATS), index=names)


def _chains_array(chains_list) -> np.ndarray:
    """A draws list (one array per chain, equal shapes) as one C-contiguous [chain][draw][...] array."""
    if chains_list is None:
        raise ValueError("level-1 draws are needed (run the sampler with draw_sink='full')")
    return np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in chains_list], axis=0))


def _diagnostics(a: np.ndarray, n_series: int, period: int, log_mask: int, device: int) -> np.ndarray:
    L = _L()
    out = np.empty((n_series, len(_lib.DIAG_STATS)), np.float64)
    check(L.clv_diagnostics(int(device), dptr(a), a.shape[0], a.shape[1], n_series, period, log_mask, dptr(out)))
    return out


def level1_diagnostics(draws: Dict[str, Any], *, log_columns=("lambda", "mu"), device: int = -1) -> pd.DataFrame:
    """Per-customer convergence diagnostics of the level-1 draws, on the GPU (``csrc/diag.hip``).

    One row per customer; columns ``f"{stat}_{param}"`` with stat in mean, sd, mcse, ess, rhat, lag
    and param in log_lambda, log_mu, tau, z (and eta for the trivariate model) — a column that is
    not in ``log_columns`` keeps its plain name (``lambda``, ``mu``).

    The estimator is the split-chain R-hat and the mean effective sample size of BDA3 / Stan /
    ArviZ WITHOUT rank normalisation: every chain is split in halves, the biased autocovariances of
    the split chains are averaged, Geyer's initial positive sequence is cut at ``lag`` and made
    monotone, ``ess = M h / tau``, ``mcse = sd / sqrt(ess)``.  ``az.summary`` reports the
    rank-normalised variants: those are :func:`level1_rank_diagnostics` (R-hat and ESS of arbitrary
    quantiles stay out of scope).  The estimator is meant for the scales the sampler works on — log lambda, log mu and the
    level-2 parameters — hence the default ``log_columns``.  A series with a non-finite value or no
    within-chain variance (a customer whose ``z`` never changes) gives NaN in all six statistics.
    Needs at least 8 draws per chain."""
    a = _chains_array(draws.get("level_1"))
    if a.ndim != 4 or a.shape[3] not in (4, 5):
        raise ValueError("level_1 draws must be (n_draws, n_customers, 4 or 5) per chain")
    n, w = a.shape[2], a.shape[3]
    mask = level1_log_mask(log_columns, w)
    return level1_diagnostics_frame(_diagnostics(a, n * w, w, mask, device), n, w, mask)


def level2_diagnostics(draws: Dict[str, Any], param_names=None, *, device: int = -1) -> pd.DataFrame:
    """The project's ``az.summary`` of the level-2 draws (bivariate/analysis_abe.py:651-706): one row
    per level-2 parameter with mean, sd, mcse, ess, rhat and the truncation lag — the estimator of
    :func:`level1_diagnostics` (not rank-normalised, unlike az.summary's ess_bulk / ess_tail /
    r_hat: :func:`level2_summary` has those, in az.summary's nine columns), on the parameters as
    drawn."""
    a = _chains_array(draws["level_2"])
    if a.ndim != 3:
        raise ValueError("level_2 draws must be (n_draws, n_params) per chain")
    return level2_diagnostics_frame(_diagnostics(a, a.shape[2], 1, 0, device), param_names)


# ---- rank-normalised diagnostics (csrc/diag.hip, clv_rank_diagnostics) -------------------------
def _check_hdi_prob(hdi_prob) -> float:
    p = float(hdi_prob)
    if not 0.0 < p < 1.0:
        raise ValueError(f"hdi_prob must be in (0, 1) (got {hdi_prob!r})")
    return p


def hdi_column_names(hdi_prob: float = 0.94):
    """ArviZ's names of the two HDI columns: ("hdi_3%", "hdi_97%") at 0.94."""
    p = _check_hdi_prob(hdi_prob)
    return f"hdi_{100 * (1 - p) / 2:g}%", f"hdi_{100 * (1 - (1 - p) / 2):g}%"


def level1_rank_diagnostics_frame(stats: np.ndarray, n: int, width: int, log_mask: int) -> pd.DataFrame:
    """[n * width][13] rank statistics -> one row per customer, columns f"{stat}_{param}"."""
    a = np.asarray(stats).reshape(n, width, len(_lib.RANK_STATS))
    cols = {}
    for j, nm in enumerate(LEVEL1_PARAMS[:width]):
        pname = f"log_{nm}" if (log_mask >> j) & 1 else nm
        for k, st in enumerate(_lib.RANK_STATS):
            cols[f"{st}_{pname}"] = a[:, j, k]
    return pd.DataFrame(cols)


def _level2_names(n_params: int, param_names):
    names = list(param_names) if param_names is not None else [f"level_2[{i}]" for i in range(n_params)]
    if len(names) != n_params:
        raise ValueError(f"param_names has {len(names)} entries for {n_params} level-2 parameters")
    return names


def level2_rank_diagnostics_frame(stats: np.ndarray, param_names=None) -> pd.DataFrame:
    a = np.asarray(stats)
    return pd.DataFrame(a, columns=list(_lib.RANK_STATS), index=_level2_names(a.shape[0], param_names))


SUMMARY_COLUMNS = ("mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat")


def level2_summary_frame(stats: np.ndarray, rank_stats: np.ndarray, param_names=None,
                         hdi_prob: float = 0.94) -> pd.DataFrame:
    """az.summary's nine columns from the [P][6] statistics of clv_diagnostics (mean, sd, mcse_mean)
    and the [P][13] of clv_rank_diagnostics (the rest)."""
    d, r = np.asarray(stats), np.asarray(rank_stats)
    D, K = _lib.DIAG_STATS.index, _lib.RANK_STATS.index
    lo, hi = hdi_column_names(hdi_prob)
    cols = {"mean": d[:, D("mean")], "sd": d[:, D("sd")], lo: r[:, K("hdi_lo")], hi: r[:, K("hdi_hi")],
            "mcse_mean": d[:, D("mcse")], "mcse_sd": r[:, K("mcse_sd")], "ess_bulk": r[:, K("ess_bulk")],
            "ess_tail": r[:, K("ess_tail")], "r_hat": r[:, K("rhat")]}
    return pd.DataFrame(cols, index=_level2_names(d.shape[0], param_names))


def _rank_diagnostics(a: np.ndarray, n_series: int, period: int, log_mask: int, hdi_prob: float,
                      device: int) -> np.ndarray:
    L = _L()
    out = np.empty((n_series, len(_lib.RANK_STATS)), np.float64)
    check(L.clv_rank_diagnostics(int(device), dptr(a), a.shape[0], a.shape[1], n_series, period, log_mask,
                                 float(hdi_prob), dptr(out)))
    return out


def level1_rank_diagnostics(draws: Dict[str, Any], *, log_columns=("lambda", "mu"), hdi_prob: float = 0.94,
                            device: int = -1) -> pd.DataFrame:
    """Per-customer rank-normalised diagnostics of the level-1 draws, on the GPU (``csrc/diag.hip``,
    ``clv_rank_diagnostics``): what ``az.summary`` computes per variable — Vehtari, Gelman, Simpson,
    Carpenter & Buerkner (2021) as ArviZ implements them — for every customer's series.

    One row per customer; columns ``f"{stat}_{param}"``, params as in :func:`level1_diagnostics`,
    stats ``rhat`` (the larger of ``rhat_bulk``, the split R-hat of the rank-normalised draws, and
    ``rhat_folded``, that of the rank-normalised absolute deviations from the median), ``ess_bulk``
    with its truncation lag ``lag_bulk``, ``ess_tail`` (the smaller of ``ess_q05`` and ``ess_q95``,
    the ESS of the indicators of the 5 % and 95 % quantiles), ``ess_sd`` and ``mcse_sd``, the
    highest-density interval ``hdi_lo`` / ``hdi_hi`` of probability ``hdi_prob`` and the
    ``median``.  Ranks are invariant under the log, so ``log_columns`` only moves ``mcse_sd``,
    ``ess_sd``, the HDI and the median to the log scale.  A series with a non-finite value is NaN
    throughout; otherwise a statistic is NaN exactly when its own transformed series has no
    within-chain variance — a binary ``z`` usually has a NaN ``ess_q95`` (and so ``ess_tail``):
    every draw is at or below its 95 % quantile."""
    a = _chains_array(draws.get("level_1"))
    if a.ndim != 4 or a.shape[3] not in (4, 5):
        raise ValueError("level_1 draws must be (n_draws, n_customers, 4 or 5) per chain")
    n, w = a.shape[2], a.shape[3]
    mask = level1_log_mask(log_columns, w)
    p = _check_hdi_prob(hdi_prob)
    return level1_rank_diagnostics_frame(_rank_diagnostics(a, n * w, w, mask, p, device), n, w, mask)


def _level2_array(draws) -> np.ndarray:
    a = _chains_array(draws["level_2"])
    if a.ndim != 3:
        raise ValueError("level_2 draws must be (n_draws, n_params) per chain")
    return a


def level2_rank_diagnostics(draws: Dict[str, Any], param_names=None, *, hdi_prob: float = 0.94,
                            device: int = -1) -> pd.DataFrame:
    """Every rank-normalised statistic of :func:`level1_rank_diagnostics` for the level-2 parameters
    as drawn: one row per parameter, columns ``_lib.RANK_STATS``."""
    a = _level2_array(draws)
    p = _check_hdi_prob(hdi_prob)
    return level2_rank_diagnostics_frame(_rank_diagnostics(a, a.shape[2], 1, 0, p, device), param_names)


def level2_summary(draws: Dict[str, Any], param_names=None, *, hdi_prob: float = 0.94,
                   device: int = -1) -> pd.DataFrame:
    """The ``az.summary(idata, var_names=["level_2"])`` table of the reference
    (bivariate/analysis_abe.py:690-693): one row per level-2 parameter, columns ``mean, sd, hdi_3%,
    hdi_97%, mcse_mean, mcse_sd, ess_bulk, ess_tail, r_hat`` (the HDI names follow ``hdi_prob`` as
    ArviZ's do), with ArviZ's rank-normalised definitions of the last five; not rounded.  One
    ``clv_diagnostics`` and one ``clv_rank_diagnostics`` call."""
    a = _level2_array(draws)
    p = _check_hdi_prob(hdi_prob)
    names = _level2_names(a.shape[2], param_names)
    return level2_summary_frame(_diagnostics(a, a.shape[2], 1, 0, device),
                                _rank_diagnostics(a, a.shape[2], 1, 0, p, device), names, p)


def level2_autocorr(draws: Dict[str, Any], max_lag: int = 100, *, device: int = -1) -> np.ndarray:
    """Per-chain autocorrelation of every level-2 parameter (what ``az.plot_autocorr`` draws,
    analysis_abe.py:693-703): ``[chain][param][max_lag + 1]``, A_c(t) / A_c(0) of the unsplit chain
    centred at its mean with divisor n.  ``max_lag`` must be below the number of draws."""
    L = _L()
    a = _chains_array(draws["level_2"])
    if a.ndim != 3:
        raise ValueError("level_2 draws must be (n_draws, n_params) per chain")
    out = np.empty((a.shape[0], a.shape[2], max(int(max_lag), 0) + 1), np.float64)
    check(L.clv_autocorr(int(device), dptr(a), a.shape[0], a.shape[1], a.shape[2], int(max_lag), dptr(out)))
    return out


def summarize_level2(draws_level2: np.ndarray, param_names, decimals: int = 2) -> pd.DataFrame:
    """analysis_bi_helpers.py:6-13 — 2.5 / 50 / 97.5 % quantiles of each level-2 parameter over the
    (stacked) draws, rounded.  Host numpy, as the reference."""
    quantiles = np.percentile(draws_level2, [2.5, 50, 97.5], axis=0)
    summary = pd.DataFrame(quantiles.T, columns=["2.5%", "50%", "97.5%"], index=param_names)
    return summary.round(decimals)


def extract_correlation(draws_level2: np.ndarray) -> np.ndarray:
    """analysis_bi_helpers.py:39-48 — 2.5 / 50 / 97.5 % quantiles of corr(log lambda, log mu) from the
    level-2 covariance draws (last three columns: var, cov, var), rounded to 2 decimals."""
    cov = draws_level2[:, -2]
    var_lambda = draws_level2[:, -3]
    var_mu = draws_level2[:, -1]
    corr = cov / np.sqrt(var_lambda * var_mu)
    return np.percentile(corr, [2.5, 50, 97.5]).round(2)


def summary_rhat(draws: Dict[str, Any]) -> pd.DataFrame:
    """Non-split R-hat of lambda and mu per customer for a ``draw_sink="summary"`` / ``"summary+pct"``
    result, where no draws exist and this is the only diagnostic available (host numpy).

    From the per-chain means of ``lambda``, ``lambda2``, ``mu``, ``mu2`` in ``draws["summary"]`` over
    n stored draws: within-chain variance s_c^2 = (E[x^2] - E[x]^2) n / (n - 1), W = mean_c s_c^2,
    B / n = var_c(E[x], ddof=1), R-hat = sqrt(((n - 1) / n W + B / n) / W).  NaN where the variance
    is not positive; needs at least 2 chains and 2 stored draws.

    ``E[x^2] - E[x]^2`` cancels: its absolute error is about 2^-52 E[x^2], so a chain whose
    coefficient of variation is below ~1e-7 loses every digit of its variance (and may come out
    zero or negative: NaN here).  The sampler's lambda and mu vary by tens of percent per customer,
    which leaves about 13 digits.  No split, no ESS: use ``draw_sink="full"`` and
    :func:`level1_diagnostics` for those."""
    sm = draws.get("summary")
    if not isinstance(sm, dict) or "lambda2" not in sm:
        raise ValueError("summary_rhat needs a draw_sink='summary' (or 'summary+pct') result")
    n = int(sm["n_draws"])
    out = {}
    for nm in ("lambda", "mu"):
        m1 = np.asarray(sm[nm], dtype=np.float64)
        m2 = np.asarray(sm[nm + "2"], dtype=np.float64)
        if m1.ndim != 2 or m1.shape[0] < 2:
            raise ValueError("summary_rhat needs at least 2 chains")
        if n < 2:
            raise ValueError("summary_rhat needs at least 2 stored draws")
        s2 = (m2 - m1 * m1) * (n / (n - 1.0))
        W = s2.mean(axis=0)
        B_n = m1.var(axis=0, ddof=1)
        ok = (s2 > 0).all(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.sqrt(((n - 1.0) / n * W + B_n) / W)
        out[f"rhat_{nm}"] = np.where(ok, r, np.nan)
    return pd.DataFrame(out)

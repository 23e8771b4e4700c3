"""float64 numpy model of csrc/ltv.hip (posterior customer lifetime value and customer equity), the
synthetic level-1 arrays its tests run on, and the error measures of the finite-horizon checks.

Per stacked draw and customer, from the level-1 row (lambda, mu, tau, z[, eta]), a = mu + delta:
    value    = (lambda m) / a                      infinite horizon: multiply, divide
             = ((lambda m) (-expm1(-(a H)))) / a   horizon H
    residual = z value
with m = eta value_scale (width 5) or monetary (width 4; ones without it).  Per customer over the
S draws: means as sequential sums in draw order / S (numpy's axis-0 reduction), numpy's std with
ddof 1 and numpy's 'linear' percentiles.  Per draw over the N customers: sums in the device's fixed
order (tests/pnbd_ref.py device_sum).
"""
from __future__ import annotations

import numpy as np

from tests.pnbd_ref import device_sum

STATS = ("value_mean", "value_sd", "value_p025", "value_p50", "value_p975", "residual_mean", "residual_sd",
         "residual_p025", "residual_p50", "residual_p975", "p_alive", "lifetime_yrs", "survival_1yr")
DRAW_STATS = ("equity", "value_total", "n_alive", "mu_share")
ULP = 2.0 ** -52


def synth_level1(S: int, N: int, width: int, seed: int = 0) -> np.ndarray:
    """[S][N][width] draws with CDNOW-like scales: lambda, mu log-normal (log-means -3.5, -3.7, log-sds
    1.2, 1.6: mu keeps its heavy tail), tau positive, z Bernoulli(0.45), eta log-normal(3.2, 0.7)."""
    g = np.random.default_rng([seed, S, N, width])
    a = np.empty((S, N, width))
    a[..., 0] = np.exp(g.normal(-3.5, 1.2, (S, N)))
    a[..., 1] = np.exp(g.normal(-3.7, 1.6, (S, N)))
    a[..., 2] = g.exponential(30.0, (S, N)) + 0.01
    a[..., 3] = (g.random((S, N)) < 0.45).astype(np.float64)
    if width == 5:
        a[..., 4] = np.exp(g.normal(3.2, 0.7, (S, N)))
    return a


def per_draw_terms(level1, delta, horizon=None, monetary=None, value_scale=1.0):
    """(value, residual, z, mu / a) as [S][N] arrays."""
    l1 = np.asarray(level1, np.float64)
    lam, mu, z = l1[..., 0], l1[..., 1], l1[..., 3]
    a = mu + delta
    if l1.shape[2] == 5:
        m = l1[..., 4] * value_scale
    else:
        m = np.ones(l1.shape[1]) if monetary is None else np.asarray(monetary, np.float64)
    v = lam * m
    if horizon is not None and np.isfinite(horizon):
        v = v * (-np.expm1(-(a * horizon)))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        v = v / a
        return v, z * v, z, mu / a


def seq_mean(x):
    """Sum over axis 0 in order, divided by the count (numpy's axis-0 mean of a C-contiguous 2-D
    array adds the rows in turn; written out so that the order is the model's, not numpy's)."""
    acc = np.zeros(x.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):
        for row in x:
            acc = acc + row
    return acc / float(x.shape[0])


def seq_std(x, mean):
    """numpy's std(axis=0, ddof=1), operation for operation; NaN at one draw."""
    acc = np.zeros(x.shape[1])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for row in x:
            d = row - mean
            acc = acc + d * d
        return np.sqrt(acc / float(x.shape[0] - 1))


def model(level1, delta, horizon=None, monetary=None, value_scale=1.0, periods_per_year=52.0):
    """(customers [N][13], draws [S][4]) in the column orders STATS / DRAW_STATS."""
    l1 = np.asarray(level1, np.float64)
    S, N = l1.shape[:2]
    v, r, z, share = per_draw_terms(l1, delta, horizon, monetary, value_scale)
    cust = np.empty((N, len(STATS)))
    for j, x in ((0, v), (5, r)):
        cust[:, j] = seq_mean(x)
        cust[:, j + 1] = seq_std(x, cust[:, j])
        cust[:, j + 2:j + 5] = np.percentile(x, [2.5, 50.0, 97.5], axis=0, method="linear").T
    pm = periods_per_year * l1[..., 1]
    cust[:, 10] = seq_mean(z)
    cust[:, 11] = seq_mean(1.0 / pm)
    cust[:, 12] = seq_mean(np.exp(-pm))
    draws = np.empty((S, len(DRAW_STATS)))
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(S):
            draws[d] = (device_sum(r[d]), device_sum(v[d]), device_sum(z[d]), device_sum(share[d]) / float(N))
    return cust, draws


def finite_horizon_errors(cust, draws, level1, delta, horizon, periods_per_year=52.0):
    """The measures of the finite-horizon check, device against model: dict name -> largest error.
    Means and percentiles of value / residual relative to the value (the model's statistic; where it
    is 0 the device must be 0 too: reported as 0 or inf), sd relative to sqrt(mean(v^2)), per-draw
    sums relative to sum |terms|, survival_1yr relative to itself."""
    mc, md = model(level1, delta, horizon, periods_per_year=periods_per_year)
    v, r, z, share = per_draw_terms(level1, delta, horizon)
    out = {}

    def rel(a, b, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.abs(a - b) / scale
        return float(np.where(a == b, 0.0, e).max())
    for j, x, nm in ((0, v, "value"), (5, r, "residual")):
        for k, st in ((0, "mean"), (2, "p025"), (3, "p50"), (4, "p975")):
            out[f"{nm}_{st}"] = rel(cust[:, j + k], mc[:, j + k], np.abs(mc[:, j + k]))
        out[f"{nm}_sd"] = rel(cust[:, j + 1], mc[:, j + 1], np.sqrt((x * x).mean(axis=0)))
    out["survival_1yr"] = rel(cust[:, 12], mc[:, 12], np.abs(mc[:, 12]))
    for q, x, nm in ((0, r, "equity"), (1, v, "value_total")):
        out[nm] = rel(draws[:, q], md[:, q], np.abs(x).sum(axis=1))
    return out, mc, md


def elasticities(level2, mu_share, n_cov: int, D: int):
    """{(k, component): per-draw array} for covariates k = 1..n_cov of level-2 rows [beta[:, 0] (K),
    beta[:, 1] (K), (beta[:, 2] (K)), ...]."""
    K = n_cov + 1
    out = {}
    for k in range(1, K):
        rate = level2[:, k]
        life = -level2[:, K + k] * mu_share
        spend = level2[:, 2 * K + k] if D == 3 else np.zeros_like(rate)
        out[k, "purchase_rate"], out[k, "lifetime"], out[k, "spend"] = rate, life, spend
        out[k, "total"] = rate + life + spend
    return out

"""Float64 model of the summary sink — TEST INFRASTRUCTURE ONLY, plain numpy.

The summary sinks (``draw_sink="summary"`` / ``"summary+pct"``) keep, per chain and customer, eleven
running sums over the stored sweeps (``CLV_SUM_*``, ``_lib.SUM_STATS``) where the full sink keeps the
draws themselves.  The sink does not change the chain, so a summary run and a full run of the same
problem and seed are one trajectory, and every sum is a function of the full run's stored draws:

* eight of them exactly — ``lambda``, ``mu``, ``z``, ``lambda2 = lam * lam``, ``mu2 = mu * mu``,
  ``eta``, ``mu_capped = min(mu, cap)``, ``tau``: the library is built with ``-ffp-contract=off`` and
  each sum is a plain ``sum + value`` from zero in stored order, which numpy reproduces bit for bit
  (:func:`sums_from_draws`; sequential, never ``np.sum``, which is pairwise);
* three of them — ``log_lambda``, ``log_mu``, ``log_eta`` — to a derived bound
  (:func:`log_sum_bound`): the device sums the log-scale state itself, the stored draw is
  ``exp_fast`` of it.

:func:`rhat_from_draws` is the non-split R-hat of ``analysis.summary_rhat``'s docstring computed from
the draws with two-pass variances, and :func:`rhat_tolerance` what the ``E[x^2] - E[x]^2`` form of
the summary route may lose against it.  :func:`check_sums` is the comparison the GPU tests run
(tests/test_gpu_summary_sink.py); its ``wrong=`` models are the power checks' mutations.
"""
from __future__ import annotations

import numpy as np

SUM_STATS = ("lambda", "mu", "z", "log_lambda", "log_mu", "lambda2", "mu2", "eta", "log_eta", "mu_capped", "tau")
EXACT_STATS = ("lambda", "mu", "z", "lambda2", "mu2", "eta", "mu_capped", "tau")
LOG_STATS = ("log_lambda", "log_mu", "log_eta")
LOG_COLUMN = {"log_lambda": 0, "log_mu": 1, "log_eta": 4}   # the level-1 column a log sum belongs to
MU_CAP = 0.05          # CLV_SUMMARY_MU_CAP
U = 2.0 ** -53         # unit roundoff of float64
EXP_FAST_ULP = 2.0     # exp_fast against the correctly rounded exp (fastmath.h; test_device_fast_exp_accuracy)

# The power checks' wrong models (check_sums / sums_from_draws ``wrong=``), one thing wrong at a time.
# "cap_0.5" is not among them: it is mu_cap=0.5.
WRONG = ("mu2_from_lam_mu", "lambda2_from_lam", "logs_exchanged", "capped_tau_exchanged", "d2_shifted_by_two",
         "one_draw_fewer")


def seq_sum(v):
    """Sum over axis 0 in order, from zero: ((0 + v[0]) + v[1]) + ... — np.cumsum's last row."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape[0] == 0:
        return np.zeros(v.shape[1:])
    return np.cumsum(v, axis=0)[-1]


def sums_from_draws(l1, mu_cap=MU_CAP, wrong=None):
    """[11][N] sums, in the order of SUM_STATS, of one chain's stored draws ``l1`` [n_draws][N][D + 2]
    (columns lambda, mu, tau, z, (eta)) taken in stored order.  The eta and log_eta planes are zero
    for D = 2, as on the device (its buffer is zeroed at create and those planes are never written).
    The three log planes are the sums of np.log of the stored draw: see log_sum_bound.
    ``wrong`` (power checks only): one of WRONG."""
    l1 = np.asarray(l1, dtype=np.float64)
    assert l1.ndim == 3 and l1.shape[2] in (4, 5), l1.shape
    assert wrong is None or wrong in WRONG, wrong
    if wrong == "one_draw_fewer":
        l1 = l1[:-1]
    D = l1.shape[2] - 2
    lam, mu, tau, z = l1[..., 0], l1[..., 1], l1[..., 2], l1[..., 3]
    cols = {"lambda": lam, "mu": mu, "z": z, "log_lambda": np.log(lam), "log_mu": np.log(mu),
            "lambda2": lam if wrong == "lambda2_from_lam" else lam * lam,
            "mu2": lam * mu if wrong == "mu2_from_lam_mu" else mu * mu,
            "mu_capped": np.minimum(mu, mu_cap), "tau": tau}
    if D == 3:
        cols.update(eta=l1[..., 4], log_eta=np.log(l1[..., 4]))
    if wrong == "logs_exchanged":
        cols["log_lambda"], cols["log_mu"] = cols["log_mu"], cols["log_lambda"]
    if wrong == "capped_tau_exchanged":
        cols["mu_capped"], cols["tau"] = cols["tau"], cols["mu_capped"]
    out = np.zeros((len(SUM_STATS), l1.shape[1]))
    for k, name in enumerate(SUM_STATS):
        if name in cols:
            out[k] = seq_sum(cols[name])
    if wrong == "d2_shifted_by_two" and D == 2:
        # the bivariate kernel's nine sums kept densely: what follows mu2 lands two planes early
        i = SUM_STATS.index("eta")
        out[i], out[i + 1] = out[i + 2].copy(), out[i + 3].copy()
        out[i + 2:] = 0.0
    return out


def log_sum_bound(l1_column):
    """Absolute bound, per customer, of |device log sum - sum of np.log(stored draw)| for one
    level-1 column ``l1_column`` [n_draws][N] (lambda, mu or eta) in stored order.

    The device adds the log-scale state s_i of each stored sweep (``cust_store``: lgl = ll, lgm = lm,
    leta = xe); the draw it stores is d_i = exp_fast(s_i).  The model adds t_i = np.log(d_i).

    1. exp_fast is within EXP_FAST_ULP = 2 ulp of the correctly rounded exp (fastmath.h;
       test_device_fast_exp_accuracy holds it to that), which is within 1/2 ulp of exp: 2.5 ulp.  An
       ulp of v is at most 2^-52 v, so d_i = exp(s_i) (1 + e_i) with |e_i| <= 2.5 * 2^-52 = 5 U, and
       log d_i = s_i + log(1 + e_i): |s_i - log d_i| <= 5 U (1 + 5 U), absolute, however small s_i.
       (eta beyond |log eta| = 700 is libm's exp, <= 1 ulp: inside the same figure.)
    2. np.log is within 1 ulp of log: |t_i - log d_i| <= 2^-52 |log d_i| = 2 U |log d_i|, and
       |log d_i| <= |t_i| (1 + 2 U).
    3. A sequential sum from zero rounds once per addition, the first (0 + x) exactly: addition k
       (k = 2..n) errs by at most U times its result, which is at most the running sum of |terms|,
       A_k = |x_1| + ... + |x_k|, to first order.  Two such sums: the device's over s_i, the model's
       over t_i; |s_i| <= |t_i| + 7 U (1 + |t_i|) by 1 and 2, so both are bounded with A_k of |t_i|.

    Together, to first order in U,

        bound = U * [ sum_i (5 + 2 |t_i|)  +  2 * sum_{k=2..n} A_k ],

    multiplied by (1 + 2^-20) for every second-order term left out (each is below 64 n U times a
    first-order one, and n <= 2^20 stored draws by far).  One stored draw: U (5 + 2 |t_1|), no
    summation term.  Nothing in it is fitted to a measurement; the GPU tests print measured / bound."""
    t = np.abs(np.log(np.asarray(l1_column, dtype=np.float64)))
    assert t.ndim == 2
    if t.shape[0] == 0:
        return np.zeros(t.shape[1])
    run = np.cumsum(t, axis=0)                       # A_k
    per_draw = seq_sum((EXP_FAST_ULP + 0.5) * 2.0 + 2.0 * t)  # parts 1 and 2
    rounding = 2.0 * (run[1:].sum(axis=0) if t.shape[0] > 1 else 0.0)  # part 3, both sums
    return (1.0 + 2.0 ** -20) * U * (per_draw + rounding)


def check_sums(got, l1, mu_cap=MU_CAP, wrong=None):
    """One chain's device sums ``got`` [11][N] against the model of its stored draws ``l1``
    [n_draws][N][D + 2].  Returns (bad, ratio): ``bad`` {stat: bool [N]}, the customers whose sum is
    off — the eight exact stats by their bits, the log stats beyond log_sum_bound (the eta planes of a
    bivariate run are exact zeros and compared as such); ``ratio`` {log stat: measured / bound [N]}."""
    got = np.asarray(got, dtype=np.float64)
    l1 = np.asarray(l1, dtype=np.float64)
    D = l1.shape[2] - 2
    assert got.shape == (len(SUM_STATS), l1.shape[1]), (got.shape, l1.shape)
    ref = sums_from_draws(l1, mu_cap, wrong)
    bad, ratio = {}, {}
    for k, name in enumerate(SUM_STATS):
        if name in LOG_STATS and (D == 3 or name != "log_eta"):
            bound = log_sum_bound(l1[..., LOG_COLUMN[name]])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio[name] = np.abs(got[k] - ref[k]) / bound
            bad[name] = ~(np.abs(got[k] - ref[k]) <= bound)   # NaN is bad
        else:
            bad[name] = got[k].view(np.uint64) != ref[k].view(np.uint64)
    return bad, ratio


def any_bad(bad):
    """Customers that fail any stat of check_sums' ``bad``."""
    return np.logical_or.reduce([bad[s] for s in SUM_STATS])


# ---------------------------------------------------------------------------------------------
# the non-split R-hat of analysis.summary_rhat, from the draws
# ---------------------------------------------------------------------------------------------
RHAT_COLUMNS = {"rhat_lambda": 0, "rhat_mu": 1}


def _rhat_parts(l1_chains, col):
    x = np.stack([np.asarray(c, dtype=np.float64)[..., col] for c in l1_chains])   # [C][n][N]
    n = x.shape[1]
    s2 = x.var(axis=1, ddof=1)              # two-pass: no cancellation
    m1 = x.mean(axis=1)
    W = s2.mean(axis=0)
    B_n = m1.var(axis=0, ddof=1)
    return x, n, s2, m1, W, B_n


def rhat_from_draws(l1_chains):
    """{"rhat_lambda", "rhat_mu"}: [N] each.  ``l1_chains``: the chains' stored draws, [C] of
    [n][N][D + 2].  s_c^2 = var(x_c, ddof=1) per chain, W = mean_c s_c^2, B / n = var_c(mean x_c,
    ddof=1), R-hat = sqrt(((n - 1) / n W + B / n) / W); NaN where a chain's variance is not positive."""
    out = {}
    for name, col in RHAT_COLUMNS.items():
        _, n, s2, _, W, B_n = _rhat_parts(l1_chains, col)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.sqrt(((n - 1.0) / n * W + B_n) / W)
        out[name] = np.where((s2 > 0).all(axis=0), r, np.nan)
    return out


def rhat_tolerance(l1_chains):
    """{"rhat_lambda", "rhat_mu"}: [N] absolute tolerances of summary_rhat (from the running means
    m1 = S1 / n, m2 = S2 / n of sums_from_draws) against rhat_from_draws, first order in U = 2^-53.

    The chain's variance by the summary route is s^2 = (m2 - m1^2) n / (n - 1).  S1 is a sequential sum
    of n positive terms: relative error <= (n - 1) U; S2 the same of terms rounded once: <= n U.  The
    divisions by n and the square add U each, so m2 carries <= (n + 1) U and m1^2 <= (2 n + 1) U,
    relatively, and the subtraction U of its result.  With m1^2 <= m2 and |m2 - m1^2| <= m2:

        |d s^2| <= (3 n + 4) U m2 n / (n - 1)        (summary_rhat's docstring: "about 2^-52 E[x^2]")

    plus the two-pass variance's own (n + 3) U s^2 on the other side.  d W <= mean_c |d s_c^2|.
    B / n = var_c(m1_c): each m1_c carries <= (n + 1) U relatively on either route, so
    |d (B / n)| <= 2 sum_c |m1_c - mean m1| * 2 (n + 1) U max_c m1_c / (C - 1), plus (C + 3) U B / n.
    R^2 = (n - 1) / n + (B / n) / W, so

        |d R| <= [ |d (B / n)| / W + (B / n) |d W| / W^2 ] / (2 R) + 4 U R     (the division, the sum, the sqrt).

    Infinite where a chain's variance is within its own |d s^2| of zero: the cancellation may then
    leave nothing (or a non-positive number: NaN) and first order says nothing."""
    out = {}
    for name, col in RHAT_COLUMNS.items():
        x, n, s2, m1, W, B_n = _rhat_parts(l1_chains, col)
        C = x.shape[0]
        m2 = (x * x).mean(axis=1)
        ds2 = (3 * n + 4) * U * m2 * n / (n - 1.0) + (n + 3) * U * s2
        dW = ds2.mean(axis=0)
        dB = (2.0 * np.abs(m1 - m1.mean(axis=0)).sum(axis=0) * 2.0 * (n + 1) * U * m1.max(axis=0) / (C - 1.0)
              + (C + 3) * U * B_n)
        with np.errstate(divide="ignore", invalid="ignore"):
            R = np.sqrt((n - 1.0) / n + B_n / W)
            tol = (dB / W + B_n * dW / (W * W)) / (2.0 * R) + 4.0 * U * R
        lost = (s2 <= 2.0 * ds2).any(axis=0)
        out[name] = np.where(lost | ~np.isfinite(tol), np.inf, tol)
    return out


# ---------------------------------------------------------------------------------------------
# the GPU module's cases (tests/test_gpu_summary_sink.py) and the model's draws at their shapes
# ---------------------------------------------------------------------------------------------
def make_case(D, K, n, chains, chain_first, mode, seed, S=20, burnin=4, mcmc=13, thin=3, sink="summary"):
    return dict(D=D, K=K, n=n, chains=chains, chain_first=chain_first, mode=mode, seed=seed, S=S, burnin=burnin,
                mcmc=mcmc, thin=thin, sink=sink, covs=[f"c{k}" for k in range(1, K)])


# mode: "fused" = one launch per sweep (CLV_PERSISTENT=0: prefetch_sums / SumsPre), "block" / "split" /
# "relay" = the persistent kernel's layouts.  N = 257 / 513: a full block plus one lane, two plus one;
# 640: the split layout's two workgroups.  17 sweeps, 5 stored (5, 8, 11, 14, 17); split and relay 13, 4 stored.
CASES = {
    "fused_bi1": make_case(2, 1, 513, 2, 0, "fused", 8101),
    "fused_bi9": make_case(2, 9, 257, 3, 2, "fused", 8102),        # the D = 2 slot remap, covariates in LDS
    "fused_tri1": make_case(3, 1, 513, 2, 0, "fused", 8103),
    "fused_tri3": make_case(3, 3, 257, 2, 0, "fused", 8104),
    "block_bi2": make_case(2, 2, 513, 2, 0, "block", 8105),
    "block_tri3": make_case(3, 3, 257, 2, 0, "block", 8106),
    "split_bi2": make_case(2, 2, 640, 2, 0, "split", 8107, burnin=3, mcmc=10),
    "relay_bi2": make_case(2, 2, 640, 2, 0, "relay", 8108, burnin=3, mcmc=10),
    "fused_pct_bi2": make_case(2, 2, 257, 3, 0, "fused", 8109, sink="summary+pct"),
    "fused_pct_tri1": make_case(3, 1, 257, 2, 0, "fused", 8110, sink="summary+pct"),
}
POWER_CASES = ("fused_tri3", "fused_bi9")     # compared again with one thing wrong in the model at a time
CONSUMER_CASE = "fused_bi9"                   # three chains: summary_rhat and the envelope's means


def case_frame(case):
    from tests.helpers import cdnow_tiled, with_covariates
    df = cdnow_tiled(case["n"])
    return with_covariates(df, case["K"] - 1) if case["K"] > 1 else df


def stored_sweeps(burnin, mcmc, thin, upto=None):
    """The sweeps (1-based) whose draw is stored (bi:402), up to sweep ``upto``."""
    last = burnin + mcmc if upto is None else min(upto, burnin + mcmc)
    return [s for s in range(burnin + 1, last + 1) if (s - burnin - 1) % thin == 0]


def model_draws(case, chain):
    """The float64 model's free run of ``case`` (philox_sweep_ref.model_chain), chain ``chain``: its
    stored draws [n_draws][N][D + 2] in the level-1 layout and the log-scale states they are exp of,
    {"log_lambda", "log_mu", ("log_eta")}: [n_draws][N]."""
    from tests import philox_sweep_ref as P
    mp = P.ModelProblem(case_frame(case), case["covs"], case["D"])
    keep = set(stored_sweeps(case["burnin"], case["mcmc"], case["thin"]))
    rows, states = [], dict(log_lambda=[], log_mu=[], log_eta=[])
    for s, r, _ in P.model_chain(mp, case["seed"], chain, case["burnin"] + case["mcmc"], case["S"]):
        if s in keep:
            cols = [r["lam"], r["mu"], r["tau"], r["z"].astype(np.float64)] + ([r["eta"]] if case["D"] == 3 else [])
            rows.append(np.column_stack(cols))
            states["log_lambda"].append(r["ll"])
            states["log_mu"].append(r["lm"])
            if case["D"] == 3:
                states["log_eta"].append(r["leta"])
    return np.stack(rows), {k: np.stack(v) for k, v in states.items() if v}

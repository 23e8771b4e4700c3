"""Drop-in for ``src/models/bivariate/mcmc.py`` (Abe 2009 HB Pareto/NBD, lambda & mu).

``mcmc_draw_parameters`` keeps the reference's signature, defaults, validation errors, trace
line and return layout (bivariate/mcmc.py:437-504); the sweeps run on the GPU
(csrc/kernels.hip).  Keyword-only extras:

* ``draw_sink``: "full" (level_1 draws, reference layout), "summary" (per-customer posterior
  means kept on device; ``level_1`` is None), "summary+pct" (as "summary", plus Table 4's
  per-customer 2.5/97.5 percentiles of lambda and mu from a float32 store of the draws:
  ``out["summary"]["level1"]``, which ``analysis.compute_table4(out)`` uses), "none".
* ``rng``: "philox" (counter-based, default) or "replay" (test mode: consume variates recorded
  from the reference's numpy Generator, ``replay_tape``).
* ``device``: HIP device ordinal (-1 = current).
* ``devices``: several device ordinals — the run is spread over them from this process
  (``shard="chains"``: chain groups, one host thread each; ``"customers"``: every chain's customers
  split into shards exchanging the level-2 statistics each sweep by peer stores or device copies,
  ``exchange`` = "auto" | "p2p" | "copy"; ``"auto"``: chains when they divide evenly), with the
  single-device run's output bit for bit (sampler.fit_multi, csrc/group.hip).
* ``diagnostics``: True adds ``out["diagnostics"] = {"level_1": DataFrame per customer, "level_2":
  DataFrame per level-2 parameter}`` — split R-hat, ESS, MCSE and truncation lag computed on the GPU
  from the draws still in HBM (``analysis.level1_diagnostics`` / ``level2_diagnostics``;
  ``draw_sink="full"`` only, at least 8 stored draws).  False changes nothing.  ``"rank"`` gives
  the same and adds ``"level_1_rank"``, ``"level_2_rank"`` (rank-normalised R-hat, bulk and tail ESS,
  MCSE of the sd, HDI, median: ``analysis.level1_rank_diagnostics`` / ``level2_rank_diagnostics``)
  and ``"level_2_summary"``, the nine columns of ``az.summary`` (``analysis.level2_summary``).
* ``lifetime_value``: True, or a dict of ``analysis.lifetime_value``'s keywords (``discount_rate``,
  ``periods_per_year``, ``horizon``, ``monetary``, ``omega2``), adds ``out["lifetime_value"]``: the
  posterior customer lifetime value per customer and the customer equity per draw, computed on the
  GPU from the draws still in HBM (``csrc/ltv.hip``; ``draw_sink="full"`` only).  None changes nothing.
* ``information_criteria``: True, or a dict of ``analysis.information_criteria``'s keywords (``spend``,
  ``omega2``, ``reff``), adds ``out["information_criteria"]``: WAIC and PSIS-LOO per customer and in
  total, from the draws still in HBM (``csrc/ic.hip``; ``draw_sink="full"`` only); compare two fits
  with ``analysis.compare_models``.  None changes nothing.
* ``forecast``: True, or a dict of ``analysis.forecast``'s keywords (``T_star``, ``x_star`` — an array or
  the name of a column of ``cal_cbs`` —, ``k_max``, ``pmf``), adds ``out["forecast"]``: the closed-form
  predictive distribution of every customer's holdout purchases and, with ``x_star``, its scores, from
  the draws still in HBM (``csrc/forecast.hip``; ``draw_sink="full"`` only).  None changes nothing.
* ``ppc``: True, or a dict of ``analysis.posterior_predictive_check``'s keywords (``level``, ``k_hist``,
  ``seed``, ``replicates``), adds ``out["ppc"]``: the calibration data replicated per draw at the customer
  or at the population level, with the frequency histogram, posterior predictive p-values and
  per-customer PIT columns, from the draws still in HBM (``csrc/ppc.hip``; ``draw_sink="full"`` only).
  None changes nothing.
* ``marginal_information_criteria``: True, or a dict of ``analysis.marginal_information_criteria``'s
  keywords (``spend``, ``omega2``, ``reff``, ``nodes``), adds ``out["marginal_information_criteria"]``: WAIC
  and PSIS-LOO from the likelihood marginal over each customer's own (lambda, mu), from the level-2
  records still in HBM (``csrc/marginal.hip``; ``draw_sink="full"`` only).  None changes nothing.
"""
from __future__ import annotations

from typing import Optional, Sequence

from .analysis import draw_future_transactions  # bi:506-546 (posterior predictive, csrc/analysis.hip)
from .sampler import build_problem, fit, forecast_kwargs

__all__ = ["mcmc_draw_parameters", "draw_future_transactions"]


def mcmc_draw_parameters(cal_cbs, covariates: Optional[Sequence[str]] = None, mcmc: int = 2500,
                         burnin: int = 500, thin: int = 50, chains: int = 2, seed: Optional[int] = None,
                         trace: int = 100, n_mh_steps: int = 20, *, draw_sink: str = "full",
                         rng: str = "philox", device: int = -1, replay_tape=None,
                         replay_sweeps: Optional[int] = None, devices: Optional[Sequence[int]] = None,
                         shard: str = "auto", exchange: str = "auto", diagnostics=False, lifetime_value=None,
                         information_criteria=None, forecast=None, ppc=None, marginal_information_criteria=None):
    """Run the Abe (2009) Gibbs/MH sampler on calibration CBS (bivariate/mcmc.py:437).

    Returns dict(level_1=[(n_draws, N, 4) per chain: lambda, mu, tau, z],
                 level_2=[(n_draws, 2K+3) per chain: beta.T.ravel(), Sigma00, Sigma01, Sigma11],
                 log_likelihood=np.float64)
    """
    if covariates is None:
        covariates = []
    for col in ("x", "t_x", "T_cal"):  # bi:461-465
        if col not in cal_cbs:
            raise ValueError(f"cal_cbs missing required column '{col}'")
    if not all(col in cal_cbs for col in covariates):
        raise ValueError("some covariate columns not in cal_cbs")
    p = build_problem(cal_cbs, covariates, D=2)
    return fit(p, mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=seed, trace=trace,
               n_mh_steps=n_mh_steps, draw_sink=draw_sink, rng=rng, device=device,
               replay_tape=replay_tape, replay_sweeps=replay_sweeps, devices=devices, shard=shard,
               exchange=exchange, diagnostics=diagnostics, lifetime_value=lifetime_value,
               information_criteria=information_criteria,
               forecast=forecast_kwargs(forecast, draw_sink, cal_cbs), ppc=ppc,
               marginal_information_criteria=marginal_information_criteria)

"""MI355X-native Gibbs/MH sampler for the Abe (2009/2015) hierarchical Pareto/NBD model.

Drop-in for lucagem29/mcmc_clv_model's sampler entry points:

    from mcmc_clv_model_amd import mcmc_draw_parameters        # src/models/bivariate/mcmc.py:437
    from mcmc_clv_model_amd import mcmc_draw_parameters_rfm_m  # src/models/trivariate/mcmc.py:580

Posterior analysis: draw_future_transactions (bi:506 / tri:660), the Table 4 helpers
of utils/analysis_bi_helpers.py and the weekly tracking curve, also on the GPU (analysis.py), and
the convergence diagnostics the reference asks of ArviZ (analysis_abe.py:651-706): split R-hat, ESS,
MCSE and autocorrelation for the level-2 draws and for every customer (level1_diagnostics), and
az.summary's table with its rank-normalised ess_bulk, ess_tail and r_hat (level2_summary,
level1_rank_diagnostics, level2_rank_diagnostics).  The classical Pareto/NBD fitted by maximum
likelihood, the baseline both HB models are measured against (analysis_abe.py:205-217, :426-438), is
mle.ParetoNBDFitter, a drop-in for what the reference uses of lifetimes', with pnbd_weekly_tracking
and mape_aggregate (analysis_bi_helpers.py:29).  What Abe (2015) derives from the draws, which the
reference stops short of: every customer's posterior lifetime value, the customer equity and the
elasticity of CLV to the covariates (lifetime_value, customer_equity, lifetime_value_elasticities).
Which model the data prefer: the pointwise log-likelihood, WAIC and PSIS-LOO with the Pareto k
diagnostic per customer, and a paired comparison with a standard error (pointwise_log_likelihood,
information_criteria, psis_loo, compare_models) — az.waic / az.loo / az.compare, which the reference
prepares for and never calls.
Customers who were not in the fit — the usual case: fit on a sample, score the whole base — get their
own level-1 draws from the fit's level-2 draws (score_customers: the level-1 half of the sweep run
against the stored (beta, Sigma) records, in the drop-ins' level_1 layout, so every function above
works on them unchanged; sink="summary" keeps only per-customer sums, for millions of customers).
(beta, Sigma) is held fixed while a record's inner sweeps run: when the records differ, a customer
enters each record distributed for the one before, a bias that shrinks as inner_sweeps grows.
The holdout forecast in closed form: every customer's posterior predictive distribution of the
number of holdout purchases, marginal over z and tau, with its mean, P(alive), quantiles, log score,
PIT and ranked probability score (forecast, forecast_pit, compare_forecasts, forecast_table).
Posterior predictive checks of the calibration data, replicated per draw at the customer or at the
population level: frequency histogram, p-values, per-customer PITs (posterior_predictive_check, ppc_pit).
The marginal likelihood of a customer under each level-2 record — its own (lambda, mu) integrated out
by adaptive Gauss-Hermite quadrature — and WAIC / PSIS-LOO and out-of-sample log scores from it
(marginal_log_likelihood, marginal_information_criteria, marginal_log_score).
Many small fits at once — the training sets of a cross-validation, fits per cohort, bootstrap or
simulation studies — run in one kernel launch with the single calls' bits (mcmc_draw_parameters_many,
mcmc_draw_parameters_rfm_m_many), and exact K-fold cross-validation on top of them
(kfold_cross_validation).
The classical baseline completed: the Pareto/NBD with time-invariant covariates of
Fader & Hardie (2007) (ParetoNBDFitter.fit(covariates=...), the fair opponent of a covariate HB
model), standard errors, a Wald summary and likelihood-ratio tests of a fit (standard_errors=True,
likelihood_ratio_test), the Gamma-Gamma spend model (GammaGammaFitter), DERT and the classical CLV
that stands beside lifetime_value (ParetoNBDFitter.discounted_expected_transactions,
classical_lifetime_value).
The log-normal Pareto/NBD fitted by maximum marginal likelihood: the HB models'
heterogeneity with the classical estimation principle (LogNormalParetoNBDFitter), its score from the
posterior moments of the marginal-likelihood quadrature by Fisher's identity.

The per-sweep work runs in hand-written HIP kernels for gfx950 (csrc/), bound through the C
ABI in include/clvmcmc.h.  There is no CPU fallback.
"""
from .analysis import (chain_total_loglik, compare_forecasts, compare_models, compute_table4, customer_equity,
                       draw_future_transactions, draw_future_transactions_rfm_m, extract_correlation,
                       forecast, forecast_pit, forecast_table, information_criteria, level1_diagnostics,
                       level1_rank_diagnostics, level2_autocorr, level2_diagnostics, level2_rank_diagnostics,
                       level2_summary, lifetime_value, lifetime_value_elasticities, pointwise_log_likelihood,
                       post_mean_lambdas, post_mean_mus, posterior_predictive_check, posterior_weekly_tracking, ppc_pit,
                       psis_loo, score_customers,
                       summarize_level2, summary_rhat,
                       marginal_information_criteria, marginal_log_likelihood, marginal_log_score)
from .batch import kfold_cross_validation, mcmc_draw_parameters_many, mcmc_draw_parameters_rfm_m_many
from .bivariate import mcmc_draw_parameters
from .mle import (GammaGammaFitter, LogNormalParetoNBDFitter, ParetoNBDFitter, classical_lifetime_value,
                  likelihood_ratio_test, mape_aggregate, pnbd_weekly_tracking)
from .trivariate import mcmc_draw_parameters_rfm_m

__all__ = ["mcmc_draw_parameters", "mcmc_draw_parameters_rfm_m", "draw_future_transactions",
           "draw_future_transactions_rfm_m", "post_mean_lambdas", "post_mean_mus", "chain_total_loglik",
           "compute_table4", "posterior_weekly_tracking", "level1_diagnostics", "level2_diagnostics",
           "level2_autocorr", "summarize_level2", "extract_correlation", "summary_rhat",
           "level1_rank_diagnostics", "level2_rank_diagnostics", "level2_summary", "ParetoNBDFitter",
           "pnbd_weekly_tracking", "mape_aggregate", "lifetime_value", "customer_equity",
           "lifetime_value_elasticities", "pointwise_log_likelihood", "information_criteria", "psis_loo",
           "compare_models", "score_customers", "forecast", "forecast_pit", "compare_forecasts",
           "forecast_table", "posterior_predictive_check", "ppc_pit", "marginal_log_likelihood",
           "marginal_information_criteria", "marginal_log_score", "mcmc_draw_parameters_many",
           "mcmc_draw_parameters_rfm_m_many", "kfold_cross_validation", "GammaGammaFitter",
           "classical_lifetime_value", "likelihood_ratio_test", "LogNormalParetoNBDFitter"]
__version__ = "0.1.0"

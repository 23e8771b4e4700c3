"""ctypes binding of libclvmcmc.so (C ABI declared in include/clvmcmc.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is visible,
every sampler call raises.  torch (when importable) is imported before the library so that
``libamdhip64.so.7`` resolves to the HIP runtime torch already loaded — one runtime per
process, so device pointers and streams can be shared with torch.distributed (RCCL).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_uint8, POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

try:  # share torch's HIP runtime when torch is present (see module docstring)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the single-GPU path
    torch = None

LIB_NAME = "libclvmcmc.so"
LIB_PATH = os.environ.get("CLV_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

ABI_VERSION = 2
BLOCK = 256
MAX_K = 9
MAX_D = 3
RNG_PHILOX, RNG_REPLAY = 0, 1
SINK_FULL, SINK_SUMMARY, SINK_NONE, SINK_SUMMARY_PCT = 0, 1, 2, 3
EXCHANGE_AUTO, EXCHANGE_P2P, EXCHANGE_COPY = 0, 1, 2
SUM_STATS = ("lambda", "mu", "z", "log_lambda", "log_mu", "lambda2", "mu2", "eta", "log_eta", "mu_capped", "tau")
SUMMARY_MU_CAP = 0.05  # CLV_SUMMARY_MU_CAP: the "mu_capped" sum is of min(mu, 0.05) (analysis_bi_helpers.py:89)
N_SUM_STATS = len(SUM_STATS)
TAPE_HYPER = 40


class ClvConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", c_int32), ("D", c_int32), ("K", c_int32), ("n_mh_steps", c_int32),
        ("burnin", c_int32), ("mcmc", c_int32), ("thin", c_int32), ("n_chains", c_int32),
        ("chain_first", c_int32), ("rng_mode", c_int32), ("draw_sink", c_int32), ("device", c_int32),
        ("seed", c_uint64), ("n_global", c_int64), ("shard_begin", c_int64),
        ("world_size", c_int32), ("rank", c_int32), ("blocks_per_rank", c_int32),
        ("blocks_per_unit", c_int32), ("stream", c_uint64),
    ]


class ClvData(ctypes.Structure):
    _fields_ = [
        ("n", c_int64), ("x", c_void_p), ("t_x", c_void_p), ("T_cal", c_void_p),
        ("covariates", c_void_p), ("log_s", c_void_p),
    ]


class ClvPrior(ctypes.Structure):
    _fields_ = [
        ("lam_init", c_double), ("V", c_double * 81), ("chol_V", c_double * 81), ("A0B0", c_double * 27),
        ("S0_B0A0B0", c_double * 9), ("nu_n", c_double), ("beta_init", c_double * 27),
        ("sigma_init", c_double * 9), ("omega2", c_double),
    ]


class ClvBatchItem(ctypes.Structure):
    """clv_batch_item: one fit of clv_batch_fit (host pointers; outputs it does not want are None)."""
    _fields_ = [
        ("n", c_int64), ("seed", c_uint64), ("x", c_void_p), ("t_x", c_void_p), ("T_cal", c_void_p),
        ("covariates", c_void_p), ("log_s", c_void_p), ("prior", POINTER(ClvPrior)),
        ("level1", c_void_p), ("level2", c_void_p), ("loglik", c_void_p), ("sums", c_void_p),
        ("state_lam", c_void_p), ("state_mu", c_void_p),
    ]


_lib = None


class ClvError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libclvmcmc.so (once) and declare every entry point of include/clvmcmc.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ClvError(
            f"{LIB_NAME} is not built ({LIB_PATH}); run `make -C mcmc_clv_model_amd/csrc` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    sp = c_void_p
    dp = POINTER(c_double)
    sigs = {
        "clv_abi_version": (c_int32, []),
        "clv_default_blocks_per_unit": (c_int32, [c_int64]),
        "clv_sizeof": (c_int64, [c_int32]),
        "clv_last_error": (c_char_p, []),
        "clv_device_count": (c_int32, [POINTER(c_int32)]),
        "clv_create": (c_int32, [POINTER(ClvConfig), POINTER(ClvData), POINTER(ClvPrior), POINTER(sp)]),
        "clv_destroy": (None, [sp]),
        "clv_set_replay_tape": (c_int32, [sp, dp, c_int64]),
        "clv_replay_sweep_stride": (c_int64, [sp]),
        "clv_run": (c_int32, [sp, c_int64]),
        "clv_rollback": (c_int32, [sp]),
        "clv_sweep": (c_int32, [sp]),
        "clv_hyper": (c_int32, [sp, c_void_p]),
        "clv_partials": (c_int32, [sp, POINTER(c_void_p), POINTER(c_int64), POINTER(c_int32)]),
        "clv_copy_partials": (c_int32, [sp, c_void_p]),
        "clv_synchronize": (c_int32, [sp]),
        "clv_sweeps_done": (c_int64, [sp]),
        "clv_clock_ghz": (c_int32, [sp, POINTER(c_double)]),
        "clv_clock_probe": (c_int32, [sp, c_double, POINTER(c_double)]),
        "clv_launch_info": (c_int32, [sp, POINTER(c_int64)]),
        "clv_split_relay_steps": (c_int32, [sp, POINTER(c_int32)]),
        "clv_p2p_info": (c_int32, [sp, POINTER(c_int64)]),
        "clv_p2p_export": (c_int32, [sp, c_void_p]),
        "clv_p2p_connect": (c_int32, [sp, c_void_p, POINTER(c_uint64)]),
        "clv_p2p_disconnect": (c_int32, [sp]),
        "clv_p2p_set_persistent": (c_int32, [sp, c_int32]),
        "clv_set_wait_timeout": (c_int32, [sp, c_double]),
        "clv_set_stream": (c_int32, [sp, c_uint64]),
        "clv_note_sweeps": (c_int32, [sp, c_int64]),
        "clv_read_draws": (c_int32, [sp, dp, dp, dp]),
        "clv_stream_draws": (c_int32, [sp, dp]),
        "clv_read_summary": (c_int32, [sp, dp, POINTER(c_int64)]),
        "clv_get_state": (c_int32, [sp, dp, dp, dp]),
        "clv_set_state": (c_int32, [sp, dp, dp, dp, c_int64]),
        "clv_set_timing": (c_int32, [sp, c_int32]),
        "clv_kernel_time": (c_int32, [sp, dp, POINTER(c_int64), dp, POINTER(c_int64)]),
        "clv_debug_philox": (c_int32, [c_uint32, c_uint32, POINTER(c_uint32), c_int64, POINTER(c_uint32)]),
        "clv_debug_variates": (c_int32, [c_uint64, c_int32, c_uint32, c_int64, c_int32, POINTER(c_float),
                                         POINTER(c_float), POINTER(c_float), dp, dp, dp, dp, POINTER(c_float)]),
        "clv_debug_log2u_scan": (c_int32, [c_uint64, c_uint64, dp]),
        "clv_debug_host_times": (c_int32, [sp, POINTER(c_int64)]),
        "clv_debug_t3": (c_int32, [POINTER(c_uint32), c_int64, c_int32, POINTER(c_float), POINTER(c_float)]),
        "clv_debug_level2": (c_int32, [c_int32, c_int32, POINTER(ClvPrior), dp, dp, dp, dp, dp, dp, dp]),
        "clv_debug_hyper_variates": (c_int32, [c_uint64, c_int32, c_uint32, c_double, c_int64, dp, dp]),
        "clv_debug_stamps": (c_int32, [sp, POINTER(c_uint64)]),
        "clv_debug_wg_stamps": (c_int32, [sp, POINTER(c_uint64)]),
        "clv_debug_split_stamps": (c_int32, [sp, POINTER(c_uint64)]),
        "clv_debug_split_relay_plan": (c_int32, [c_int32, c_int32, POINTER(c_int32)]),
        "clv_debug_split_draw_plan": (c_int32, [c_int32, c_int32, POINTER(c_int32)]),
        "clv_debug_exp": (c_int32, [dp, c_int64, dp]),
        "clv_debug_log": (c_int32, [dp, c_int64, dp]),
        "clv_debug_mh_step": (c_int32, [c_int64, POINTER(c_int32), POINTER(c_uint8), dp, dp, dp, dp, dp,
                                        POINTER(c_float), dp, POINTER(c_float), dp]),
        "clv_debug_wg_map": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_int32)]),
        "clv_debug_sweep_plan": (c_int32, [POINTER(c_int64), POINTER(c_int32)]),
        "clv_debug_world_has_empty_shard": (c_int32, [c_int64, c_int32, c_int32]),
        "clv_debug_persist_choice": (c_int32, [c_int32, c_int32, c_int32, c_int64, c_int32, c_int32]),
        "clv_debug_persist_fits": (c_int32, [c_int64, c_int32, c_int32]),
        "clv_group_create": (c_int32, [POINTER(sp), c_int32, c_int32, POINTER(sp)]),
        "clv_group_run": (c_int32, [sp, c_int64]),
        "clv_group_exchange": (c_int32, [sp]),
        "clv_group_destroy": (None, [sp]),
        "clv_predict": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, dp, c_double, c_uint64, c_int32, c_double,
                                  POINTER(c_int64), dp]),
        "clv_predict_sampler": (c_int32, [sp, c_double, c_uint64, c_int32, c_double, POINTER(c_int64), dp]),
        "clv_track": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, dp, dp, c_int32, c_uint64, dp]),
        "clv_track_sampler": (c_int32, [sp, dp, dp, c_int32, c_uint64, dp]),
        "clv_level1_summary": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, c_double, dp]),
        "clv_level1_summary_sampler": (c_int32, [sp, c_double, dp]),
        "clv_chain_total_loglik": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp, dp]),
        "clv_chain_total_loglik_sampler": (c_int32, [sp, dp]),
        "clv_lifetime_value": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, dp, c_double, c_double, c_double,
                                         c_double, dp, dp]),
        "clv_lifetime_value_sampler": (c_int32, [sp, dp, c_double, c_double, c_double, c_double, dp, dp]),
        "clv_ltv_info": (c_int32, [POINTER(c_int64)]),
        "clv_pointwise_loglik": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp, dp, dp,
                                           c_double, dp]),
        "clv_psis_loo": (c_int32, [c_int32, dp, c_int64, c_int64, c_double, dp]),
        "clv_information_criteria": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp, dp, dp,
                                               c_double, c_double, dp]),
        "clv_information_criteria_sampler": (c_int32, [sp, c_int32, c_double, c_double, dp]),
        "clv_ic_info": (c_int32, [POINTER(c_int64)]),
        "clv_debug_information_criteria": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp,
                                                     dp, dp, c_double, c_double, c_int64, c_int32, dp]),
        "clv_score_customers": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64, dp, c_int64, POINTER(c_int32), dp,
                                          dp, dp, dp, c_double, c_int32, c_int32, c_int32, c_uint64, c_int32, c_int64,
                                          c_int64, dp, dp, c_int32, dp, dp, dp, dp]),
        "clv_score_customers_sampler": (c_int32, [sp, c_int64, POINTER(c_int32), dp, dp, dp, dp, c_int32, c_int32,
                                                  c_int32, c_uint64, c_int64, c_int64, dp, dp, c_int32, dp, dp, dp, dp]),
        "clv_score_info": (c_int32, [POINTER(c_int64)]),
        "clv_debug_score_hyper": (c_int32, [c_int32, c_int32, c_int32, c_int64, dp, c_double, dp]),
        "clv_forecast": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp, dp, c_double, c_int32,
                                   POINTER(c_int32), dp, dp]),
        "clv_forecast_sampler": (c_int32, [sp, c_double, c_int32, POINTER(c_int32), dp, dp]),
        "clv_forecast_info": (c_int32, [POINTER(c_int64)]),
        "clv_debug_forecast": (c_int32, [c_int32, dp, c_int64, c_int64, c_int32, POINTER(c_int32), dp, dp, c_double,
                                         c_int32, POINTER(c_int32), c_int64, c_int32, dp, dp]),
        "clv_ppc": (c_int32, [c_int32, c_int32, dp, c_int32, dp, c_int32, c_int32, dp, c_int64, c_int64,
                              POINTER(c_int32), dp, dp, c_int32, c_uint64, c_int64, dp, POINTER(c_int64), dp,
                              POINTER(c_int64), dp]),
        "clv_ppc_sampler": (c_int32, [sp, c_int32, c_int32, c_uint64, dp, POINTER(c_int64), dp, POINTER(c_int64), dp]),
        "clv_ppc_info": (c_int32, [POINTER(c_int64)]),
        "clv_debug_ppc": (c_int32, [c_int32, c_int32, dp, c_int32, dp, c_int32, c_int32, dp, c_int64, c_int64,
                                    POINTER(c_int32), dp, dp, c_int32, c_uint64, c_int64, dp, POINTER(c_int64), dp,
                                    POINTER(c_int64), dp, c_int64, c_int32]),
        "clv_marginal_loglik": (c_int32, [c_int32, dp, c_int32, c_int32, dp, c_int64, c_int64, POINTER(c_int32), dp,
                                          dp, dp, c_double, c_int32, dp]),
        "clv_marginal_information_criteria": (c_int32, [c_int32, dp, c_int32, c_int32, dp, c_int64, c_int64,
                                                        POINTER(c_int32), dp, dp, dp, c_double, c_int32, c_double, dp]),
        "clv_marginal_information_criteria_sampler": (c_int32, [sp, c_int32, c_double, c_double, c_int32, dp]),
        "clv_marginal_info": (c_int32, [POINTER(c_int64)]),
        "clv_debug_marginal_loglik": (c_int32, [c_int32, dp, c_int32, c_int32, dp, c_int64, c_int64, POINTER(c_int32),
                                                dp, dp, dp, c_double, c_int32, c_int64, c_int32, dp, dp]),
        "clv_mml_create": (c_int32, [c_int32, c_int64, POINTER(c_int32), dp, dp, dp, c_int32, dp, POINTER(sp)]),
        "clv_mml_destroy": (None, [sp]),
        "clv_mml_eval": (c_int32, [sp, dp, c_int32, dp, POINTER(c_int64)]),
        "clv_mml_customers": (c_int32, [sp, dp, c_int32, c_double, dp]),
        "clv_debug_mml_eval": (c_int32, [sp, dp, c_int32, c_int32, dp, POINTER(c_int64)]),
        "clv_mml_info": (c_int32, [POINTER(c_int64)]),
        "clv_diagnostics": (c_int32, [c_int32, dp, c_int32, c_int64, c_int64, c_int32, c_uint32, dp]),
        "clv_diagnostics_sampler": (c_int32, [sp, c_uint32, dp, dp]),
        "clv_autocorr": (c_int32, [c_int32, dp, c_int32, c_int64, c_int64, c_int32, dp]),
        "clv_rank_diagnostics": (c_int32, [c_int32, dp, c_int32, c_int64, c_int64, c_int32, c_uint32, c_double, dp]),
        "clv_rank_diagnostics_sampler": (c_int32, [sp, c_uint32, c_double, dp, dp]),
        "clv_debug_zscale": (c_int32, [c_int32, dp, c_int32, c_int64, c_int64, c_int32, dp, dp]),
        "clv_elog2cbs": (c_int32, [c_int32, c_int64, POINTER(c_int64), POINTER(c_int64), dp, c_int64, c_int64, c_int64,
                                   POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), dp, dp, dp, dp,
                                   POINTER(c_int64), dp, dp, POINTER(c_int64), dp]),
        "clv_generate_pareto_abe": (c_int32, [c_int32, c_int64, c_int32, dp, dp, dp, dp, c_int32, dp, c_uint64,
                                              POINTER(c_int64), dp, dp, dp, dp, POINTER(c_uint8), POINTER(c_int64), dp,
                                              POINTER(c_int64), POINTER(c_int64), c_int64, POINTER(c_int64), dp]),
        "clv_pnbd_create": (c_int32, [c_int32, c_int64, POINTER(c_int32), dp, dp, dp, POINTER(sp)]),
        "clv_pnbd_destroy": (None, [sp]),
        "clv_pnbd_eval": (c_int32, [sp, dp, dp, POINTER(c_int64)]),
        "clv_pnbd_customers": (c_int32, [sp, dp, c_double, dp]),
        "clv_pnbd_track": (c_int32, [c_int32, c_int64, dp, dp, c_int32, dp, dp]),
        "clv_pnbd_set_covariates": (c_int32, [sp, c_int32, dp, c_int32, dp]),
        "clv_pnbd_eval_cov": (c_int32, [sp, dp, dp, POINTER(c_int64)]),
        "clv_pnbd_customers_cov": (c_int32, [sp, dp, c_double, dp]),
        "clv_pnbd_track_cov": (c_int32, [c_int32, c_int64, dp, dp, c_int32, dp, c_int32, dp, c_int32, dp, dp]),
        "clv_pnbd_dert": (c_int32, [sp, dp, c_double, c_double, dp]),
        "clv_pnbd_set_integral": (c_int32, [sp, c_int32]),
        "clv_dert_integral": (c_int32, [c_int32, c_int64, dp, dp, dp, dp, dp]),
        "clv_gg_create": (c_int32, [c_int32, c_int64, POINTER(c_int32), dp, dp, POINTER(sp)]),
        "clv_gg_destroy": (None, [sp]),
        "clv_gg_eval": (c_int32, [sp, dp, dp]),
        "clv_gg_customers": (c_int32, [sp, dp, dp]),
        "clv_digamma": (c_int32, [c_int32, c_int64, dp, dp]),
        "clv_batch_fit": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                    c_int64, POINTER(ClvBatchItem), dp]),
        "clv_batch_plan": (c_int32, [c_int64, POINTER(c_int64), c_int32, POINTER(c_int64), POINTER(c_int32),
                                     POINTER(c_int32)]),
        "clv_batch_info": (c_int32, [c_int32, c_int32, POINTER(c_int64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.clv_abi_version() != ABI_VERSION:
        raise ClvError("libclvmcmc.so ABI version mismatch; rebuild it")
    for i, st in enumerate((ClvConfig, ClvData, ClvPrior)):
        if L.clv_sizeof(i) != ctypes.sizeof(st):
            raise ClvError(f"ctypes mirror of {st.__name__} does not match the C struct; rebuild")
    _lib = L
    return L


# Columns of clv_level1_summary() (include/clvmcmc.h CLV_L1_*).
L1_STATS = ("mean_lambda", "lambda_p025", "lambda_p975", "mean_mu", "mean_mu_capped", "mu_p025", "mu_p975",
            "mean_z", "mean_tau", "mean_eta")

# Columns of clv_diagnostics() (include/clvmcmc.h CLV_DIAG_*).
DIAG_STATS = ("mean", "sd", "mcse", "ess", "rhat", "lag")

# Columns of clv_rank_diagnostics() (include/clvmcmc.h CLV_RANK_*), and CLV_RANK_LDS_ELEMS: the
# longest series (chains x draws) that is ranked in LDS; longer ones take global-memory scratch.
RANK_STATS = ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "ess_sd", "mcse_sd",
              "hdi_lo", "hdi_hi", "median", "lag_bulk")
RANK_LDS_ELEMS = 4080

# Columns of clv_lifetime_value() (include/clvmcmc.h CLV_LTV_* / CLV_LTV_DRAW_*).
LTV_STATS = ("value_mean", "value_sd", "value_p025", "value_p50", "value_p975", "residual_mean", "residual_sd",
             "residual_p025", "residual_p50", "residual_p975", "p_alive", "lifetime_yrs", "survival_1yr")
LTV_DRAW_STATS = ("equity", "value_total", "n_alive", "mu_share")
LTV_BATCH_ENV = "CLV_LTV_BATCH"  # customers per sort batch (whole 256-customer blocks): the tests' knob
DIAG_BATCH_ENV = "CLV_DIAG_BATCH"  # series per batch of the diagnostics (csrc/diag.hip batch_series): the tests' knob
SUMMARY_BATCH_ENV = "CLV_SUMMARY_BATCH"  # customers per sort batch of the level-1 summary: the tests' knob
# The limits of csrc/ltv.hip (clv_ltv_info reports the library's own; tests/test_ltv_cpu.py compares):
# customers per reduction block, draws per LDS tile of the transposing pass, keys per sort batch,
# the most stacked draws, draws per LDS tile of the sd kernel.
LTV_BLOCK, LTV_TILE_DRAWS, LTV_BATCH_KEYS, LTV_MAX_DRAWS, LTV_SD_TILE_DRAWS = 256, 16, 1 << 27, 1 << 22, 32


def ltv_info() -> dict:
    """The limits of csrc/ltv.hip (clv_ltv_info): customers per reduction block, draws per tile of
    the transposing pass, keys per sort batch, the most stacked draws, draws per tile of the sd kernel."""
    out = (c_int64 * 5)()
    check(lib().clv_ltv_info(out))
    return dict(block=int(out[0]), tile_draws=int(out[1]), batch_keys=int(out[2]), max_draws=int(out[3]),
                sd_tile_draws=int(out[4]))


# Columns of clv_information_criteria() / clv_psis_loo() (include/clvmcmc.h CLV_IC_*).
IC_STATS = ("lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "pareto_k", "tail_len")
# The limits of csrc/ic.hip (clv_ic_info reports the library's own; tests/test_ic_cpu.py compares):
# customers per workgroup of the pass, draws per LDS tile of its transpose, keys per sort batch, the
# fewest and the most stacked draws, the longest tail, the shortest tail that is fitted.
IC_BLOCK, IC_TILE_DRAWS, IC_BATCH_KEYS, IC_MIN_DRAWS, IC_MAX_DRAWS, IC_MAX_TAIL, IC_MIN_FIT = (
    256, 16, 1 << 27, 8, 1 << 20, 4096, 5)


def ic_info() -> dict:
    """The limits of csrc/ic.hip (clv_ic_info)."""
    out = (c_int64 * 7)()
    check(lib().clv_ic_info(out))
    return dict(block=int(out[0]), tile_draws=int(out[1]), batch_keys=int(out[2]), min_draws=int(out[3]),
                max_draws=int(out[4]), max_tail=int(out[5]), min_fit=int(out[6]))


def score_info() -> dict:
    """clv_score_info: customers per workgroup and the sum-stat count of csrc/score.hip, and of the
    instance this thread's last score_customers call launched (-1 before one): D, K, sink, VGPRs and
    scratch bytes per lane, the kernel's device time in ns."""
    out = (c_int64 * 8)()
    check(lib().clv_score_info(out))
    keys = ("block", "n_sum_stats", "D", "K", "sink", "vgprs", "scratch_bytes", "kernel_ns")
    return {k: int(v) for k, v in zip(keys, out)}


# Columns of clv_forecast() (include/clvmcmc.h CLV_FC_*); the last four are NaN without x_star.
FC_STATS = ("xstar_mean", "p_alive", "p_zero", "q05", "q50", "q95", "tail_mass", "log_score", "pit_lo", "pit_hi",
            "rps")
# The limits of csrc/forecast.hip (clv_forecast_info reports the library's own; tests/test_forecast_cpu.py
# compares): customers per workgroup, the largest k_max, the most stacked draws, the cap on the terms
# of the series that starts the recurrence, the accumulator doubles of one customer batch.
FC_BLOCK, FC_MAX_K, FC_MAX_DRAWS, FC_SERIES_CAP, FC_BATCH_DOUBLES = 256, 4096, (1 << 31) - 1, 4096, 1 << 25


def forecast_info() -> dict:
    """The limits of csrc/forecast.hip (clv_forecast_info)."""
    out = (c_int64 * 5)()
    check(lib().clv_forecast_info(out))
    return dict(block=int(out[0]), max_k=int(out[1]), max_draws=int(out[2]), series_cap=int(out[3]),
                batch_doubles=int(out[4]))


# Columns of clv_ppc() (include/clvmcmc.h CLV_PPC_* / CLV_PPC_DRAW_*): per customer; per draw the integer
# columns that follow the k_hist + 1 histogram bins, and the float column.
PPC_STATS = ("x_rep_mean", "p_x_lt", "p_x_eq", "p_zero", "tx_rep_mean", "p_tx_le", "p_alive_rep")
PPC_DRAW_INTS = ("sum_x", "sum_x2", "max_x", "n_alive")
PPC_DRAW_FLOATS = ("sum_tx",)
PPC_LEVELS = {"customer": 0, "population": 1}
# The limits of csrc/ppc.hip (clv_ppc_info reports the library's own; tests/test_ppc_cpu.py compares):
# customers per workgroup, the largest k_hist, the t_x_rep doubles of one customer batch.
PPC_BLOCK, PPC_MAX_K, PPC_BATCH_DOUBLES = 256, 4096, 1 << 27
PPC_ITEM_ENV = "CLV_PPC_ITEM_DRAWS"  # draws per work item of the replicate kernel (whole 32-draw chunks; default 32): the profile's knob


def ppc_info() -> dict:
    """clv_ppc_info: the limits of csrc/ppc.hip and, of the replicate kernel this thread's last
    posterior predictive check launched (-1 before one), VGPRs and scratch bytes per lane and the
    device time of the call's kernels in ns."""
    out = (c_int64 * 6)()
    check(lib().clv_ppc_info(out))
    keys = ("block", "max_k", "batch_doubles", "vgprs", "scratch_bytes", "kernel_ns")
    return {k: int(v) for k, v in zip(keys, out)}


# The limits of csrc/marginal.hip (clv_marginal_info reports the library's own; tests/test_marginal_cpu.py
# compares): the supported Gauss-Hermite orders and the default, the Newton steps per component,
# customers per workgroup, the most level-2 records, the doubles of one (record, customer) centre.
MARGINAL_ORDERS, MARGINAL_DEFAULT_NODES, MARGINAL_NEWTON, MARGINAL_BLOCK, MARGINAL_MAX_RECORDS, MARGINAL_CENTRE = (
    (8, 16, 24, 32), 32, 16, 256, 1 << 20, 12)


def marginal_info() -> dict:
    """clv_marginal_info: the limits of csrc/marginal.hip and, of the quadrature kernel this thread's
    last marginal-likelihood call launched (-1 before one), VGPRs and scratch bytes per lane and the
    device time of the call's quadrature kernels in ns."""
    out = (c_int64 * 11)()
    check(lib().clv_marginal_info(out))
    return dict(orders=tuple(int(v) for v in out[0:4]), default_nodes=int(out[4]), newton=int(out[5]),
                block=int(out[6]), max_records=int(out[7]), vgprs=int(out[8]), scratch_bytes=int(out[9]),
                kernel_ns=int(out[10]))


# Columns of clv_mml_customers() (include/clvmcmc.h): (da, db) = (log lambda, log mu) - m_i.
MML_ROW = ("loglik", "p_alive", "e_da", "e_db", "e_dada", "e_dadb", "e_dbdb", "xstar")


def mml_info() -> dict:
    """clv_mml_info: customers and lanes per workgroup of csrc/mml.hip, and VGPRs and scratch bytes per
    lane of its eval kernel and of its customers kernel, and the device time in ns of the eval kernel
    of this thread's last clv_mml_eval (-1 before one)."""
    out = (c_int64 * 7)()
    check(lib().clv_mml_info(out))
    keys = ("customers", "block", "eval_vgprs", "eval_scratch_bytes", "customers_vgprs", "customers_scratch_bytes",
            "eval_kernel_ns")
    return {k: int(v) for k, v in zip(keys, out)}


# Many fits in one launch (csrc/batch.hip): the most 256-customer tiles of a fit the batch kernel takes
# (one block per unit, as clv_default_blocks_per_unit gives up to here), and the most tiles at which
# mcmc_draw_parameters_many routes a fit to it by default: the largest T of the tile sweep of
# tools/profile_batch.py at which the full-card batch beat the loop of single fits by 2 in wall time
# (profiles/batch_fits.json).  Measured on one MI355X, bivariate K = 2, 4 chains,
# 2,000 sweeps, summary sink; ratio = wall time of the loop of single calls / wall time of the one call:
#   tiles per fit            1     2     4     8    16    32    64
#   256 fits (full card)  22.3  18.1  12.7   8.4   4.7   2.7   1.7
#   4 fits                 2.25  1.55  0.98  0.56  0.30  0.16  0.10
# 32 is the largest with the full-card ratio >= 2; with 4 fits the batch loses there by 6 x (the rule
# looks at one fit at a time: pass max_blocks for a short list of large fits).
BATCH_TILE_LIMIT = 512
BATCH_MAX_BLOCKS = 32


def exported_symbols():
    """Names of every entry point declared in include/clvmcmc.h (checked by the CPU tests)."""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")
    with open(hdr) as f:
        return sorted(set(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(", f.read())))


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().clv_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(msg)
        raise ClvError(f"libclvmcmc error {rc}: {msg}")


def dptr(a):
    """ctypes double* of a C-contiguous float64 numpy array (or None)."""
    if a is None:
        return None
    return a.ctypes.data_as(POINTER(c_double))


def device_count() -> int:
    n = c_int32(0)
    rc = lib().clv_device_count(ctypes.byref(n))
    if rc != 0:
        return 0
    return n.value

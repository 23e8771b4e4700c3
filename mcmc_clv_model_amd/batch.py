"""Many small fits in one kernel launch (csrc/batch.hip).

A fit of Table-3 size leaves most of the card idle; tens to hundreds of them — the K training sets
of a cross-validation, fits per cohort or country, bootstrap refits, parameter-recovery studies —
fill it.  ``mcmc_draw_parameters_many`` / ``mcmc_draw_parameters_rfm_m_many`` run every fit of a
list with one ``clv_batch_fit`` call: one workgroup per (fit, chain), no hand-off between
workgroups.  ``out[j]`` is, bit for bit, what the single call returns for fit j with
``seed=seeds[j]`` — the routing by ``max_blocks`` between the batch kernel and the single-fit path
is therefore invisible in the results.  ``kfold_cross_validation`` is host glue over these fits
and :func:`analysis.marginal_log_score`: exact K-fold elpd, the check on PSIS-LOO's approximation.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _lib
from ._lib import check
from .sampler import _SINKS, _assemble, build_problem, fit, make_prior, resolve_seed

__all__ = ["mcmc_draw_parameters_many", "mcmc_draw_parameters_rfm_m_many", "kfold_cross_validation",
           "batch_info", "packing_plan", "resolve_seeds", "route", "fold_assignment"]

BATCH_SINKS = ("full", "summary", "none")


def resolve_seeds(n_fits: int, chains: int, seed=None, seeds=None) -> List[int]:
    """One Philox key base per fit.  ``seeds``: one non-negative int per fit, each through
    :func:`sampler.resolve_seed`; otherwise fit j gets ``resolve_seed(seed) + j * chains``, so no two
    chains of a call share a key (chain c of a fit keys on its seed + c, bi:486)."""
    if seeds is not None:
        if seed is not None:
            raise ValueError("give seed or seeds, not both")
        seeds = list(seeds)
        if len(seeds) != n_fits:
            raise ValueError(f"seeds must hold one seed per fit ({n_fits}), got {len(seeds)}")
        if any(s is None for s in seeds):
            raise ValueError("seeds must hold one non-negative int per fit")
        return [resolve_seed(s) for s in seeds]
    base = resolve_seed(seed)
    return [(base + j * int(chains)) & ((1 << 64) - 1) for j in range(n_fits)]


def tiles_of(n: int) -> int:
    """256-customer tiles of a fit of n customers."""
    return -(-int(n) // _lib.BLOCK)


def route(ns: Sequence[int], max_blocks: Optional[int] = None) -> List[str]:
    """"batch" or "solo" per fit: a fit of more than ``max_blocks`` tiles (None: the measured default
    ``_lib.BATCH_MAX_BLOCKS``; never above ``_lib.BATCH_TILE_LIMIT``) runs on the single-fit path, an
    empty one too (the single path defines what it returns); 0 sends every fit there."""
    mb = _lib.BATCH_MAX_BLOCKS if max_blocks is None else int(max_blocks)
    if mb < 0:
        raise ValueError("max_blocks must be >= 0")
    mb = min(mb, _lib.BATCH_TILE_LIMIT)
    return ["batch" if 1 <= tiles_of(n) <= mb else "solo" for n in ns]


def packing_plan(ns: Sequence[int], chains: int) -> dict:
    """clv_batch_plan (host only): how clv_batch_fit packs fits of ``ns`` customers.  ``seg_offsets``
    [n_fits + 1] customers before each fit in the concatenated arrays, ``tiles`` [n_fits], ``wg_map``
    [n_fits * chains, 2] the (fit, chain) of every workgroup, the fits with the most tiles first."""
    F = len(ns)
    n = (ctypes.c_int64 * max(F, 1))(*[int(v) for v in ns])
    seg = np.zeros(F + 1, np.int64)
    tiles = np.zeros(max(F, 1), np.int32)
    wg = np.zeros((max(F * int(chains), 1), 2), np.int32)
    check(_lib.lib().clv_batch_plan(F, n, int(chains), seg.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    wg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return dict(seg_offsets=seg, tiles=tiles[:F], wg_map=wg[:F * int(chains)])


def batch_info(D: int, K: int) -> dict:
    """clv_batch_info: VGPRs, scratch bytes per lane and workgroups per CU of the (D, K) instance of
    the batch kernel, ``slots`` = CUs x workgroups per CU (the (fit, chain) pairs the card runs side
    by side) and the CU count."""
    out = (ctypes.c_int64 * 5)()
    check(_lib.lib().clv_batch_info(int(D), int(K), out))
    return dict(zip(("vgprs", "scratch_bytes", "blocks_per_cu", "slots", "n_cu"), (int(v) for v in out)))


def _problems(cbs_list, covariates, D: int):
    """Every fit's Problem by the single call's own checks and setup; a ValueError names the fit."""
    covariates = list(covariates or [])
    ps = []
    for j, cbs in enumerate(cbs_list):
        try:
            if D == 2:  # bi:461-465 (the trivariate call has no such check of its own)
                for col in ("x", "t_x", "T_cal"):
                    if col not in cbs:
                        raise ValueError(f"cal_cbs missing required column '{col}'")
                if not all(col in cbs for col in covariates):
                    raise ValueError("some covariate columns not in cal_cbs")
            ps.append(build_problem(cbs, covariates, D=D))
        except ValueError as e:
            raise ValueError(f"fit {j}: {e}") from None
        except KeyError as e:
            raise KeyError(f"fit {j}: {e.args[0] if e.args else e}") from None
    return ps


def _run_batch(ps, idx, seeds, D, K, chains, burnin, mcmc, thin, n_mh_steps, draw_sink, device):
    """The fits ``idx`` of ``ps`` through clv_batch_fit: {j: out dict}, kernel ms."""
    n_draws = (mcmc - 1) // thin + 1 if mcmc >= 1 else 0
    l2w = D * K + D * (D + 1) // 2
    items = (_lib.ClvBatchItem * len(idx))()
    keep, bufs = [], {}
    for q, j in enumerate(idx):
        p = ps[j]
        pr = make_prior(p)
        l1 = np.empty((chains, n_draws, p.N, D + 2)) if draw_sink == "full" else None
        l2 = np.empty((chains, n_draws, l2w))
        ll = np.empty((chains, n_draws))
        sums = np.empty((chains, _lib.N_SUM_STATS, p.N)) if draw_sink == "summary" else None
        it = items[q]
        it.n, it.seed = p.N, seeds[j]
        it.x, it.t_x, it.T_cal = p.x.ctypes.data, p.t_x.ctypes.data, p.T_cal.ctypes.data
        it.covariates = p.cov.ctypes.data if K > 1 else None
        it.log_s = p.log_s.ctypes.data if D == 3 else None
        it.prior = ctypes.pointer(pr)
        it.level1 = l1.ctypes.data if l1 is not None and n_draws else None
        it.level2 = l2.ctypes.data if n_draws else None
        it.loglik = ll.ctypes.data if n_draws else None
        it.sums = sums.ctypes.data if sums is not None else None
        keep.append(pr)
        bufs[j] = (l1, l2, ll, sums)
    ms = ctypes.c_double(0.0)
    check(_lib.lib().clv_batch_fit(int(device), D, K, int(n_mh_steps), chains, burnin, mcmc, thin, _SINKS[draw_sink],
                                   len(idx), items, ctypes.byref(ms)))
    outs = {}
    for j in idx:
        l1, l2, ll, sums = bufs[j]
        outs[j] = _assemble(D, chains, l1, l2, ll, sums, n_draws, n_draws, draw_sink, None)
    return outs, float(ms.value)


def _many(D: int, cbs_list, covariates, mcmc, burnin, thin, chains, seed, n_mh_steps, seeds, draw_sink, max_blocks,
          device, return_info):
    cbs_list = list(cbs_list)
    if not cbs_list:
        raise ValueError("cbs_list must hold at least one CBS table")
    chains, mcmc, burnin, thin = int(chains), int(mcmc), int(burnin), int(thin)
    if chains < 1:
        raise ValueError("chains must be >= 1")
    if thin < 1:
        raise ValueError("thin must be >= 1")
    if draw_sink not in BATCH_SINKS:
        raise ValueError(f"draw_sink must be one of {sorted(BATCH_SINKS)} for a batch of fits")
    seeds = resolve_seeds(len(cbs_list), chains, seed, seeds)
    ps = _problems(cbs_list, covariates, D)
    K = ps[0].K
    paths = route([p.N for p in ps], max_blocks)
    if _lib.device_count() < 1:
        raise _lib.ClvError("no HIP device visible; the sampler has no CPU fallback")
    out: List[Optional[dict]] = [None] * len(ps)
    idx = [j for j, w in enumerate(paths) if w == "batch"]
    ms = 0.0
    if idx:
        outs, ms = _run_batch(ps, idx, seeds, D, K, chains, burnin, mcmc, thin, n_mh_steps, draw_sink, device)
        for j, o in outs.items():
            out[j] = o
    for j, w in enumerate(paths):
        if w == "solo":
            out[j] = fit(ps[j], mcmc=mcmc, burnin=burnin, thin=thin, chains=chains, seed=seeds[j], trace=0,
                         n_mh_steps=n_mh_steps, draw_sink=draw_sink, device=device)
    if D == 3:
        for o in out:
            o["log_likelihood"] = float(o["log_likelihood"])  # tri:652 returns a Python float
    if not return_info:
        return out
    info = pd.DataFrame(dict(fit=np.arange(len(ps)), n=[p.N for p in ps], blocks=[tiles_of(p.N) for p in ps],
                             seed=pd.array(seeds, dtype=object), path=paths))
    info.attrs["kernel_ms"] = ms
    return out, info


def mcmc_draw_parameters_many(cbs_list, covariates: Optional[Sequence[str]] = None, mcmc: int = 2500,
                              burnin: int = 500, thin: int = 50, chains: int = 2, seed: Optional[int] = None,
                              n_mh_steps: int = 20, *, seeds: Optional[Sequence[int]] = None, draw_sink: str = "full",
                              max_blocks: Optional[int] = None, device: int = -1, return_info: bool = False):
    """:func:`mcmc_draw_parameters` of every CBS table of ``cbs_list`` — independent fits that share
    the covariate names and every other argument — in one kernel launch.  Returns a list, ``out[j]``
    bit for bit (level_1, level_2, log_likelihood, the summary sink's means, the types) what

        mcmc_draw_parameters(cbs_list[j], covariates, mcmc, burnin, thin, chains, seed=seeds[j], trace=0,
                             n_mh_steps=n_mh_steps, draw_sink=draw_sink)

    returns.  ``seeds``: one per fit; otherwise ``seeds[j] = resolve_seed(seed) + j * chains``
    (:func:`resolve_seeds`).  ``draw_sink``: "full", "summary" or "none".  Fits of more than
    ``max_blocks`` 256-customer tiles run one after another on the single-fit path (None: the
    measured default; 0: all of them) — the same bits either way.  A fit's
    ValueError carries the prefix ``fit j: ``.  No trace lines.  ``return_info=True`` also returns a
    DataFrame (fit, n, blocks, seed, path = "batch" | "solo") with ``attrs["kernel_ms"]``, the batch
    kernel's device time."""
    return _many(2, cbs_list, covariates, mcmc, burnin, thin, chains, seed, n_mh_steps, seeds, draw_sink, max_blocks,
                 device, return_info)


def mcmc_draw_parameters_rfm_m_many(cbs_list, covariates: Optional[Sequence[str]] = None, mcmc: int = 2500,
                                    burnin: int = 500, thin: int = 50, chains: int = 2, seed: Optional[int] = None,
                                    n_mh_steps: int = 20, *, seeds: Optional[Sequence[int]] = None,
                                    draw_sink: str = "full", max_blocks: Optional[int] = None, device: int = -1,
                                    return_info: bool = False):
    """The trivariate counterpart of :func:`mcmc_draw_parameters_many`: ``out[j]`` is bit for bit
    ``mcmc_draw_parameters_rfm_m(cbs_list[j], ..., seed=seeds[j], trace=0, ...)``."""
    return _many(3, cbs_list, covariates, mcmc, burnin, thin, chains, seed, n_mh_steps, seeds, draw_sink, max_blocks,
                 device, return_info)


def fold_assignment(n: int, k: int, fold_seed: int = 0) -> np.ndarray:
    """The fold of every customer: a ``numpy.random.default_rng(fold_seed)`` permutation dealt round
    the k folds, so every customer is in exactly one fold and fold sizes differ by at most one."""
    n, k = int(n), int(k)
    if k < 2:
        raise ValueError("k must be >= 2")
    if n < k:
        raise ValueError(f"k = {k} folds need at least {k} customers (got {n})")
    fold = np.empty(n, np.int64)
    fold[np.random.default_rng(fold_seed).permutation(n)] = np.arange(n) % k
    return fold


def kfold_cross_validation(cbs, covariates: Optional[Sequence[str]] = None, *, k: int = 10, model: str = "bivariate",
                           fold_seed: int = 0, spend: bool = False, nodes=None, loo=None, **fit_kwargs) -> dict:
    """Exact K-fold cross-validation of a fit: the customers are dealt into k folds
    (:func:`fold_assignment`), the k training sets are fitted in one launch (``model`` = "bivariate" |
    "trivariate"; ``fit_kwargs`` go to the ``_many`` call) and every held-out fold is scored with
    :func:`analysis.marginal_log_score` against the fit that did not see it.

    Returns ``pointwise`` (one row per customer in the order of ``cbs``: elpd_kfold, fold),
    ``estimates`` (elpd_kfold and its standard error sqrt(N var(., ddof 0)) through
    ``fixed_order_sum``, as marginal_log_score forms its own), ``folds`` (per fold: n, elpd_kfold)
    and, when ``loo`` is the :func:`analysis.marginal_information_criteria` result of the whole data,
    ``loo_difference`` (elpd_loo - elpd_kfold, paired, with its standard error)."""
    from . import analysis as A
    if model not in ("bivariate", "trivariate"):
        raise ValueError("model must be 'bivariate' or 'trivariate'")
    if "return_info" in fit_kwargs:
        raise ValueError("return_info is not an argument of kfold_cross_validation")
    frame = cbs.reset_index(drop=True)
    n = len(frame)
    fold = fold_assignment(n, k, fold_seed)
    many = mcmc_draw_parameters_many if model == "bivariate" else mcmc_draw_parameters_rfm_m_many
    fits = many([frame[fold != f] for f in range(k)], covariates, **fit_kwargs)
    score = np.full(n, np.nan)
    for f in range(k):
        held = frame[fold == f]
        s = A.marginal_log_score(fits[f], held, covariates, spend=spend, nodes=nodes,
                                 device=fit_kwargs.get("device", -1))
        score[np.flatnonzero(fold == f)] = s["pointwise"]["log_score"].to_numpy()

    def total(v):
        t = A.fixed_order_sum(v)
        dev = v - t / len(v)
        return t, float(np.sqrt(len(v) * (A.fixed_order_sum(dev * dev) / len(v))))
    elpd, se = total(score)
    out = dict(pointwise=pd.DataFrame(dict(elpd_kfold=score, fold=fold)),
               estimates=pd.DataFrame([dict(elpd_kfold=elpd, se=se, k=int(k), n_customers=int(n))]),
               folds=pd.DataFrame(dict(fold=np.arange(k), n=[int(np.count_nonzero(fold == f)) for f in range(k)],
                                       elpd_kfold=[A.fixed_order_sum(score[fold == f]) for f in range(k)])))
    if loo is not None:
        pl = loo["pointwise"]["elpd_loo"].to_numpy()
        if pl.shape[0] != n:
            raise ValueError("loo must be the marginal_information_criteria result of the same customers")
        d, dse = total(pl - score)
        out["loo_difference"] = pd.DataFrame([dict(elpd_diff=d, se=dse)])
    return out

"""WAIC and PSIS-LOO without a device: the C ABI's declarations and argument checks, the validation
of the Python layer, the float64 model (tests/ic_ref.py) against 40-digit mpmath and against the
properties its definitions imply, and compare_models' arithmetic.

The model's own error, measured here against mpmath (fixtures of N = 64 customers x S = 100 draws):
  E_L     largest relative deviation of the pointwise log-likelihood, the spend term included, on a
          fixture with the extreme rows (log lambda = +-70, mu = e^5, x = 0, t_x = 0, t_x = T_cal):
          measured 6.47e-16, recorded 7e-16;
  E_STAT  largest deviation of lppd, p_waic, elpd_loo (relative: 7.99e-16, 2.6e-16, 5.7e-16) and of
          pareto_k (absolute: 2.8e-16), on ic_ref.planted_matrix (tails of 20 values; a tied, a
          constant and a dominated series among them): measured 7.99e-16, recorded 8e-16.
Both are recorded rounded up to one digit (ic_ref.E_L, ic_ref.E_STAT); the GPU tolerances of
tests/test_gpu_ic.py are 4 x these.
Without the spend term the log-likelihood of a customer with x = 0, t_x = 0 and mu >> lambda is
log(mu) - log(lambda + mu), which cancels to nothing: there no relative bound holds for any float64
evaluation of the formula, and the bound is the floor of 4 ulp of the largest term (ic_ref.loglik_scale)."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import ic_ref as R

E_L, E_STAT, ULP = R.E_L, R.E_STAT, R.ULP

NEW_SYMBOLS = ("clv_pointwise_loglik", "clv_psis_loo", "clv_information_criteria", "clv_information_criteria_sampler",
               "clv_ic_info", "clv_debug_information_criteria")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")


def test_header_declares_and_library_exports_the_new_symbols():
    from mcmc_clv_model_amd import _lib
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    with open(HDR) as f:
        text = f.read()
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2


def test_enum_order_matches_the_column_names():
    from mcmc_clv_model_amd import _lib
    with open(HDR) as f:
        text = " ".join(f.read().split())
    cols = re.search(r"enum \{ (CLV_IC_LPPD = 0,[^}]*?CLV_N_IC_STATS) \}", text).group(1)
    names = [t.strip().split(" ")[0] for t in cols.split(",")]
    assert names == ["CLV_IC_" + c.upper() for c in _lib.IC_STATS] + ["CLV_N_IC_STATS"]
    assert _lib.IC_STATS == R.STATS and len(_lib.IC_STATS) == 7


def test_limits_are_exported():
    from mcmc_clv_model_amd import _lib
    info = _lib.ic_info()
    assert info == dict(block=_lib.IC_BLOCK, tile_draws=_lib.IC_TILE_DRAWS, batch_keys=_lib.IC_BATCH_KEYS,
                        min_draws=_lib.IC_MIN_DRAWS, max_draws=_lib.IC_MAX_DRAWS, max_tail=_lib.IC_MAX_TAIL,
                        min_fit=_lib.IC_MIN_FIT)
    assert info["block"] == 256 == _lib.BLOCK and info["min_draws"] == 8 and info["min_fit"] == R.MIN_FIT
    assert R.tail_max(info["max_draws"]) <= info["max_tail"] and info["max_draws"] >= 4000


# ---- the C ABI's argument checks: -1 before any device call ---------------------------------------
def _c_args(S=8, N=3, width=5):
    l1, d = R.synth_case(S, N, width, seed=2)
    from mcmc_clv_model_amd._lib import dptr
    i32 = d["x"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    keep = (l1, d)
    return keep, dict(level1=dptr(l1), n_draws=S, n=N, width=width, x=i32, t_x=dptr(d["t_x"]), T_cal=dptr(d["T_cal"]),
                      log_s=dptr(d["log_s"]) if width == 5 else None, omega2=0.3, reff=1.0)


BAD = [dict(level1=None), dict(x=None), dict(t_x=None), dict(T_cal=None), dict(out=None),
       dict(n_draws=7), dict(n_draws=0), dict(n=0), dict(n=-1), dict(width=3), dict(width=6),
       dict(width=4),                                       # log_s (the spend term) with width 4
       dict(reff=0.0), dict(reff=-1.0), dict(reff=float("inf")), dict(reff=float("nan")),
       dict(omega2=0.0), dict(omega2=-0.5), dict(omega2=float("nan")), dict(omega2=float("inf"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_c_abi_rejects_bad_arguments(bad):
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    keep, a = _c_args()
    out = np.empty((8 * 3 * 7,), np.float64)
    a["out"] = dptr(out)
    a.update(bad)
    order = ("level1", "n_draws", "n", "width", "x", "t_x", "T_cal", "log_s", "omega2")
    head = [0] + [a[k] for k in order]
    if "reff" not in bad:
        assert L.clv_pointwise_loglik(*head, a["out"]) == -1
        assert L.clv_last_error()
    assert L.clv_information_criteria(*head, a["reff"], a["out"]) == -1
    assert L.clv_debug_information_criteria(*head, a["reff"], 0, 0, a["out"]) == -1
    if set(bad) <= {"n_draws", "n", "reff", "out"}:
        ll = a["level1"] if "level1" not in bad else None
        assert L.clv_psis_loo(0, ll, a["n_draws"], a["n"], a["reff"], a["out"]) == -1


def test_c_abi_rejects_the_rest():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    keep, a = _c_args()
    out = np.empty((8 * 3 * 7,), np.float64)
    assert L.clv_psis_loo(0, None, 8, 3, 1.0, dptr(out)) == -1
    assert L.clv_ic_info(None) == -1
    assert L.clv_information_criteria_sampler(None, 0, 1.0, 1.0, dptr(out)) == -1
    head = [0] + [a[k] for k in ("level1", "n_draws", "n", "width", "x", "t_x", "T_cal", "log_s", "omega2")]
    assert L.clv_debug_information_criteria(*head, 1.0, -1, 0, dptr(out)) == -1
    assert L.clv_debug_information_criteria(*head, 1.0, 0, -1, dptr(out)) == -1
    # reff so small that the tail would not fit the kernel's LDS
    big = _lib.IC_MAX_TAIL * 5 + 5
    assert L.clv_psis_loo(0, dptr(out), big, 1, 1e-9, dptr(out)) == -1
    assert L.clv_psis_loo(0, dptr(out), _lib.IC_MAX_DRAWS + 1, 1, 1.0, dptr(out)) == -1


# ---- the Python layer ------------------------------------------------------------------------------
def _py_case(width=5, S=8, N=3):
    l1, d = R.synth_case(S, N, width, seed=2)
    return {"level_1": [l1[:S // 2], l1[S // 2:]]}, pd.DataFrame(d)


@pytest.mark.parametrize("kw", [
    dict(reff=0.0), dict(reff=-1.0), dict(reff=float("inf")), dict(reff=float("nan")),
    dict(spend=True, omega2=0.0), dict(spend=True, omega2=-1.0), dict(spend=True, omega2=float("nan")),
    dict(omega2=0.3),                                                    # omega2 without the spend term
])
def test_wrappers_reject_bad_arguments_without_a_device(kw):
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case(5)
    with pytest.raises(ValueError):
        A.information_criteria(draws, cbs, **kw)
    if "reff" not in kw:
        with pytest.raises(ValueError):
            A.pointwise_log_likelihood(draws, cbs, **kw)
    else:
        with pytest.raises(ValueError):
            A.psis_loo(np.zeros((8, 3)), **kw)


def test_wrappers_reject_bad_shapes_without_a_device():
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case(4)
    for fn in (A.information_criteria, A.pointwise_log_likelihood):
        with pytest.raises(ValueError):
            fn(draws, cbs, spend=True)                                   # spend with width 4
        with pytest.raises(ValueError):
            fn({"level_1": None}, cbs)                                   # a "summary" sink's result
        with pytest.raises(ValueError):
            fn({"level_1": [draws["level_1"][0]]}, cbs)                  # 4 < 8 draws
        with pytest.raises(ValueError):
            fn(draws, cbs.iloc[:2])                                      # cbs of another size
        with pytest.raises(ValueError):
            fn({"level_1": [np.ones((8, 3, 6))]}, cbs)                   # a bad width
    d5, c5 = _py_case(5)
    with pytest.raises(ValueError):
        A.information_criteria(d5, c5.drop(columns="log_s"), spend=True)
    with pytest.raises(ValueError):
        A.psis_loo(np.zeros((7, 3)))
    with pytest.raises(ValueError):
        A.psis_loo(np.zeros((8, 0)))
    with pytest.raises(ValueError):
        A.psis_loo(np.zeros(8))


def test_fit_keyword_is_validated_before_the_run():
    from mcmc_clv_model_amd.sampler import information_criteria_kwargs as kwargs
    assert kwargs(None, "summary", 2) is None and kwargs(False, "summary", 2) is None
    assert kwargs(True, "full", 2) == {}
    assert kwargs(dict(reff=0.5), "full", 2) == dict(reff=0.5)
    assert kwargs(dict(spend=True), "full", 3) == dict(spend=True)
    for bad, sink, D in ((True, "summary", 2), (True, "summary+pct", 2), (dict(reff=-1.0), "full", 2),
                         (dict(reffs=1.0), "full", 2), ("yes", "full", 2), (dict(spend=True), "full", 2),
                         (dict(spend=True, omega2=0.0), "full", 3), (dict(omega2=0.5), "full", 3)):
        with pytest.raises(ValueError):
            kwargs(bad, sink, D)


# ---- the model against mpmath ----------------------------------------------------------------------
def test_model_loglik_against_mpmath():
    S, N = 100, 64
    l1, d = R.synth_case(S, N, 5, seed=11, extremes=True)
    w2 = float(np.var(d["log_s"], ddof=1))
    ll = R.loglik(l1, d, True, w2)
    assert np.isfinite(ll).all()
    mp = R.mp_loglik_matrix(l1, d, True, w2)
    e_l = max(R.rel_dev(ll[s, i], mp[s, i]) for s in range(S) for i in range(N))
    print(f"e_l = {e_l:.3g}")
    assert e_l <= E_L
    # the transaction part alone: the same bound where it does not cancel, the floor where it does
    ll4, scale = R.loglik(l1, d), R.loglik_scale(l1, d)
    mp4 = R.mp_loglik_matrix(l1[:8], d)
    for s in range(8):
        for i in range(N):
            assert R.abs_dev(ll4[s, i], mp4[s, i]) <= max(E_L * abs(float(mp4[s, i])), 4 * ULP * scale[s, i]), (s, i)


def test_model_statistics_against_mpmath():
    S, N = 100, 64
    ll = R.planted_matrix(S, N, seed=12)
    m = R.model(ll)
    e = dict(lppd=0.0, p_waic=0.0, elpd_loo=0.0, pareto_k=0.0)
    for i in range(N):
        r = R.mp_stats(ll[:, i])
        assert r["tail_len"] == m[i, 6] == {R.TIED: 18, R.CONST: 0}.get(i, 20)
        assert np.isfinite(m[i, 5]) == (i != R.CONST) and (r["pareto_k"] == np.inf) == (i == R.CONST)
        for k in ("lppd", "p_waic", "elpd_loo"):
            if i != R.CONST or k != "p_waic":                # the constant series: p_waic is 0 exactly
                e[k] = max(e[k], R.rel_dev(m[i, R.STATS.index(k)], r[k]))
        if i != R.CONST:
            e["pareto_k"] = max(e["pareto_k"], R.abs_dev(m[i, 5], r["pareto_k"]))
    assert m[R.CONST, 1] == 0.0 and m[R.DOMINANT, 5] > 0.7
    print("e_stat:", {k: f"{v:.3g}" for k, v in e.items()})
    assert max(e.values()) <= E_STAT
    assert np.array_equal(m[:, 2], m[:, 0] - m[:, 1]) and np.array_equal(m[:, 4], m[:, 0] - m[:, 3])


# ---- the model's properties ------------------------------------------------------------------------
def test_constant_series():
    for S, l in ((8, -3.25), (100, -17.0), (4000, -0.5)):
        row = R.model(np.full((S, 1), l))[0]
        # (l + log S) - log S, twice: one rounding of l + log S each way
        tol = 4 * ULP * (abs(l) + np.log(S))
        assert abs(row[3] - l) <= tol and abs(row[0] - l) <= tol and abs(row[4]) <= 2 * tol
        assert row[1] == 0.0 and row[5] == np.inf and row[6] == 0


def test_weights_sum_to_one():
    g = np.random.default_rng(5)
    for S in (8, 20, 25, 100, 1000, 4000):
        for scale in (0.3, 3.0):
            l = g.normal(-5.0, scale, S)
            logw = R.psis_one(l)[3]
            assert abs(np.exp(logw).sum() - 1.0) <= 4 * ULP, (S, scale)
            assert np.all(logw <= 0.0)


def test_short_tails_are_never_fitted():
    g = np.random.default_rng(6)
    assert R.tail_max(20) == 4 and R.tail_max(25) == 5 and R.tail_max(8) == 2
    for _ in range(20):
        elpd, k, n, logw = R.psis_one(g.normal(0.0, 2.0, 20))
        assert k == np.inf and n == 4
        # raw weights: proportional to exp(-l)
    l = g.normal(0.0, 2.0, 25)
    elpd, k, n, logw = R.psis_one(l)
    assert n == 5 and np.isfinite(k)
    raw = -np.sort(l)
    raw = raw - R.logsumexp(raw)
    assert not np.allclose(logw[:5], raw[:5]) and np.all(np.diff(logw[:5]) <= 0.0)
    elpd20, k20, n20, logw20 = R.psis_one(l[:20])
    raw = -np.sort(l[:20])
    assert np.allclose(logw20, raw - R.logsumexp(raw), rtol=0, atol=1e-14)


def test_ties_straddling_the_cutoff_shorten_the_tail():
    g = np.random.default_rng(7)
    l = np.sort(g.normal(0.0, 1.0, 100))          # M = 20: the cutoff is the 21st smallest l
    assert R.psis_one(l)[2] == 20
    tied = l.copy()
    tied[17:24] = l[20]                           # values 18 .. 24 equal: 18 .. 20 fall out of the tail
    elpd, k, n, _ = R.psis_one(tied)
    assert n == 17 and np.isfinite(k)
    tied[3:24] = l[20]
    assert R.psis_one(tied)[1:3] == (np.inf, 3)   # 3 values left: not fitted


def test_generalised_pareto_ratios_are_ranked():
    ks = [R.psis_one(R.gpd_series(k, 4000, 1)) for k in (0.2, 0.5, 0.9)]
    print("khat:", [f"{r[1]:.3f}" for r in ks])
    assert all(r[2] == R.tail_max(4000) == 190 for r in ks)
    assert 0.0 < ks[0][1] < ks[1][1] < ks[2][1] < 1.5
    assert ks[0][1] < 0.7 < ks[2][1]


def test_bad_k_threshold():
    from mcmc_clv_model_amd.analysis import bad_k_threshold
    assert bad_k_threshold(4000) == 0.7 == R.bad_k_threshold(4000)
    assert bad_k_threshold(100) == 0.5 and abs(bad_k_threshold(1000) - (1 - 1 / 3)) < 1e-15


# ---- totals and compare_models on hand-made frames -------------------------------------------------
def _frames(elpd_loo, k=None, S=100):
    from mcmc_clv_model_amd import analysis as A
    n = len(elpd_loo)
    st = np.zeros((n, 7))
    st[:, 0] = np.asarray(elpd_loo) + 0.25
    st[:, 1] = 0.5
    st[:, 2] = st[:, 0] - st[:, 1]
    st[:, 3] = elpd_loo
    st[:, 4] = 0.25
    st[:, 5] = 0.1 if k is None else k
    st[:, 6] = 20
    return A.ic_frames(st, S)


def test_totals_use_the_fixed_order_sum():
    from mcmc_clv_model_amd import analysis as A
    from tests.pnbd_ref import device_sum
    g = np.random.default_rng(8)
    for n in (1, 255, 257, 70000):
        v = g.normal(-4.0, 2.0, n)
        assert A.fixed_order_sum(v) == device_sum(v)
    v = g.normal(-4.0, 2.0, 600)
    k = np.full(600, 0.2)
    k[[3, 77]] = [0.9, np.inf]
    f = _frames(v, k, S=4000)
    loo, waic = f["loo"].iloc[0], f["waic"].iloc[0]
    assert list(f["loo"].columns) == ["elpd", "se", "p", "n_samples", "n_data_points", "n_bad_k", "warning"]
    assert loo["elpd"] == device_sum(v) and loo["p"] == 150.0 and loo["n_samples"] == 4000 and loo["n_data_points"] == 600
    assert np.isclose(loo["se"], np.sqrt(600 * v.var()), rtol=1e-13) and np.isclose(loo["elpd"], v.sum(), rtol=1e-13)
    assert loo["n_bad_k"] == 2 and bool(loo["warning"]) and waic["n_bad_k"] == 0 and bool(waic["warning"])
    assert waic["p"] == 300.0 and np.isclose(waic["elpd"], (v - 0.25).sum(), rtol=1e-13)
    assert list(f["pointwise"].columns) == list(R.STATS)
    quiet = _frames(v)
    assert not bool(quiet["loo"].iloc[0]["warning"]) and quiet["loo"].iloc[0]["n_bad_k"] == 0


def test_compare_models_arithmetic():
    from mcmc_clv_model_amd import analysis as A
    a = np.array([-1.0, -2.0, -3.0, -4.0])
    b = np.array([-1.5, -2.0, -2.0, -5.5])
    c = np.array([-3.0, -3.0, -3.0, -3.0])
    cmp = A.compare_models({"A": _frames(a), "B": _frames(b), "C": _frames(c)})
    assert list(cmp.index) == ["A", "B", "C"] and list(cmp["rank"]) == [0, 1, 2]
    assert list(cmp["elpd"]) == [-10.0, -11.0, -12.0] and list(cmp["elpd_diff"]) == [0.0, 1.0, 2.0]
    assert cmp.loc["A", "dse"] == 0.0
    assert cmp.loc["B", "dse"] == np.sqrt(4 * np.var(a - b)) and cmp.loc["C", "dse"] == np.sqrt(4 * np.var(a - c))
    assert cmp.loc["B", "se"] == np.sqrt(4 * np.var(b)) and list(cmp["p"]) == [1.0, 1.0, 1.0]
    w = A.compare_models({"A": _frames(a), "B": _frames(b)}, criterion="waic")
    assert list(w["elpd"]) == [-11.0, -12.0] and list(w["p"]) == [2.0, 2.0]
    with pytest.raises(ValueError):
        A.compare_models({"A": _frames(a), "B": _frames(b[:3])})
    with pytest.raises(ValueError):
        A.compare_models({"A": _frames(a)}, criterion="dic")
    with pytest.raises(ValueError):
        A.compare_models({})

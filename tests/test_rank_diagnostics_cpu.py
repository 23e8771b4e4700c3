"""Rank-normalised diagnostics without a GPU: the C ABI's declarations and argument checks, the frame
builders and az.summary's column names, and the yardstick itself (tests/diagnostics_rank_ref.py) —
known answers, and the decision margins that make the exact comparison of the truncation lag in
tests/test_gpu_rank_diagnostics.py fair."""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import diagnostics_rank_ref as K
from tests import diagnostics_ref as R

NEW_SYMBOLS = ("clv_rank_diagnostics", "clv_rank_diagnostics_sampler", "clv_debug_zscale")


def rank_input_sets():
    """Names (diagnostics_rank_ref.reference) of every input set of the GPU parity tests."""
    from mcmc_clv_model_amd import _lib
    half = _lib.RANK_LDS_ELEMS // 2
    return ([f"small:{m}:{n}" for m, n in R.SMALL_SHAPES] + [f"min:{m}:{n}" for m, n in R.MIN_SHAPES]
            + ["long", f"threshold:{half}", f"threshold:{half + 1}", "golden:bi", "golden:tri"])


def test_header_declares_and_library_exports_the_new_symbols():
    from mcmc_clv_model_amd import _lib
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")
    with open(hdr) as f:
        text = f.read()
    enum = ("CLV_RANK_RHAT = 0, CLV_RANK_RHAT_BULK, CLV_RANK_RHAT_FOLDED, CLV_RANK_ESS_BULK, CLV_RANK_ESS_TAIL, "
            "CLV_RANK_ESS_Q05, CLV_RANK_ESS_Q95, CLV_RANK_ESS_SD, CLV_RANK_MCSE_SD, CLV_RANK_HDI_LO, CLV_RANK_HDI_HI, "
            "CLV_RANK_MEDIAN, CLV_RANK_LAG_BULK, CLV_N_RANK_STATS")
    assert enum in " ".join(text.split())
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert f"#define CLV_RANK_LDS_ELEMS {_lib.RANK_LDS_ELEMS}\n" in text
    assert _lib.RANK_LDS_ELEMS >= 4000  # the benchmark shape, 4 x 1,000, is ranked in LDS
    assert _lib.RANK_STATS == K.STATS and len(_lib.RANK_STATS) == 13
    assert _lib.DIAG_STATS == R.STATS
    import mcmc_clv_model_amd as pkg
    for n in ("level1_rank_diagnostics", "level2_rank_diagnostics", "level2_summary"):
        assert n in pkg.__all__ and callable(getattr(pkg, n))


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    x = np.zeros((2, 16, 3))
    out = np.zeros((3, 13))
    rk, z = np.zeros((3, 4, 8)), np.zeros((3, 4, 8))
    ok = dict(series=dptr(x), m=2, n=16, ns=3, period=1, p=0.94, out=dptr(out))

    def rank(**kw):
        a = dict(ok, **kw)
        return L.clv_rank_diagnostics(0, a["series"], a["m"], a["n"], a["ns"], a["period"], 0, a["p"], a["out"])

    for kw in (dict(series=None), dict(out=None), dict(m=0), dict(n=7), dict(ns=0), dict(period=0), dict(period=33),
               dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(p=1.5), dict(p=float("nan"))):
        assert rank(**kw) == -1, kw
        assert L.clv_last_error()

    def zscale(series=dptr(x), m=2, n=16, ns=3, folded=0, ranks=dptr(rk), zz=dptr(z)):
        return L.clv_debug_zscale(0, series, m, n, ns, folded, ranks, zz)

    for kw in (dict(series=None), dict(ranks=None), dict(zz=None), dict(m=0), dict(n=7), dict(ns=0)):
        assert zscale(**kw) == -1, kw
    assert L.clv_rank_diagnostics_sampler(None, 3, 0.94, dptr(out), None) == -1


def test_frames_and_column_names_need_no_device():
    from mcmc_clv_model_amd import analysis as A
    assert A.hdi_column_names(0.94) == ("hdi_3%", "hdi_97%")
    assert A.hdi_column_names(0.95) == ("hdi_2.5%", "hdi_97.5%")
    assert A.hdi_column_names(0.5) == ("hdi_25%", "hdi_75%")
    for bad in (0.0, 1.0, -1, 2, float("nan")):
        with pytest.raises(ValueError, match="hdi_prob"):
            A.hdi_column_names(bad)
    with pytest.raises(ValueError, match="hdi_prob"):
        A.level2_summary({"level_2": [np.zeros((16, 3))] * 2}, hdi_prob=1.0)
    with pytest.raises(ValueError, match="draw_sink='full'"):
        A.level1_rank_diagnostics({"level_1": None, "level_2": []})
    ns = len(K.STATS)
    st = np.arange(2 * 4 * ns, dtype=float).reshape(8, ns)
    df = A.level1_rank_diagnostics_frame(st, 2, 4, 3)
    assert list(df.columns[:ns]) == [f"{s}_log_lambda" for s in K.STATS]
    assert list(df.columns[2 * ns:3 * ns]) == [f"{s}_tau" for s in K.STATS] and "rhat_z" in df and "ess_bulk_log_mu" in df
    assert df.shape == (2, 4 * ns) and df["lag_bulk_log_mu"].tolist() == [2.0 * ns - 1, 6.0 * ns - 1]
    assert list(A.level1_rank_diagnostics_frame(st, 2, 4, 0).columns[:ns]) == [f"{s}_lambda" for s in K.STATS]
    d2 = A.level2_rank_diagnostics_frame(st[:5], list("abcde"))
    assert list(d2.columns) == list(K.STATS) and list(d2.index) == list("abcde")
    with pytest.raises(ValueError):
        A.level2_rank_diagnostics_frame(st[:5], ["a"])
    six = np.arange(30, dtype=float).reshape(5, 6) + 100
    for p, names in ((0.94, ("hdi_3%", "hdi_97%")), (0.95, ("hdi_2.5%", "hdi_97.5%"))):
        sm = A.level2_summary_frame(six, st[:5], list("abcde"), p)
        assert list(sm.columns) == ["mean", "sd", names[0], names[1], "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat"]
        assert list(sm.index) == list("abcde")
        want = np.stack([six[:, 0], six[:, 1], st[:5, K.HDI_LO], st[:5, K.HDI_HI], six[:, 2], st[:5, K.MCSE_SD],
                         st[:5, K.ESS_BULK], st[:5, K.ESS_TAIL], st[:5, K.RHAT]], axis=1)
        assert np.array_equal(sm.to_numpy(), want)
    assert list(A.level2_summary_frame(six, st[:5]).index) == [f"level_2[{i}]" for i in range(5)]


def test_yardstick_known_answers():
    rng = np.random.default_rng(31)
    # ranks, hence the bulk R-hat and ESS and the tail indicators, do not change under a monotone map
    # (the folded R-hat may: here the bulk one is the larger on both scales, so rhat keeps its bits)
    y = R.ar1(rng, 4, 200, 0.6) * 0.5
    a, _ = K.rank_series_stats(y)
    b, _ = K.rank_series_stats(np.exp(y))
    c, _ = K.rank_series_stats(np.exp(y), log=True)
    assert a[K.RHAT] == b[K.RHAT] and a[K.ESS_BULK] == b[K.ESS_BULK] and a[K.LAG_BULK] == b[K.LAG_BULK]
    assert a[K.RHAT_BULK] == b[K.RHAT_BULK] and a[K.ESS_Q05] == b[K.ESS_Q05]
    np.testing.assert_allclose(c, a, rtol=1e-9)
    assert a[K.RHAT] == max(a[K.RHAT_BULK], a[K.RHAT_FOLDED]) and a[K.ESS_TAIL] == min(a[K.ESS_Q05], a[K.ESS_Q95])
    # one chain with triple the scale and the same mean: only the folded R-hat sees it
    y = rng.standard_normal((4, 1000))
    y[3] *= 3.0
    s, _ = K.rank_series_stats(y)
    print("scale: rhat_bulk", s[K.RHAT_BULK], "rhat_folded", s[K.RHAT_FOLDED])
    assert s[K.RHAT_FOLDED] > 1.05 and s[K.RHAT_BULK] < 1.02 and s[K.RHAT] == s[K.RHAT_FOLDED]
    # independent draws: every ESS near the number of draws, mcse_sd near sd / sqrt(2 N)
    y = rng.standard_normal((4, 1000))
    s, _ = K.rank_series_stats(y)
    for k in (K.ESS_BULK, K.ESS_Q05, K.ESS_Q95, K.ESS_SD):
        assert 0.75 * 4000 < s[k] < 1.35 * 4000, (K.STATS[k], s[k])
    assert s[K.MCSE_SD] == pytest.approx(y.std() / np.sqrt(2 * 4000), rel=0.15)
    # the HDI is a pick of two data values, the first narrowest interval of floor(P N) steps
    assert K.hdi(np.arange(100.0), 0.94) == (0.0, 94.0)
    assert K.hdi(np.r_[0.0, 10.0, 11.0, 12.0, 13.0, 30.0], 0.5) == (10.0, 13.0)
    s, _ = K.rank_series_stats(np.arange(100.0).reshape(2, 50))
    assert (s[K.HDI_LO], s[K.HDI_HI], s[K.MEDIAN]) == (0.0, 94.0, 49.5)
    # average ranks with ties, over the pooled split chains, in split-chain order
    sp = K.split_chains(np.array([[3.0, 1, 1, 2, 9, 2, 2, 5, 1]]))  # odd n: the middle draw (9) is dropped
    assert sp.tolist() == [[3.0, 1, 1, 2], [2.0, 2, 5, 1]]
    r, z = K.zscale(sp)
    assert r.tolist() == [[7.0, 2, 2, 5], [5.0, 5, 8, 2]]
    np.testing.assert_allclose(z, K.ndtri((r - 0.375) / 8.25), rtol=0, atol=0)
    assert K.zscale(np.full((2, 4), 7.0))[1].tolist() == [[0.0] * 4] * 2  # all tied: rank (S + 1) / 2, z exactly 0


def test_yardstick_nan_policy():
    y = R.ar1(3, 2, 40, 0.3)
    bad = y.copy()
    bad[1, 7] = np.nan
    assert np.isnan(K.rank_series_stats(bad)[0]).all()
    assert np.isnan(K.rank_series_stats(-np.abs(y), log=True)[0]).all()
    s, _ = K.rank_series_stats(np.full((2, 40), 2.5))  # constant: only the picks are finite
    finite = np.isfinite(s)
    assert [K.STATS[k] for k in np.flatnonzero(finite)] == ["hdi_lo", "hdi_hi", "median"] and (s[finite] == 2.5).all()
    z = (np.random.default_rng(5).random((2, 40)) < 0.3).astype(float)  # binary, 30 % ones
    s, _ = K.rank_series_stats(z)
    assert np.isfinite(s[[K.ESS_BULK, K.RHAT_BULK, K.ESS_Q05, K.ESS_SD, K.MCSE_SD]]).all()
    assert np.isnan(s[K.ESS_Q95]) and np.isnan(s[K.ESS_TAIL])  # I(z <= 1) is all ones
    assert np.isfinite(s[K.RHAT_FOLDED]) and np.isfinite(s[K.RHAT])  # median 0: |z - 0| is z itself
    half = np.tile([0.0, 1.0], (2, 20))  # median 0.5 and mean 0.5: the folded and the squared series are constant
    s, _ = K.rank_series_stats(half)
    assert np.isnan(s[[K.RHAT_FOLDED, K.RHAT, K.ESS_SD, K.MCSE_SD]]).all() and np.isfinite(s[[K.RHAT_BULK, K.ESS_BULK]]).all()


@pytest.mark.parametrize("name", rank_input_sets())
def test_decision_margins_allow_the_exact_lag_comparison(name):
    """Every comparison against zero in Geyer's truncation, in each of the four ESS evaluations (bulk,
    q05, q95, sd), is at least 1e-6 from going the other way on every input set of the GPU tests, so
    lags are compared exactly (a different summation order or Phi^-1 moves rho(t) by 1e-12 at most)."""
    st, mg = K.reference(name)
    print(name, "minimum margins", dict(zip(K.MARGINS, mg.min(axis=0))),
          "NaN counts", {s: int(c) for s, c in zip(K.STATS, np.isnan(st).sum(axis=0)) if c})
    assert mg.shape == (len(st), 4) and (mg.min(axis=0) >= 1e-6).all()
    assert np.isfinite(st[:, [K.HDI_LO, K.HDI_HI, K.MEDIAN]]).all()
    if not name.startswith(("golden:", "min:")):
        assert np.isfinite(st).all()
    if name.startswith("golden:"):  # z never changes (12 bi, 21 tri), z one half of the time (3 tri), constant indicators
        counts = {s: int(c) for s, c in zip(K.STATS, np.isnan(st).sum(axis=0))}
        want = dict(bi=dict(ess_bulk=12, rhat_folded=12, ess_q05=26, ess_q95=393, ess_sd=12),
                    tri=dict(ess_bulk=21, rhat_folded=24, ess_q05=30, ess_q95=396, ess_sd=24))[name.split(":")[1]]
        assert {s: counts[s] for s in want} == want

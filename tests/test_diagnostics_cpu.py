"""Convergence diagnostics without a GPU: the C ABI's declarations and argument checks, the host-only
helpers (summary_rhat, summarize_level2, extract_correlation), and the yardstick itself
(tests/diagnostics_ref.py) — its ESS and R-hat on AR(1) chains with a known answer, and the decision
margin that makes the exact comparison of the truncation lag in tests/test_gpu_diagnostics.py fair."""
from __future__ import annotations

import os

import numpy as np
import pandas as pd
import pytest

from tests import diagnostics_ref as R

NEW_SYMBOLS = ("clv_diagnostics", "clv_diagnostics_sampler", "clv_autocorr")


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
    for c in ("CLV_DIAG_MEAN = 0", "CLV_DIAG_SD", "CLV_DIAG_MCSE", "CLV_DIAG_ESS", "CLV_DIAG_RHAT", "CLV_DIAG_LAG",
              "CLV_N_DIAG_STATS"):
        assert c in text
    assert "#define CLV_ABI_VERSION 2" in text
    assert _lib.DIAG_STATS == R.STATS
    import mcmc_clv_model_amd as pkg
    for n in ("level1_diagnostics", "level2_diagnostics", "level2_autocorr", "summarize_level2",
              "extract_correlation", "summary_rhat"):
        assert n in pkg.__all__ and callable(getattr(pkg, n))


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    x = np.zeros((2, 16, 3))
    out = np.zeros((3, 6))
    acf = np.zeros((2, 3, 16))
    ok = dict(series=dptr(x), m=2, n=16, ns=3, period=1, out=dptr(out))

    def diag(**kw):
        a = dict(ok, **kw)
        return L.clv_diagnostics(0, a["series"], a["m"], a["n"], a["ns"], a["period"], 0, a["out"])

    for kw in (dict(series=None), dict(out=None), dict(m=0), dict(n=7), dict(ns=0), dict(period=0), dict(period=33)):
        assert diag(**kw) == -1, kw
        assert L.clv_last_error()

    def autocorr(series=dptr(x), m=2, n=16, ns=3, max_lag=5, out=dptr(acf)):
        return L.clv_autocorr(0, series, m, n, ns, max_lag, out)

    for kw in (dict(series=None), dict(out=None), dict(m=0), dict(n=7), dict(ns=0), dict(max_lag=-1), dict(max_lag=16)):
        assert autocorr(**kw) == -1, kw
    assert L.clv_diagnostics_sampler(None, 3, dptr(out), None) == -1


def test_python_argument_checks_need_no_device():
    from mcmc_clv_model_amd import analysis as A
    with pytest.raises(ValueError, match="draw_sink='full'"):
        A.level1_diagnostics({"level_1": None, "level_2": []})
    with pytest.raises(ValueError, match="log_columns"):
        A.level1_log_mask(("eta",), 4)
    assert A.level1_log_mask(("lambda", "mu"), 4) == 3 and A.level1_log_mask((), 5) == 0
    assert A.level1_log_mask(("eta", "mu"), 5) == 0b10010
    st = np.arange(2 * 4 * 6, dtype=float).reshape(8, 6)
    df = A.level1_diagnostics_frame(st, 2, 4, 3)
    assert list(df.columns[:6]) == [f"{s}_log_lambda" for s in R.STATS]
    assert list(df.columns[12:18]) == [f"{s}_tau" for s in R.STATS] and "rhat_z" in df and "ess_log_mu" in df
    assert df.shape == (2, 24) and df["lag_log_mu"].tolist() == [11.0, 35.0]
    assert list(A.level1_diagnostics_frame(st, 2, 4, 0).columns[:6]) == [f"{s}_lambda" for s in R.STATS]
    d2 = A.level2_diagnostics_frame(st[:5], ["a", "b", "c", "d", "e"])
    assert list(d2.columns) == list(R.STATS) and list(d2.index) == ["a", "b", "c", "d", "e"]
    with pytest.raises(ValueError):
        A.level2_diagnostics_frame(st[:5], ["a"])


def test_summary_rhat_matches_direct_computation():
    from mcmc_clv_model_amd.analysis import summary_rhat
    rng = np.random.default_rng(3)
    C, nd, n = 3, 50, 40
    lam = np.exp(rng.normal(-2.0, 0.4, (C, nd, n)))
    mu = np.exp(rng.normal(-4.0, 0.6, (C, nd, n)))
    lam[:, :, 5] = 0.25        # a constant series: variance not positive -> NaN
    mu[1] += 0.05              # a chain that sits elsewhere: R-hat well above 1
    sm = dict(n_draws=nd, **{"lambda": lam.mean(1), "lambda2": (lam * lam).mean(1), "mu": mu.mean(1),
                             "mu2": (mu * mu).mean(1)})
    got = summary_rhat({"level_1": None, "summary": sm})
    for nm, x in (("lambda", lam), ("mu", mu)):
        W = x.var(axis=1, ddof=1).mean(axis=0)
        B_n = x.mean(axis=1).var(axis=0, ddof=1)
        with np.errstate(invalid="ignore"):
            want = np.sqrt(((nd - 1) / nd * W + B_n) / W)
        keep = np.ones(n, bool)
        if nm == "lambda":
            keep[5] = False
            assert np.isnan(got["rhat_lambda"][5])
        # E[x^2] - E[x]^2 against the two-pass variance: cancellation leaves ~1e-12 here
        np.testing.assert_allclose(got[f"rhat_{nm}"][keep], want[keep], rtol=1e-10)
    assert (got["rhat_mu"] > 1.2).all() and (got["rhat_lambda"][np.arange(n) != 5] < 1.2).all()
    with pytest.raises(ValueError, match="2 chains"):
        summary_rhat({"summary": dict(sm, **{k: sm[k][:1] for k in ("lambda", "lambda2", "mu", "mu2")})})
    with pytest.raises(ValueError):
        summary_rhat({"level_1": [], "level_2": []})


def test_level2_ports_equal_the_reference_formulas():
    """summarize_level2 / extract_correlation (analysis_bi_helpers.py:6-13, 39-48) on level-2 arrays of
    the bivariate K = 1 and K = 2 layouts: numpy percentiles, bit for bit."""
    from mcmc_clv_model_amd.analysis import extract_correlation, summarize_level2
    rng = np.random.default_rng(5)
    for K in (1, 2):
        P = 2 * K + 3
        d = rng.normal(size=(60, P))
        d[:, -3] = np.exp(d[:, -3])
        d[:, -1] = np.exp(d[:, -1])
        d[:, -2] = 0.3 * np.sqrt(d[:, -3] * d[:, -1]) * np.tanh(d[:, -2])
        names = [f"p{i}" for i in range(P)]
        for dec in (2, 4):
            got = summarize_level2(d, names, decimals=dec)
            q = np.percentile(d, [2.5, 50, 97.5], axis=0)
            want = pd.DataFrame(q.T, columns=["2.5%", "50%", "97.5%"], index=names).round(dec)
            pd.testing.assert_frame_equal(got, want, check_exact=True)
        corr = d[:, -2] / np.sqrt(d[:, -3] * d[:, -1])
        np.testing.assert_array_equal(extract_correlation(d), np.percentile(corr, [2.5, 50, 97.5]).round(2))


def test_yardstick_on_ar1_with_known_answer():
    """AR(1) at phi = 0.5: ESS / N -> (1 - phi) / (1 + phi) = 1/3 (mean over 200 replicates of 4 x 1000
    within 5 %); with chain 4 shifted by +1.0 every R-hat is above 1.05."""
    rng = np.random.default_rng(2024)
    ratio, rh = [], []
    for _ in range(200):
        y = R.ar1(rng, 4, 1000, 0.5)
        st, _ = R.series_stats(y)
        ratio.append(st[3] / 4000.0)
        y[3] += 1.0
        rh.append(R.series_stats(y)[0][4])
    print("mean ESS/N", np.mean(ratio), "R-hat range", min(rh), max(rh))
    assert abs(np.mean(ratio) - 1.0 / 3.0) < 0.05 / 3.0
    assert min(rh) > 1.05


def test_yardstick_edge_cases():
    y = R.ar1(1, 2, 20, 0.3)
    st, _ = R.series_stats(y)
    assert np.isfinite(st).all()
    bad = y.copy()
    bad[1, 3] = np.inf
    assert np.isnan(R.series_stats(bad)[0]).all()
    assert np.isnan(R.series_stats(np.ones((2, 20)))[0]).all()       # W == 0
    assert np.isnan(R.series_stats(-np.abs(y), log=True)[0]).all()  # log of a negative value
    np.testing.assert_allclose(R.series_stats(np.exp(y), log=True)[0], st, rtol=1e-9)
    # n = 8: h = 4, the loop never runs: lag -1, tau at its floor 1 / log10(M h)
    s8, _ = R.series_stats(R.ar1(2, 2, 8, 0.0))
    assert s8[5] == -1 and s8[3] == pytest.approx(16 * np.log10(16))
    a = R.autocorr(y, 5)
    assert a.shape == (2, 6) and (a[:, 0] == 1).all()


@pytest.mark.parametrize("name", [f"small:{m}:{n}" for m, n in R.SMALL_SHAPES] + [f"min:{m}:{n}" for m, n in R.MIN_SHAPES]
                         + ["long", "golden:bi", "golden:tri"])
def test_decision_margin_allows_the_exact_lag_comparison(name):
    """Every comparison against zero in Geyer's truncation is at least 1e-6 from going the other way on
    every input set of the GPU tests — far beyond the 1e-13 a different summation order can move rho(t)
    — so the truncation lag is compared exactly."""
    if name.startswith("golden:"):
        _, _, _, st, mg = R.golden_level1(name.split(":")[1])
        assert int(np.isnan(st[:, 0]).sum()) == {"bi": 12, "tri": 21}[name.split(":")[1]]
    else:
        st, mg = R.reference(name)
        assert np.isfinite(st).all()
    print(name, "minimum margin", mg.min())
    assert mg.min() >= 1e-6

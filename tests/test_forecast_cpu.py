"""The closed-form holdout forecast without a device: the C ABI's declarations and argument checks,
the validation of the Python layer, the float64 model (tests/forecast_ref.py) against 40-digit
mpmath, the identities the definitions imply (in mpmath, on a grid that includes lambda t = 780 with
mu t = 0.04 and log lambda = +-70), and the host frames.

The model's own error against mpmath on the 64-draw x 100-customer fixture, k_max 64 (measured here,
printed before the assertion, recorded in forecast_ref.E_PMF / E_STAT with the procedure):
  E_PMF   2.91e-14 -> 3e-14     E_STAT   2.27e-15 -> 3e-15 (relative for xstar_mean and p_alive, relative to max(|value|, 1)
  for log_score and rps: forecast_ref's docstring says why)."""
import ctypes
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import forecast_ref as R

NEW_SYMBOLS = ("clv_forecast", "clv_forecast_sampler", "clv_forecast_info", "clv_debug_forecast")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clvmcmc.h")
T = 39.0


def test_header_declares_and_library_exports_the_new_symbols():
    from mcmc_clv_model_amd import _lib
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    with open(HDR) as f:
        text = f.read()
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2   # additions only: no bump


def test_enum_order_and_limits():
    from mcmc_clv_model_amd import _lib
    with open(HDR) as f:
        text = " ".join(f.read().split())
    cols = re.search(r"enum \{ (CLV_FC_XSTAR_MEAN = 0,[^}]*?CLV_N_FC_STATS) \}", text).group(1)
    names = [t.strip().split(" ")[0] for t in cols.split(",")]
    assert names == ["CLV_FC_" + c.upper() for c in _lib.FC_STATS] + ["CLV_N_FC_STATS"]
    assert _lib.FC_STATS == R.STATS and len(_lib.FC_STATS) == 11
    info = _lib.forecast_info()
    assert info == dict(block=_lib.FC_BLOCK, max_k=_lib.FC_MAX_K, max_draws=_lib.FC_MAX_DRAWS,
                        series_cap=_lib.FC_SERIES_CAP, batch_doubles=_lib.FC_BATCH_DOUBLES)
    assert info["block"] == 256 == _lib.BLOCK and info["max_k"] == 4096 and info["series_cap"] == R.SER_CAP
    assert info["max_draws"] >= 4000


# ---- the C ABI's argument checks: -1 before any device call ---------------------------------------
def _c_args(S=4, N=3, width=4, K=8):
    from mcmc_clv_model_amd._lib import dptr
    l1, d = R.synth_case(S, N, width, seed=2)
    xs = np.array([0, K - 1, 2], np.int32)
    out, pmf = np.empty(N * 11), np.empty(N * K)
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    keep = (l1, d, xs, out, pmf)
    return keep, dict(level1=dptr(l1), n_draws=S, n=N, width=width, x=i32(d["x"]), t_x=dptr(d["t_x"]),
                      T_cal=dptr(d["T_cal"]), T_star=T, k_max=K, x_star=i32(xs), out=dptr(out), out_pmf=dptr(pmf))


ORDER = ("level1", "n_draws", "n", "width", "x", "t_x", "T_cal", "T_star", "k_max", "x_star")
BAD = [dict(level1=None), dict(x=None), dict(t_x=None), dict(T_cal=None), dict(out=None),
       dict(n_draws=0), dict(n_draws=-1), dict(n=0), dict(n=-1), dict(width=3), dict(width=6),
       dict(T_star=0.0), dict(T_star=-1.0), dict(T_star=float("inf")), dict(T_star=float("nan")),
       dict(k_max=0), dict(k_max=-1), dict(k_max=4097),
       dict(k_max=7),                                     # x_star[1] = 7 is outside [0, 7)
       dict(x_star=np.array([0, -1, 2], np.int32)), dict(x_star=np.array([0, 1, 8], np.int32))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_c_abi_rejects_bad_arguments(bad):
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    keep, a = _c_args()
    bad = dict(bad)
    if isinstance(bad.get("x_star"), np.ndarray):
        keep = keep + (bad["x_star"],)
        bad["x_star"] = bad["x_star"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    a.update(bad)
    head = [0] + [a[k] for k in ORDER]
    assert L.clv_forecast(*head, a["out"], a["out_pmf"]) == -1
    assert L.clv_last_error()
    assert L.clv_debug_forecast(*head, 0, 0, a["out"], a["out_pmf"]) == -1


def test_c_abi_rejects_the_rest():
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    keep, a = _c_args()
    head = [0] + [a[k] for k in ORDER]
    assert L.clv_forecast_info(None) == -1
    assert L.clv_debug_forecast(*head, -1, 0, a["out"], a["out_pmf"]) == -1
    assert L.clv_debug_forecast(*head, 0, -1, a["out"], a["out_pmf"]) == -1
    assert L.clv_forecast_sampler(None, T, 8, None, a["out"], None) == -1


# ---- the Python layer ------------------------------------------------------------------------------
def _py_case(width=4, S=8, N=3):
    l1, d = R.synth_case(S, N, width, seed=2)
    cbs = pd.DataFrame(d)
    cbs["x_star"] = [0, 3, 70]
    return {"level_1": [l1[:S // 2], l1[S // 2:]]}, cbs


@pytest.mark.parametrize("kw", [
    dict(T_star=0.0), dict(T_star=-2.0), dict(T_star=float("nan")), dict(T_star=float("inf")),
    dict(k_max=0), dict(k_max=4097), dict(k_max=2.5), dict(x_star="x_star", k_max=64),   # 70 >= 64
    dict(x_star="no_such_column"), dict(x_star=[0, 1]), dict(x_star=[0, -1, 2]), dict(x_star=[0, 1.5, 2]),
    dict(x_star=[0, 1, 5000])], ids=str)
def test_forecast_validates_before_any_device_call(kw):
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case()
    with pytest.raises(ValueError):
        A.forecast(draws, cbs, **kw)


def test_forecast_rejects_mismatched_cbs():
    from mcmc_clv_model_amd import analysis as A
    draws, cbs = _py_case()
    with pytest.raises(ValueError):
        A.forecast(draws, cbs.iloc[:2])


def test_k_max_default():
    from mcmc_clv_model_amd import analysis as A
    f = A.forecast_params
    assert f()["k_max"] == 64 and f(x_star=[0, 63])["k_max"] == 64 and f(x_star=[64])["k_max"] == 128
    assert f(x_star=[127])["k_max"] == 128 and f(x_star=[128])["k_max"] == 192 and f(x_star=[4095])["k_max"] == 4096
    assert f(x_star=[0, 63])["k_max"] == R.default_k_max([0, 63]) and R.default_k_max([200]) == f(x_star=[200])["k_max"]
    draws, cbs = _py_case()
    par = f(39.0, "x_star", None, False, cbs, 3)
    assert par["k_max"] == 128 and par["x_star"].dtype == np.int32 and list(par["x_star"]) == [0, 3, 70]
    with pytest.raises(ValueError):
        f(x_star=[4096])


def test_fit_keyword_is_validated_before_the_run():
    from mcmc_clv_model_amd.sampler import forecast_kwargs
    draws, cbs = _py_case()
    assert forecast_kwargs(None, "full") is None and forecast_kwargs(False, "summary") is None
    assert forecast_kwargs(True, "full") == {}
    kw = forecast_kwargs(dict(x_star="x_star", T_star=20.0), "full", cbs, 3)
    assert list(kw["x_star"]) == [0, 3, 70] and kw["T_star"] == 20.0
    for bad, sink in ((True, "summary"), (dict(horizon=3), "full"), (3, "full"), (dict(T_star=-1.0), "full"),
                      (dict(x_star="x_star"), "full"), (dict(k_max=9999), "full")):
        with pytest.raises(ValueError):
            forecast_kwargs(bad, sink)


# ---- the model against mpmath ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_refs():
    """The 64 x 100 fixture in mpmath, with and without the extreme draws (lambda and mu do not depend
    on the width, so both widths share it)."""
    out = {}
    for ext in (False, True):
        l1, d = R.synth_case(64, 100, 4, 11, extremes=ext)
        xs = R.holdout_counts(100, 11)
        out[ext] = R.mp_reference(l1, d, T, 64, xs)
    R.mp_draw.cache_clear()
    return out


@pytest.mark.parametrize("width", [4, 5])
@pytest.mark.parametrize("ext", [False, True])
def test_model_against_mpmath(cpu_refs, width, ext):
    l1, d = R.synth_case(64, 100, width, 11, extremes=ext)
    xs = R.holdout_counts(100, 11)
    st, pmf = R.model(l1, d, T, 64, xs)
    mst, mpmf, _ = cpu_refs[ext]
    col = R.STATS.index
    e_pmf = R.rel_err(pmf, mpmf, R.PMF_FLOOR)
    e_rel = max(R.rel_err(st[:, col(c)], mst[:, col(c)]) for c in ("xstar_mean", "p_alive"))
    e_mix = max(R.mixed_err(st[:, col(c)], mst[:, col(c)]) for c in ("log_score", "rps"))
    print(f"width {width} extremes {ext}: E_PMF {e_pmf:.3g}  E_STAT relative {e_rel:.3g} mixed {e_mix:.3g}")
    assert e_pmf <= R.E_PMF
    assert max(e_rel, e_mix) <= R.E_STAT
    # the rest: the quantiles exactly, the cumulative columns to the roundings of k_max additions
    for c in ("q05", "q50", "q95"):
        assert np.array_equal(st[:, col(c)], mst[:, col(c)])
    for c in ("p_zero", "pit_lo", "pit_hi", "tail_mass"):
        assert R.mixed_err(st[:, col(c)], mst[:, col(c)]) <= 64 * 2.0 ** -53 + R.E_PMF
    assert (mpmf >= R.PMF_FLOOR).sum() > 0.9 * mpmf.size


def test_model_without_x_star_and_with_a_bad_draw():
    l1, d = R.synth_case(8, 5, 4, 3)
    xs = R.holdout_counts(5, 3)
    a, pa = R.model(l1, d, T, 64, xs)
    b, pb = R.model(l1, d, T, 64, None)
    assert np.array_equal(a[:, :7], b[:, :7]) and np.isnan(b[:, 7:]).all() and np.array_equal(pa, pb)
    l1[3, 2, 0] = np.nan
    l1[5, 4, 1] = np.inf
    c, pc = R.model(l1, d, T, 64, xs)
    assert np.isnan(c[[2, 4]]).all() and np.isnan(pc[[2, 4]]).all()
    assert np.array_equal(c[[0, 1, 3]], a[[0, 1, 3]])


def test_margin_inputs_are_the_gpu_fixtures():
    """The exponent arguments forecast_ref's DEVICE_MARGIN is derived from."""
    for ext in (False, True):
        l1, d, xs = R.gpu_case(4, ext)
        lam, mu = l1[..., 0], l1[..., 1]
        a, y = lam * R.GPU_T, (lam + mu) * R.GPU_T
        live = y < 700.0                     # exp(-y) underflows in the rest: their g is 0
        m = np.floor(a[live])
        assert (m * np.abs(np.log(a[live]))).max() <= R.GPU_MAX_MLOGA
        assert max(math.lgamma(v + 1.0) for v in m) <= R.GPU_MAX_LGAMMA
        assert y[live].max() <= R.GPU_MAX_Y
        with np.errstate(all="ignore"):
            lv = np.log(mu / (lam + mu)) + 127.0 * -np.log1p(mu / lam)
        assert not (y > 1e4).any() or np.abs(lv[y > 1e4]).max() <= 141.0
        assert xs.max() < 64 and xs[0] == 0 and xs[1] == 63
    dev = (R.GPU_MAX_MLOGA + 4.0 * R.GPU_MAX_LGAMMA + 1.0) * 2.0 ** -53
    assert 1.0 + dev / R.E_PMF <= R.DEVICE_MARGIN


def test_golden_rows_are_what_mpmath_gives():
    g = np.load(R.GOLDEN)
    l1, d, xs = R.gpu_case(4, True)
    rows = [0, 1, 257]
    for K in (64, 128):
        st, pm, _ = R.mp_reference(l1, d, R.GPU_T, K, xs, customers=rows)
        # to one rounding to float64 (the order of the 40-digit additions may differ); tail_mass = 1 - F
        # carries the 40-digit sum's own rounding, 1e-39 absolute
        assert np.allclose(pm, g["pmf_x1"][rows, :K], rtol=2.0 ** -52, atol=0.0)
        assert np.allclose(st, g[f"stats{K}_x1"][rows], rtol=2.0 ** -52, atol=1e-30, equal_nan=True)
    R.mp_draw.cache_clear()


# ---- identities, in mpmath -------------------------------------------------------------------------
GRID = [(780.0 / T, 0.04 / T, 1024), (780.0 / T, 0.04 / T, 64), (math.exp(70.0), 0.03, 64),
        (math.exp(-70.0), 0.03, 64), (math.exp(70.0), math.exp(-70.0), 64), (math.exp(-70.0), math.exp(5.0), 64),
        (0.08, 0.03, 64), (0.08, 0.03, 256), (0.5, 15.0, 128), (1.6, 0.002, 200),
        (0.05, 25.0, 64), (0.02, 4.0, 64), (0.02, 5.0, 64), (2.0, 120.0, 4096)]   # mu t large: either side of closed branch 1


@pytest.mark.parametrize("lam,mu,K", GRID, ids=lambda v: f"{v:.3g}")
def test_identities_in_mpmath(lam, mu, K):
    mp = R._mp()
    pm = R.mp_pmf_alive(lam, mu, T, K)
    L, M = mp.mpf(lam), mp.mpf(mu)
    ml = L + M
    y, r, w = ml * T, L / ml, M / ml
    # sum_k pmf + tail = 1: K purchases before min(death, t) is r^K P(K, y)
    tail = r ** K * mp.gammainc(K, 0, y, regularized=True)
    assert abs(mp.fsum(pm) + tail - 1) < mp.mpf(10) ** -30
    # pmf(0) against its closed form
    p0 = mp.exp(-y) + w * (1 - mp.exp(-y))
    assert abs(pm[0] - p0) <= mp.mpf(10) ** -35 * p0
    # the recurrence against one gammainc per value
    for k in sorted({0, 1, K // 3, K - 2, K - 1}):
        ref = R.mp_pmf_alive_direct(lam, mu, T, k)
        assert abs(pm[k] - ref) <= mp.mpf(10) ** -28 * ref + mp.mpf(10) ** -1000
    # sum_k k pmf -> mean as k_max grows: rises with K, never above, and reaches the mean once K is
    # far above lambda t
    mean = (L / M) * (-mp.expm1(-M * T))
    part = [mp.fsum(k * pm[k] for k in range(n)) for n in (K // 2, K)]
    assert part[0] <= part[1] <= mean * (1 + mp.mpf(10) ** -30)
    if lam * T + 12 * math.sqrt(lam * T) + 40 < K:
        assert abs(part[1] - mean) < mp.mpf(10) ** -9 * mean


@pytest.mark.parametrize("lam,mu,K", GRID + [(100.0, 1e-3, 4096), (1.0, 0.02, 4096), (104.0, 1.0, 4096)],
                         ids=lambda v: f"{v:.3g}")
def test_model_on_the_grid(lam, mu, K):
    """The model's branches (the mode start where exp(-y) underflows, both closed branches, the long
    series) against mpmath.  The bound: the recurrence's E_PMF (K / 64) plus 2 ulp in each term of the
    start's exponent (m log a, lgamma(m + 1), y) — numpy's and libm's functions."""
    pmf, pa, mean = R.draw_pmf(np.array([lam]), np.array([mu]), np.array([0.0]), T, K)
    ref = np.array([float(v) for v in R.mp_pmf_alive(lam, mu, T, K)])
    a = lam * T
    m = min(math.floor(a), K - 1)
    X = m * abs(math.log(a)) + math.lgamma(m + 1.0) + (lam + mu) * T if (lam + mu) * T < 1e4 else 80.0
    tol = R.E_PMF * (K / 64.0) + 2.0 * X * 2.0 ** -53
    assert pa[0] == 1.0
    assert R.rel_err(pmf[0], ref, R.PMF_FLOOR) <= tol
    assert np.all(pmf[0][ref < 1e-300] < 1e-290)


# ---- the host frames -------------------------------------------------------------------------------
def _frames(seed=0, N=600, K=64, shift=0.0):
    from mcmc_clv_model_amd import analysis as A
    l1, d = R.synth_case(6, N, 4, seed)
    l1[..., 0] *= math.exp(shift)
    xs = R.holdout_counts(N, seed)
    st, pmf = R.model(l1, d, T, K, xs)
    return A.forecast_frames(st, pmf, 6, True), st, pmf, xs, d


def test_scores_totals_and_frequency():
    from mcmc_clv_model_amd import analysis as A
    fc, st, pmf, xs, d = _frames()
    col = R.STATS.index
    sc = fc["scores"].iloc[0]
    ls = st[:, col("log_score")]
    assert sc["log_score"] == A.fixed_order_sum(ls) and abs(sc["log_score"] - math.fsum(ls)) <= 1e-12 * abs(math.fsum(ls))
    assert abs(sc["se"] - math.sqrt(len(ls) * ls.var())) <= 1e-12 * sc["se"]
    assert abs(sc["rps"] - st[:, col("rps")].mean()) <= 1e-12 * sc["rps"]
    cover = np.mean((st[:, col("q05")] <= xs) & (xs <= st[:, col("q95")]))
    assert abs(sc["coverage_90"] - cover) < 1e-12
    assert sc["n_data_points"] == 600 and sc["n_samples"] == 6
    fr = fc["frequency"]
    assert len(fr) == 65 and fr.index[-1] == ">=64"
    assert np.allclose(fr.to_numpy()[:64], pmf.sum(axis=0), rtol=1e-12)
    assert abs(fr.sum() - 600.0) < 1e-9                         # every customer is somewhere
    none = A.forecast_frames(st, None, 6, False)
    assert none["frequency"] is None and none["pmf"] is None and np.isnan(none["scores"].iloc[0]["log_score"])


def test_compare_forecasts_order_and_dse():
    from mcmc_clv_model_amd import analysis as A
    good, st_g, _, _, _ = _frames()
    poor, st_p, _, _, _ = _frames(shift=1.0)                    # lambda inflated e-fold
    t = A.compare_forecasts({"poor": poor, "good": good})
    assert list(t.index) == ["good", "poor"] and list(t["rank"]) == [0, 1]
    col = R.STATS.index("log_score")
    diff = st_g[:, col] - st_p[:, col]
    assert t.loc["good", "diff"] == 0.0 and t.loc["good", "dse"] == 0.0
    assert abs(t.loc["poor", "diff"] - diff.sum()) <= 1e-10 * abs(diff.sum())
    assert abs(t.loc["poor", "dse"] - math.sqrt(len(diff) * diff.var())) <= 1e-12 * t.loc["poor", "dse"]
    with pytest.raises(ValueError):
        A.compare_forecasts({})
    with pytest.raises(ValueError):
        A.compare_forecasts({"a": good, "b": A.forecast_frames(st_g[:5], None, 6, True)})


def test_forecast_pit_bins_sum_to_n():
    from mcmc_clv_model_amd import analysis as A
    fc, st, _, _, _ = _frames()
    for bins in (1, 10, 7):
        h = A.forecast_pit(fc, bins=bins, seed=3)
        assert len(h) == bins and int(h.sum()) == 600
    assert A.forecast_pit(fc, seed=3).equals(A.forecast_pit(fc, seed=3))
    unscored = st.copy()
    unscored[:, 7:] = np.nan                                    # what the device returns without x_star
    with pytest.raises(ValueError):
        A.forecast_pit(A.forecast_frames(unscored, None, 6, False))
    with pytest.raises(ValueError):
        A.forecast_pit(fc, bins=0)


def test_forecast_table_against_numpy():
    from mcmc_clv_model_amd import analysis as A
    x = np.array([0, 0, 1, 2, 7, 9, 12, 3, 1, 0])
    act = np.array([0, 1, 2, 1, 9, 6, 14, 2, 0, 0], float)
    pred = np.array([0.2, 0.3, 1.1, 1.9, 6.5, 7.0, 10.0, 2.5, 0.9, 0.1])
    fc = dict(pointwise=pd.DataFrame(dict(xstar_mean=pred)))
    tb = A.forecast_table(fc, pd.DataFrame(dict(x=x, x_star=act)))
    m = tb["metrics"].iloc[0]
    assert abs(m["correlation"] - np.corrcoef(act, pred)[0, 1]) < 1e-15 and abs(m["mse"] - np.mean((act - pred) ** 2)) < 1e-15
    by = tb["by_frequency"]
    assert list(by.index) == ["0", "1", "2", "3", "7+"]
    assert list(by["n"]) == [3, 2, 1, 1, 3]
    assert abs(by.loc["7+", "actual"] - (9 + 6 + 14) / 3) < 1e-15 and abs(by.loc["7+", "predicted"] - 23.5 / 3) < 1e-15
    assert abs(by.loc["0", "predicted"] - 0.2) < 1e-15 and by.loc["1", "actual"] == 1.0
    with pytest.raises(ValueError):
        A.forecast_table(fc, pd.DataFrame(dict(x=x)))

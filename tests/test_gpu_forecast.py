"""The closed-form holdout forecast on the GPU (csrc/forecast.hip) against 40-digit mpmath, through
the Python API and the debug ABI only.

The reference of the S = 100 x N = 300 case (one full 256-customer block and a partial one) is
tests/golden/forecast_mp_S100_N300.npz: forecast_ref.mp_gpu_reference rounded to float64 (two minutes
of mpmath; tests/test_forecast_cpu.py recomputes a sample of its rows).  The tolerances are
forecast_ref.pmf_tol / stat_tol: the model's measured error E_PMF / E_STAT, scaled with the steps of
the recurrence, times a margin derived from the documented ulp bounds of the device's exp, log and
lgamma at the fixture's largest exponent argument (forecast_ref's docstring).  Every figure is printed
before it is asserted."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from tests import forecast_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu
col = R.STATS.index
T = R.GPU_T


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(R.GOLDEN)
    return {k: g[k] for k in g.files}


def as_draws(l1):
    h = l1.shape[0] // 2
    return {"level_1": [l1[:h], l1[h:]]} if h else {"level_1": [l1]}


def c_forecast(l1, d, K, xs=None, pmf=True, debug=None):
    """clv_forecast (debug: (batch_customers, grid) through clv_debug_forecast): (out, pmf or None)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    l1 = np.ascontiguousarray(l1)
    S, N, w = l1.shape
    i32 = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out = np.full((N, 11), -7.0)
    dist = np.full((N, K), -7.0) if pmf else None
    head = (0, dptr(l1), S, N, w, i32(d["x"]), dptr(d["t_x"]), dptr(d["T_cal"]), T, K, i32(xs))
    if debug is None:
        _lib.check(L.clv_forecast(*head, dptr(out), dptr(dist)))
    else:
        _lib.check(L.clv_debug_forecast(*head, debug[0], debug[1], dptr(out), dptr(dist)))
    return out, dist


@pytest.mark.parametrize("with_xs", [True, False], ids=["xstar", "noxstar"])
@pytest.mark.parametrize("ext", [False, True], ids=["moderate", "extremes"])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("width", [4, 5])
def test_device_against_mpmath(width, K, ext, with_xs):
    from mcmc_clv_model_amd import analysis as A
    l1, d, xs = R.gpu_case(width, ext)
    g = golden()
    want_pmf, want = g[f"pmf_x{int(ext)}"][:, :K], g[f"stats{K}_x{int(ext)}"].copy()
    fc = A.forecast(as_draws(l1), pd.DataFrame(d), T, x_star=xs if with_xs else None, k_max=K, pmf=True)
    st, pmf = fc["pointwise"].to_numpy(), fc["pmf"]
    assert st.shape == (R.GPU_N, 11) and pmf.shape == (R.GPU_N, K) and list(fc["pointwise"].columns) == list(R.STATS)
    if not with_xs:
        assert np.isnan(st[:, 7:]).all()
        want[:, 7:] = np.nan
    e_pmf = R.rel_err(pmf, want_pmf, R.PMF_FLOOR)
    e_rel = max(R.rel_err(st[:, col(c)], want[:, col(c)]) for c in ("xstar_mean", "p_alive"))
    e_ls = R.mixed_err(st[:, col("log_score")], want[:, col("log_score")])
    e_rps = R.mixed_err(st[:, col("rps")], want[:, col("rps")])
    e_cum = max(R.mixed_err(st[:, col(c)], want[:, col(c)]) for c in ("p_zero", "pit_lo", "pit_hi", "tail_mass"))
    print(f"width {width} k_max {K} extremes {ext}: pmf {e_pmf:.3g} (tol {R.pmf_tol(K):.3g})  mean/p_alive {e_rel:.3g} "
          f"rps {e_rps:.3g} (tol {R.stat_tol(K):.3g})  log_score {e_ls:.3g}  cumulative {e_cum:.3g}")
    assert e_pmf <= R.pmf_tol(K)
    assert max(e_rel, e_rps) <= R.stat_tol(K)
    assert e_ls <= R.pmf_tol(K)
    # the cumulative columns: k_max additions' roundings and the pmf's own error
    assert e_cum <= K * 2.0 ** -53 + R.pmf_tol(K)
    for c in ("q05", "q50", "q95"):
        assert np.array_equal(st[:, col(c)], want[:, col(c)]), c
    assert np.all(pmf[want_pmf < 1e-300] < R.PMF_FLOOR)
    # the frames
    fr = fc["frequency"]
    assert len(fr) == K + 1 and abs(fr.sum() - R.GPU_N) < 1e-9
    sc = fc["scores"].iloc[0]
    assert sc["n_samples"] == R.GPU_S and sc["n_data_points"] == R.GPU_N
    assert np.isfinite(sc["log_score"]) == with_xs


@pytest.mark.parametrize("K", [64, 100])
def test_geometry_batch_and_null_pmf_give_the_same_bits(K):
    l1, d, xs = R.gpu_case(4, True)
    out, pmf = c_forecast(l1, d, K, xs)
    assert not (out == -7.0).any() and not (pmf == -7.0).any()
    o2, p2 = c_forecast(l1, d, K, xs, debug=(256, 1))
    assert np.array_equal(bits(out), bits(o2)) and np.array_equal(bits(pmf), bits(p2))
    o3, p3 = c_forecast(l1, d, K, xs, debug=(1, 2))             # rounded up to one block per batch
    assert np.array_equal(bits(out), bits(o3)) and np.array_equal(bits(pmf), bits(p3))
    o4, none = c_forecast(l1, d, K, xs, pmf=False)
    assert none is None and np.array_equal(bits(out), bits(o4))
    # a customer's result does not depend on the others: the second block alone
    sub = {k: np.ascontiguousarray(v[256:]) for k, v in d.items()}
    o5, p5 = c_forecast(l1[:, 256:], sub, K, xs[256:])
    assert np.array_equal(bits(out[256:]), bits(o5)) and np.array_equal(bits(pmf[256:]), bits(p5))


def test_one_customer_one_draw():
    l1, d, xs = R.gpu_case(5, False)
    one = {k: np.ascontiguousarray(v[7:8]) for k, v in d.items()}
    out, pmf = c_forecast(l1[3:4, 7:8], one, 64, xs[7:8])
    want, want_pmf, _ = R.mp_reference(l1[3:4], d, T, 64, xs, customers=[7])
    R.mp_draw.cache_clear()
    e_pmf, e_st = R.rel_err(pmf, want_pmf, R.PMF_FLOOR), R.mixed_err(out[:, [0, 1, 7, 10]], want[:, [0, 1, 7, 10]])
    print(f"N = 1, S = 1: pmf {e_pmf:.3g}  statistics {e_st:.3g}")
    assert e_pmf <= R.pmf_tol(64) and e_st <= R.pmf_tol(64)
    assert np.array_equal(out[:, 3:6], want[:, 3:6])


def test_extreme_only_input_finishes_with_all_mass_in_the_tail():
    """Every draw at log lambda = 70: the closed branch, no loop over the draw's value."""
    l1, d, xs = R.gpu_case(4, False)
    l1 = l1[:8].copy()
    l1[..., 0] = np.exp(70.0)
    d = dict(d, t_x=d["T_cal"].copy())                           # alive for certain: p_alive = 1
    for K in (4096, 64):
        out, pmf = c_forecast(l1, d, K, None)
        assert np.array_equal(out[:, col("tail_mass")], np.ones(R.GPU_N))
        assert np.array_equal(out[:, col("p_alive")], np.ones(R.GPU_N))
        assert np.array_equal(out[:, col("q50")], np.full(R.GPU_N, float(K)))
        assert np.all((pmf > 0) & (pmf < 1e-28))                 # w r^k: the customer died first
    st, mpmf = R.model(l1, d, T, 64, None)
    assert R.rel_err(pmf, mpmf, R.PMF_FLOOR) <= R.pmf_tol(64)


def test_nan_draw_marks_the_customer():
    l1, d, xs = R.gpu_case(4, False)
    l1 = l1[:10].copy()
    clean, clean_pmf = c_forecast(l1, d, 64, xs)
    l1[4, 5, 0] = np.nan
    l1[9, 299, 1] = np.inf
    l1[0, 17, 0] = -1.0
    out, pmf = c_forecast(l1, d, 64, xs)
    bad = [5, 17, 299]
    assert np.isnan(out[bad]).all() and np.isnan(pmf[bad]).all()
    keep = np.setdiff1d(np.arange(R.GPU_N), bad)
    assert np.array_equal(bits(out[keep]), bits(clean[keep])) and np.array_equal(bits(pmf[keep]), bits(clean_pmf[keep]))


def test_long_horizon_and_large_k_max():
    """lambda t near 800 (exp(-y) underflows: the log-domain start at the mode) and k_max = 1024 against
    the model, whose own error there tests/test_forecast_cpu.py bounds against mpmath."""
    l1, d, xs = R.gpu_case(4, False)
    l1, d = l1[:4, :40].copy(), {k: np.ascontiguousarray(v[:40]) for k, v in d.items()}
    l1[..., 0] = np.linspace(15.0, 25.0, 40)
    l1[..., 1] = 0.04 / T
    out, pmf = c_forecast(l1, d, 1024, None)
    st, mpmf = R.model(l1, d, T, 1024, None)
    # device and model share the recurrence's roundings and differ by their functions in the start's
    # exponent: log (1 + 1 ulp) on m log a, lgamma (4 + 1 ulp) on lgamma(m + 1) < m log a, exp (1 + 1 ulp)
    # on the sum, whose size is below y
    a = l1[..., 0].max() * T
    tol = (2.0 * a * np.log(a) + 5.0 * a * np.log(a) + 2.0 * a) * 2.0 ** -53
    e = R.rel_err(pmf, mpmf, R.PMF_FLOOR)
    print(f"lambda t up to {a:.0f}, k_max 1024: device against the model {e:.3g} (tol {tol:.3g})")
    assert e <= tol and abs(pmf.sum(axis=1) + out[:, col("tail_mass")] - 1.0).max() < 1e-11


def test_almost_surely_dead_customers():
    """mu t from 80 to 1,200 at k_max 64, either side of closed branch 1 (y - K - K log(y / K) = 45 at
    y = 172), t_x = T_cal so that p_alive = 1 and the values count: against mpmath.  The start's exponent
    is at most y there (m = 0 or 1), so the margin's inputs cover y <= 62 only in part: the bound adds
    (1 + 1) ulp of y for exp and of log w + 63 log r <= 63 log(ml / lambda) for closed branch 1."""
    l1, d, xs = R.gpu_case(4, False)
    n = 48
    l1, d = l1[:2, :n].copy(), {k: np.ascontiguousarray(v[:n]) for k, v in d.items()}
    d["t_x"] = d["T_cal"].copy()
    l1[0, :, 0], l1[1, :, 0] = 0.02, 0.3
    l1[..., 1] = np.geomspace(80.0, 1200.0, n) / T
    out, pmf = c_forecast(l1, d, 64, xs[:n])
    want, want_pmf, _ = R.mp_reference(l1, d, T, 64, xs[:n])
    R.mp_draw.cache_clear()
    big = 63.0 * np.log((l1[..., 0] + l1[..., 1]).max() / 0.02) + 1200.0
    tol = R.pmf_tol(64) + 2.0 * big * 2.0 ** -53
    e = R.rel_err(pmf, want_pmf, R.PMF_FLOOR)
    print(f"mu t 80 ... 1200: pmf {e:.3g} (tol {tol:.3g})")
    assert np.isfinite(out).all() and np.isfinite(pmf).all()
    assert e <= tol and np.array_equal(out[:, 3:6], want[:, 3:6])
    assert R.mixed_err(out[:, [0, 1, 7, 10]], want[:, [0, 1, 7, 10]]) <= tol


RUN = dict(mcmc=100, burnin=20, thin=2, chains=2, seed=5)


def frames_equal(a, b):
    for k in ("pointwise", "scores"):
        assert list(a[k].columns) == list(b[k].columns)
        assert np.array_equal(bits(a[k].to_numpy(dtype=np.float64)), bits(b[k].to_numpy(dtype=np.float64))), k
    assert np.array_equal(bits(a["frequency"].to_numpy()), bits(b["frequency"].to_numpy()))
    assert np.array_equal(bits(a["pmf"]), bits(b["pmf"]))


def test_sampler_path_and_drop_in():
    from mcmc_clv_model_amd import _lib, mcmc_draw_parameters
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", n=553)
    df["x_star"] = R.holdout_counts(553, 9)
    covs = ["first_sales_scaled"]
    p = build_problem(df, covs, D=2)
    kw = dict(T_star=39.0, x_star="x_star", pmf=True)
    with HipSampler(p, n_mh_steps=20, **RUN) as s:
        with pytest.raises(_lib.ClvError, match="-3"):          # CLV_ESTATE: the run has not stored its draws
            s.forecast()
        s.run(120)
        dev = s.forecast(39.0, x_star=df["x_star"].to_numpy(), pmf=True)
        plain = s.forecast()
        l1, l2, _ = s.read_draws()
    assert l1.shape[:3] == (2, 50, 553)
    draws = dict(level_1=list(l1), level_2=list(l2))
    host = A.forecast(draws, df, **kw)
    frames_equal(dev, host)
    assert dev["pointwise"].shape == (553, 11) and np.isfinite(dev["pointwise"].to_numpy()).all()
    assert dev["scores"].iloc[0]["n_samples"] == 100 and dev["pmf"].shape == (553, 64)
    assert plain["pmf"] is None and plain["frequency"] is None
    assert np.array_equal(bits(plain["pointwise"].to_numpy()[:, :7]), bits(dev["pointwise"].to_numpy()[:, :7]))
    out = mcmc_draw_parameters(df, covs, trace=0, forecast=kw, **RUN)
    assert np.array_equal(bits(np.stack(out["level_1"])), bits(l1))
    frames_equal(out["forecast"], host)
    assert "forecast" not in mcmc_draw_parameters(df, covs, trace=0, **RUN)
    with pytest.raises(ValueError):
        mcmc_draw_parameters(df, covs, trace=0, draw_sink="summary", forecast=True, **RUN)
    with HipSampler(p, n_mh_steps=20, draw_sink="summary", **RUN) as s:
        s.run(120)
        with pytest.raises(_lib.ClvError, match="-3"):
            s.forecast()
    # the closed form lets an alive customer drop out during the holdout; the simulation does not
    tb = A.forecast_table(host, df)
    assert tb["by_frequency"]["n"].sum() == 553 and np.isfinite(tb["metrics"].to_numpy()).all()
    assert int(A.forecast_pit(host).sum()) == 553

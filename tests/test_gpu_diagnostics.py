"""Convergence diagnostics on the GPU (csrc/diag.hip) against the numpy yardstick
(tests/diagnostics_ref.py): split R-hat, mean ESS, MCSE, mean, sd and the truncation lag per series.

Tolerances (float64 summation, not guessed): the truncation lag is compared exactly — the yardstick's
decision margin is >= 1e-6 on every input set (tests/test_diagnostics_cpu.py) while a different
summation order moves rho(t) by at most h 2^-52; R-hat within relative 1e-11; ESS and MCSE within
relative 1e-8 (each rho(t) carries at most h 2^-52 of absolute error, tau adds at most 2 (lag + 2) of
them and tau >= 0.25: 8 * 3000 * 3000 * 2^-52 = 1.6e-8 in the worst case at the largest shape, about
3e-9 at the lags seen; a wrong lag or an off-by-one moves ESS by 1e-3 or more); mean and sd within
rtol 1e-12, atol 1e-12 max|y|."""
import ctypes

import numpy as np
import pytest

from tests import diagnostics_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu

MEAN, SD, MCSE, ESS, RHAT, LAG = range(6)


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def gpu_stats(L, arr, period=1, log_mask=0):
    """One clv_diagnostics call on arr (m, n, n_series)."""
    from mcmc_clv_model_amd._lib import check, dptr
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    m, n, ns = arr.shape
    out = np.full((ns, 6), -7.0)
    check(L.clv_diagnostics(-1, dptr(arr), m, n, ns, period, log_mask, dptr(out)))
    return out


def assert_parity(got, want, ymax, label):
    nan = np.isnan(want[:, 0])
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN rows differ"
    assert np.isnan(want[nan]).all()
    g, w = got[~nan], want[~nan]
    rel = lambda k: float(np.max(np.abs(g[:, k] / w[:, k] - 1.0))) if len(w) else 0.0  # noqa: E731
    print(f"{label}: lag mismatches {int((g[:, LAG] != w[:, LAG]).sum())}, max rel rhat {rel(RHAT):.2e} "
          f"ess {rel(ESS):.2e} mcse {rel(MCSE):.2e} mean abs {np.max(np.abs(g[:, MEAN] - w[:, MEAN])):.2e} sd {rel(SD):.2e}")
    assert np.array_equal(g[:, LAG], w[:, LAG]), f"{label}: truncation lag"
    np.testing.assert_allclose(g[:, RHAT], w[:, RHAT], rtol=1e-11, atol=0, err_msg=label)
    np.testing.assert_allclose(g[:, ESS], w[:, ESS], rtol=1e-8, atol=0, err_msg=label)
    np.testing.assert_allclose(g[:, MCSE], w[:, MCSE], rtol=1e-8, atol=0, err_msg=label)
    np.testing.assert_allclose(g[:, MEAN], w[:, MEAN], rtol=1e-12, atol=1e-12 * ymax, err_msg=label)
    np.testing.assert_allclose(g[:, SD], w[:, SD], rtol=1e-12, atol=1e-12 * ymax, err_msg=label)


@pytest.mark.parametrize("shape", R.SMALL_SHAPES)
def test_parity_small_set(L, shape):
    arr = R.small_set()[shape]
    assert_parity(gpu_stats(L, arr), R.reference(f"small:{shape[0]}:{shape[1]}")[0], np.abs(arr).max(), f"small {shape}")


@pytest.mark.parametrize("shape", R.MIN_SHAPES)
def test_parity_minimum_length_set(L, shape):
    arr = R.min_set()[shape]
    want = R.reference(f"min:{shape[0]}:{shape[1]}")[0]
    if shape[1] < 10:
        assert (want[:, LAG] == -1).all()  # h = 4: no pair is ever evaluated
    assert_parity(gpu_stats(L, arr), want, np.abs(arr).max(), f"min {shape}")


def test_parity_long_set_global_memory_path(L):
    arr = R.long_set()
    assert arr.shape[0] * arr.shape[1] * 8 > 160 * 1024  # beyond any LDS budget
    assert_parity(gpu_stats(L, arr), R.reference("long")[0], np.abs(arr).max(), "long")


def test_parity_on_both_sides_of_the_lds_threshold(L):
    """2 x 4096 draws fill the kernel's LDS budget exactly (64 KiB), 2 x 4097 take the global-memory
    path: parity with the yardstick on both sides of the threshold."""
    rng = np.random.default_rng(17)
    for n in (4096, 4097):
        arr = np.stack([R.ar1(rng, 2, n, 0.9) for _ in range(3)], axis=2)
        want, mg = R.stats_many(arr)
        assert mg.min() >= 1e-6  # of the yardstick alone (measured 4.6e-4): the lag is comparable exactly
        assert_parity(gpu_stats(L, arr), want, np.abs(arr).max(), f"threshold n={n}")


@pytest.mark.parametrize("kind", ["bi", "tri"])
def test_parity_real_draws(L, kind):
    """Real level-1 draws with lambda and mu logged, through clv_diagnostics and level1_diagnostics; the
    customers whose z never changes are NaN in both (12 series bi, 21 tri)."""
    from mcmc_clv_model_amd.analysis import level1_diagnostics
    a, w, mask, want, _ = R.golden_level1(kind)
    n = a.shape[2]
    assert int(np.isnan(want[:, 0]).sum()) == {"bi": 12, "tri": 21}[kind]
    ymax = max(np.abs(np.log(a[..., :2])).max(), np.abs(a[..., 2:]).max())
    got = gpu_stats(L, a.reshape(a.shape[0], a.shape[1], n * w), period=w, log_mask=mask)
    assert_parity(got, want, ymax, f"golden {kind}")
    df = level1_diagnostics({"level_1": list(a)})
    params = ["log_lambda", "log_mu", "tau", "z"] + (["eta"] if w == 5 else [])
    assert list(df.columns) == [f"{s}_{p}" for p in params for s in R.STATS] and len(df) == n
    assert np.array_equal(bits(df.to_numpy().reshape(n * w, 6)), bits(got))
    plain = level1_diagnostics({"level_1": list(a)}, log_columns=())
    assert "rhat_lambda" in plain and "rhat_log_lambda" not in plain
    assert np.array_equal(bits(plain["ess_tau"]), bits(df["ess_tau"]))


def test_non_finite_series_is_nan_and_neighbours_untouched(L):
    arr = R.small_set()[(2, 101)][:, :, :70].copy()
    clean = gpu_stats(L, arr)
    arr[1, 57, 33] = np.inf
    got = gpu_stats(L, arr)
    assert np.isnan(got[33]).all()
    keep = np.arange(70) != 33
    assert np.array_equal(bits(got[keep]), bits(clean[keep])) and np.isfinite(clean).all()
    # a logged series with a non-positive value, period 3: series 1, 4, 7, ... are logged
    pos = np.exp(R.small_set()[(3, 16)][:, :, :9])
    pos[0, 2, 4] = -1.0
    got = gpu_stats(L, pos, period=3, log_mask=0b010)
    assert np.isnan(got[4]).all() and np.isfinite(got[np.arange(9) != 4]).all()
    want, _ = R.stats_many(pos, log_mask=0b010, period=3)
    assert_parity(got, want, np.abs(pos).max(), "logged, period 3")


def test_autocorr_matches_numpy(L):
    from mcmc_clv_model_amd._lib import check, dptr
    from mcmc_clv_model_amd.analysis import level2_autocorr
    rng = np.random.default_rng(19)
    arr = np.ascontiguousarray(np.stack([R.ar1(rng, 3, 200, 0.1 * k) for k in range(8)], axis=2))
    outs = {}
    for max_lag in (100, 199, 0):
        out = np.full((3, 8, max_lag + 1), -7.0)
        check(L.clv_autocorr(-1, dptr(arr), 3, 200, 8, max_lag, dptr(out)))
        want = np.stack([R.autocorr(arr[:, :, s], max_lag) for s in range(8)], axis=1)
        np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)
        assert (out[..., 0] == 1.0).all()
        outs[max_lag] = out
    acf = level2_autocorr({"level_2": list(arr)}, max_lag=100)
    assert acf.shape == (3, 8, 101) and np.array_equal(bits(acf), bits(outs[100]))
    assert np.array_equal(bits(outs[199][..., :101]), bits(outs[100]))  # a lag's sum does not depend on max_lag


@pytest.mark.parametrize("D", [2, 3])
def test_sampler_route_equals_host_route_bitwise(L, D):
    """HipSampler.diagnostics() on the draws in HBM == level1_diagnostics / level2_diagnostics on the
    draws read back, bit for bit (n = 300 is no multiple of the 256-customer block)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.analysis import level1_diagnostics, level2_diagnostics
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    p = build_problem(cdnow("abe", n=300), [], D=D)
    with HipSampler(p, mcmc=40, burnin=20, thin=1, chains=2, seed=5) as s:
        out = np.empty((300 * (D + 2), 6))
        assert L.clv_diagnostics_sampler(s.h, 3, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None) == -3  # CLV_ESTATE
        s.run(60)
        dev = s.diagnostics()
        l1, l2, _ = s.read_draws()
    draws = dict(level_1=list(l1), level_2=list(l2))
    host1, host2 = level1_diagnostics(draws), level2_diagnostics(draws)
    assert list(dev["level_1"].columns) == list(host1.columns) and dev["level_1"].shape == (300, 6 * (D + 2))
    assert np.array_equal(bits(dev["level_1"].to_numpy()), bits(host1.to_numpy()))
    assert np.array_equal(bits(dev["level_2"].to_numpy()), bits(host2.to_numpy()))
    assert dev["level_2"].shape == (D + D * (D + 1) // 2, 6) and np.isfinite(dev["level_2"].to_numpy()).all()
    # against the yardstick too (lambda, mu logged)
    w = D + 2
    # (series whose yardstick margin is below 1e-6 have no exactly comparable lag: left out)
    want, mg = R.stats_many(l1.reshape(2, 40, 300 * w), log_mask=3, period=w)
    sure = mg >= 1e-6
    print(f"D={D}: {int(sure.sum())} of {len(sure)} series compared")
    assert sure.mean() > 0.99
    ymax = max(np.abs(np.log(l1[..., :2])).max(), np.abs(l1[..., 2:]).max())
    assert_parity(host1.to_numpy().reshape(300 * w, 6)[sure], want[sure], ymax, f"sampler draws D={D}")
    with HipSampler(p, mcmc=40, burnin=20, thin=1, chains=2, seed=5, draw_sink="summary") as s:
        s.run(60)
        with pytest.raises(_lib.ClvError):
            s.diagnostics()
        only2 = s.diagnostics(level1=False)["level_2"]
        l2s = s.read_draws(level1=False)[1]
    assert np.array_equal(bits(only2.to_numpy()), bits(level2_diagnostics(dict(level_2=list(l2s))).to_numpy()))


def test_drop_in_keyword(L):
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    from mcmc_clv_model_amd.analysis import level1_diagnostics, level2_diagnostics
    df = cdnow("abe", n=300)
    kw = dict(mcmc=40, burnin=20, thin=1, chains=2, seed=5, trace=0)
    for fn in (mcmc_draw_parameters, mcmc_draw_parameters_rfm_m):
        a = fn(df, **kw)
        b = fn(df, diagnostics=True, **kw)
        assert "diagnostics" not in a and set(b) == set(a) | {"diagnostics"}
        assert np.array_equal(bits(np.stack(a["level_1"])), bits(np.stack(b["level_1"])))
        assert np.array_equal(bits(np.stack(a["level_2"])), bits(np.stack(b["level_2"])))
        assert np.array_equal(bits(a["log_likelihood"]), bits(b["log_likelihood"]))
        d = b["diagnostics"]
        assert np.array_equal(bits(d["level_1"].to_numpy()), bits(level1_diagnostics(a).to_numpy()))
        assert np.array_equal(bits(d["level_2"].to_numpy()), bits(level2_diagnostics(a).to_numpy()))
        assert len(d["level_1"]) == 300
        with pytest.raises(ValueError, match="draw_sink='full'"):
            fn(df, diagnostics=True, draw_sink="summary", **kw)

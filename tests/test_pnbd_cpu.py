"""CPU: the Pareto/NBD models and fixtures (tests/pnbd_ref.py, tests/golden/pnbd_*.npz), the numpy
BFGS of mcmc_clv_model_amd.mle and its host formulas.  The device side is tests/test_gpu_pnbd.py."""
import sys
import warnings

import numpy as np
import pytest

from tests import pnbd_ref as R
from tests.helpers import GOLDEN, cdnow, golden

sys.path.insert(0, GOLDEN)
import make_pnbd_goldens as G  # noqa: E402

# Fader & Hardie's published CDNOW estimates (r, alpha, s, beta, log L) and the optima recorded in DESIGN.md section 4e
PUBLISHED = (0.553, 10.578, 0.606, 11.669, -9595.0)
OPTIMUM = dict(abe=((0.55328, 10.5777, 0.60624, 11.6687), -9594.9762),
               full=((0.59742, 11.5857, 0.52219, 8.8278), -95415.1186))


@pytest.fixture(scope="module")
def fits():
    """The numpy-model fits of both CBS fixtures from both starts, computed once."""
    out = {}
    for name in ("abe", "full"):
        for start in ((1.0, 1.0, 1.0, 1.0), (3.0, 1.0, 0.3, 20.0)):
            with warnings.catch_warnings():
                warnings.simplefilter("error")          # a converged fit does not warn
                out[name, start] = G.fit_model(name, start)
    return out


def test_edge_fixture_regenerates_identically():
    pytest.importorskip("mpmath")
    e, new = golden("pnbd_edge.npz"), G.build_edge()
    assert sorted(e.files) == sorted(new)
    for k in e.files:
        assert np.array_equal(e[k], new[k], equal_nan=True), k


def test_edge_fixture_covers_the_issue_cases():
    e = golden("pnbd_edge.npz")
    x, tx, T, P = e["x"], e["t_x"], e["T"], e["params"]
    assert len(x) == 12 and P.shape == (6, 4)
    assert np.any((x == 0) & (tx == 0)) and np.any(tx == T) and np.any(tx == T - 1e-12) and np.any(tx == 1e-9)
    assert {17, 60, 200} <= set(x.tolist()) and np.any(T == 1.0)
    assert P[0, 1] < P[0, 3] and P[1, 1] == P[0, 3] and P[1, 3] == P[0, 1] and P[2, 1] == P[2, 3]
    assert e["model_terms"][2].max() == 0 and 600 <= e["model_terms"][3].max() <= 800
    assert not e["model_nan"][:5].any() and e["model_nan"][5].any()
    # the last set's converged customers stop well short of the cap: device and model agree on who is NaN
    assert e["model_terms"][5][~e["model_nan"][5]].max() < 0.75 * R.TERM_CAP


def test_model_meets_its_recorded_error():
    e = golden("pnbd_edge.npz")
    for k, p in enumerate(e["params"]):
        m = R.model_customers(e["x"], e["t_x"], e["T"], p, float(e["t_star"]))
        ok = ~e["model_nan"][k]
        assert np.array_equal(m["converged"], ok)
        assert np.isnan(m["logL"][~ok]).all() and np.isnan(m["grad"][~ok]).all()
        for key in ("logL", "p_alive", "ey"):
            assert G.rel(m[key][ok], e[key][k][ok]).max() <= e["eref_" + key][k], (k, key)
        if ok.all():
            err = np.abs(m["grad"].sum(0) - e["grad_sum"][k]) / np.maximum(1.0, e["grad_abs"][k])
            assert err.max() <= e["eref_grad"][k], k
    assert np.nanmax(e["eref_logL"]) < 1e-13     # the log form: 1.5e-7 when 2F1 is summed directly


@pytest.mark.parametrize("name", ["abe", "full"])
def test_optimum_and_start_agreement(fits, name):
    want_p, want_ll = OPTIMUM[name]
    (p1, ll1, f1), (p2, ll2, f2) = fits[name, (1.0, 1.0, 1.0, 1.0)], fits[name, (3.0, 1.0, 0.3, 20.0)]
    for p, ll, f in ((p1, ll1, f1), (p2, ll2, f2)):
        assert f.converged_ and f.n_eval_ < 200 and f.grad_norm_ <= 1e-7
        assert np.allclose(p, want_p, rtol=1e-4, atol=0) and abs(ll - want_ll) < 1e-4
    assert abs(ll1 - ll2) <= 1e-6 and np.allclose(p1, p2, rtol=1e-4, atol=0)
    g = golden("pnbd_fit.npz")
    assert abs(ll1 - float(g[f"{name}_logL"])) <= 1e-6 and np.allclose(p1, g[f"{name}_params"], rtol=1e-4, atol=0)
    if name == "abe":
        assert np.allclose(p1, PUBLISHED[:4], rtol=0, atol=6e-4) and abs(ll1 - PUBLISHED[4]) < 0.05


def test_start_outside_the_series_domain_does_not_converge_quietly():
    from mcmc_clv_model_amd.mle import ParetoNBDFitter
    df = cdnow("abe", 300)
    vg = R.model_value_and_grad(df["x"].to_numpy(), df["t_x"].to_numpy(), df["T_cal"].to_numpy())
    assert not np.isfinite(vg(np.log([0.03, 0.48, 0.71, 40.2]))[0])     # x = 0, t_x = 0 rows: z = 0.988
    f = ParetoNBDFitter()
    with pytest.warns(RuntimeWarning, match="did not converge"):
        f.fit_objective(vg, (0.03, 0.48, 0.71, 40.2))
    assert f.converged_ is False and f.n_eval_ == 1 and "starting point" in f.message_


def test_minimize_bfgs_backtracks_non_finite_trials_and_reports_max_iter():
    from mcmc_clv_model_amd.mle import minimize_bfgs

    def rosen(t):   # NaN outside |t| <= 3: a failed trial step, not a value
        if np.max(np.abs(t)) > 3.0:
            return np.nan, np.full(2, np.nan)
        a, b = t
        return (1 - a) ** 2 + 100 * (b - a * a) ** 2, np.array([-2 * (1 - a) - 400 * a * (b - a * a), 200 * (b - a * a)])

    res = minimize_bfgs(rosen, [-1.2, 1.0], tol=1e-8, max_iter=200)
    assert res.converged and np.allclose(res.x, 1.0, atol=1e-6) and res.grad_norm <= 1e-8
    short = minimize_bfgs(rosen, [-1.2, 1.0], tol=1e-8, max_iter=3)
    assert not short.converged and short.n_iter == 3 and "max_iter" in short.message


def test_host_formulas():
    from mcmc_clv_model_amd.mle import ParetoNBDFitter, phi
    import pandas as pd
    f = ParetoNBDFitter()
    with pytest.raises(RuntimeError):
        f.expected_number_of_purchases_up_to_time(1.0)
    t = np.array([0.0, 1.0, 7.5, 39.0])
    f.params_ = pd.Series([0.5, 10.0, 1.0, 12.0], index=["r", "alpha", "s", "beta"])     # s = 1 exactly
    assert np.array_equal(f.expected_number_of_purchases_up_to_time(t), 0.5 * 12.0 / 10.0 * np.log1p(t / 12.0))
    f.params_ = pd.Series([0.5, 10.0, 3.0, 12.0], index=["r", "alpha", "s", "beta"])     # s - 1 = 2: closed form
    want = 0.5 * 12.0 / 10.0 * (1.0 - (12.0 / (12.0 + t)) ** 2) / 2.0
    assert np.allclose(f.expected_number_of_purchases_up_to_time(t), want, rtol=1e-14, atol=0)
    assert np.array_equal(f.expected_number_of_purchases_up_to_time(t), R.model_expected_purchases(t, f.params_))
    assert phi(0.0, 0.25) == 0.25 and phi(1e-9, 0.25) == pytest.approx(0.25, rel=1e-9)


def test_mape_aggregate_by_hand():
    import mcmc_clv_model_amd as pkg
    from mcmc_clv_model_amd.mle import mape_aggregate
    # cumulative actual 2, 6, 12; predicted 1, 6, 15: |dev| 1, 0, 3 -> mean 4/3 over 12 -> 100/9 percent
    assert mape_aggregate([2, 4, 6], [1, 5, 9]) == pytest.approx(100.0 / 9.0, rel=1e-15)
    assert pkg.mape_aggregate is mape_aggregate and pkg.pnbd_weekly_tracking.__module__.endswith("mle")
    assert pkg.ParetoNBDFitter(penalizer_coef=0.0).penalizer_coef == 0.0


def test_device_sum_order_model():
    """pnbd_ref.device_sum is a permutation-free restatement: exact on integers, and equal to the
    plain tree for one block."""
    v = np.arange(1, 2358, dtype=np.float64)
    assert R.device_sum(v) == v.sum()
    w = np.random.default_rng(3).normal(size=256)
    assert R.device_sum(w) == R.tree256(w[None])[0]


@pytest.mark.parametrize("n", [65_537, 524_545])
def test_device_sum_second_level(n):
    """More than 256 block partials (257: lane 0 adds partials 0 and 256; 2,050: up to 9 per lane): on
    integers, whose every partial sum is exact, device_sum equals math.fsum — each value enters once."""
    import math
    assert -(-n // 256) == {65_537: 257, 524_545: 2_050}[n]
    v = np.arange(1, n + 1, dtype=np.float64)
    assert R.device_sum(v) == math.fsum(v) == n * (n + 1) / 2
    w = np.random.default_rng(5).integers(-2 ** 20, 2 ** 20, n).astype(np.float64)     # signed, |sum| < 2^40
    assert R.device_sum(w) == math.fsum(w)
    one = np.zeros(n)
    one[-1] = 3.0                                                                      # the last block's only customer
    assert R.device_sum(one) == 3.0


def test_create_validation_runs_before_any_device_call():
    """Every CLV_EINVAL path of clv_pnbd_create / clv_pnbd_track is host code: reachable without a GPU."""
    import ctypes
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    x, tx, T = np.array([1, 0, 2], np.int32), np.array([1.0, 0.0, 3.0]), np.array([2.0, 5.0, 3.0])
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    h = ctypes.c_void_p()

    def create(n=3, x=x, tx=tx, T=T, w=None):
        return L.clv_pnbd_create(-1, n, ip(x), _lib.dptr(tx), _lib.dptr(T), _lib.dptr(w), ctypes.byref(h))

    bad = [(dict(n=0), "n must be"), (dict(x=np.array([1, -1, 2], np.int32)), "negative x at customer 1"),
           (dict(tx=np.array([1.0, 0.0, 3.5])), "t_x <= T violated at customer 2"),
           (dict(tx=np.array([-0.5, 0.0, 3.0])), "t_x <= T violated at customer 0"),
           (dict(T=np.array([2.0, np.inf, 3.0])), "non-finite"), (dict(tx=np.array([np.nan, 0.0, 3.0])), "non-finite"),
           (dict(w=np.array([1.0, -1.0, 1.0])), "weight at customer 1"),
           (dict(w=np.array([1.0, 1.0, np.nan])), "weight at customer 2")]
    for kw, msg in bad:
        assert create(**kw) == -1 and not h.value, kw
        assert msg in L.clv_last_error().decode(), (kw, L.clv_last_error())
    b, t, p, out = np.array([1.0, 2.0]), np.array([1.0, 2.0, 3.0]), np.array([1.0, 1.0, 1.0, 1.0]), np.zeros(3)
    track = lambda n=2, b=b, t=t, nt=3, p=p: L.clv_pnbd_track(-1, n, _lib.dptr(b), _lib.dptr(t), nt, _lib.dptr(p),  # noqa: E731
                                                              _lib.dptr(out))
    for kw in (dict(n=0), dict(nt=0), dict(nt=65536), dict(p=np.array([1.0, 0.0, 1.0, 1.0])),
               dict(p=np.array([1.0, 1.0, np.inf, 1.0])), dict(b=np.array([1.0, np.nan])),
               dict(t=np.array([1.0, np.inf, 3.0]))):
        assert track(**kw) == -1 and L.clv_last_error(), kw
    L.clv_pnbd_destroy(None)

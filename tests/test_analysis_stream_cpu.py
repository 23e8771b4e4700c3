"""Pins tests/analysis_stream_ref.py — the float64 model that tests/test_gpu_analysis_stream.py holds
the predictive, tracking and generator kernels to — without a GPU: its Poisson is a Poisson, its
borderline share stays under the cap at the GPU module's shapes, its generator reproduces the
reference's generate_pareto_abe fed the same variates (tests/golden/generator_replay.npz), its
fixed-order tracking rate is the exact rate to rounding, and its tau_star is the oracle's."""
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import stats

from oracle import analysis_cpu as oan
from tests import analysis_stream_ref as A
from tests.helpers import GOLDEN

MEANS = (0.3, 2.0, 9.99, 10.0, 37.5, 600.0, 1e5)
N_DRAWS = 1_000_000


@functools.lru_cache(maxsize=None)
def _draws(m):
    return A.poisson(np.full(N_DRAWS, m), A.SEED_LO, np.arange(N_DRAWS), 3, 0, A.STREAM_PREDICT)


@pytest.mark.parametrize("m", MEANS)
def test_model_poisson_is_poisson(m):
    """1,000,000 model draws per mean: the chi-square bucketing of test_poisson_sampler_distribution
    (tests/test_gpu_analysis.py) against scipy.stats.poisson, p > 1e-4; mean and variance within 6
    standard errors of m."""
    x, _ = _draws(m)
    lo, hi = stats.poisson.ppf([1e-6, 1 - 1e-6], m).astype(int)
    counts = np.bincount(np.clip(x, lo - 1, hi) - (lo - 1), minlength=hi - lo + 2)
    obs = np.concatenate([[counts[0]], counts[1:hi - lo + 1], [counts[hi - lo + 1]]])
    p = np.concatenate([[stats.poisson.cdf(lo - 1, m)], stats.poisson.pmf(np.arange(lo, hi), m),
                        [stats.poisson.sf(hi - 1, m)]])
    keep = p * x.size >= 5
    chi = ((obs[keep] - p[keep] * x.size) ** 2 / (p[keep] * x.size)).sum()
    pval = stats.chi2.sf(chi, keep.sum() - 1)
    print(f"m = {m}: chi2 {chi:.1f} on {keep.sum() - 1} dof, p = {pval:.3g}; mean {x.mean():.6g}, variance {x.var():.6g}")
    assert pval > 1e-4, (m, chi)
    assert abs(x.mean() - m) < 6 * np.sqrt(m / x.size)
    assert abs(x.var() - m) < 6 * np.sqrt((m + 2 * m * m) / x.size)   # var of the sample variance ~ (m + 2 m^2) / n


def _gpu_case_margins():
    """(name, margins) of the model on exactly the inputs of the GPU module, both seeds."""
    for seed in A.SEEDS:
        for name, c, kw in (("P1", A.predict_case_p1(), {}), ("P2", A.predict_case_p2(), dict(simulate_spend=True)),
                            ("P3", A.predict_case_p3(), {})):
            yield f"{name}/{seed:#x}", A.predict(c["level1"], c["T_cal"], c["T_star"], seed, **kw)["margin"]
        for name, c in (("T1", A.track_case_t1()), ("T2-113", A.track_case_t2(113)), ("T2-225", A.track_case_t2(225)),
                        ("T3", A.track_case_t3())):
            yield f"{name}/{seed:#x}", A.track(c["level1"], c["birth"], c["times"], seed)["margin"]
        for name, c in A.gen_cases().items():
            p = A.gen_params(c["n"], c["beta"], c["gamma"], seed, c["covars"])
            yield f"{name}/{seed:#x}", A.gen_events(p["lam"], p["tau"], c["T_cal"], c["T_star"], seed)["margin"]


def test_borderline_cap_holds_for_the_model_alone():
    """The share of lanes with margin <= RTOL is at most BORDERLINE_CAP at every mean and at every
    shape the GPU module uses.  Measured with this margin definition, lanes of 1,000,000 per mean:
    0 at 0.3, 2, 9.99, 10, 37.5 and 600; 3 at 1e5 (the floor's argument within 1e-12 * ~1e5 of an
    integer).  At 1e7 it is 698 (0.07 %: the floor again), which is why the GPU cases keep means
    <= 1e5.  Every GPU-module case: 0 lanes, both seeds."""
    for m in MEANS:
        _, mg = _draws(m)
        n_b = int((mg <= A.RTOL).sum())
        print(f"m = {m}: {n_b} of {mg.size} lanes borderline, smallest margin {mg.min():.2e}")
        assert n_b <= A.BORDERLINE_CAP * mg.size, m
    for name, mg in _gpu_case_margins():
        n_b = int((mg <= A.RTOL).sum())
        print(f"{name}: {n_b} of {mg.size} lanes borderline, smallest margin {mg.min():.2e}")
        assert n_b <= A.BORDERLINE_CAP * mg.size, name


def _rel_dev(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0))


@pytest.mark.parametrize("name", ["scalar", "percust", "k1"])
def test_generator_model_matches_reference_replay(name):
    """generate_pareto_abe of the reference, fed the model's variates through a stub Generator
    (make_goldens.py, step generator_replay), against the model: integers, alive_true and row counts
    exact; floats to 1e-12 relative (covars @ beta goes through BLAS in the reference, and it scales
    where the model divides)."""
    f = np.load(f"{GOLDEN}/generator_replay.npz", allow_pickle=False)
    assert name in list(f["cases"])
    g = lambda k: f[f"{name}_{k}"]  # noqa: E731
    n, seed, T_cal, T_star, beta = int(g("n")), int(g("seed")), g("T_cal"), g("T_star"), g("beta")
    covars = g("covars") if g("covars").size else None
    p = A.gen_params(n, beta, f["gamma"], seed, covars)
    K = beta.shape[0]
    for j in range(K):   # generated: pure arithmetic on u53; supplied: passed through — bitwise either way
        assert np.array_equal(p["cov"][:, j], g(f"cbs_cov{j}")), j
    devs = {k: _rel_dev(p[k], g(f"cbs_{c}")) for k, c in (("lam", "lambda_true"), ("mu", "mu_true"), ("tau", "tau_true"))}
    # the event rules, teacher-forced with the reference's own (lambda, tau)
    e = A.gen_events(g("cbs_lambda_true"), g("cbs_tau_true"), T_cal, T_star, seed)
    assert (e["margin"] > A.RTOL).all()
    assert np.array_equal(g("cbs_cust"), np.arange(1, n + 1))
    assert np.array_equal(e["x"], g("cbs_x"))
    assert np.array_equal(e["alive"], g("cbs_alive_true"))
    assert np.array_equal(g("cbs_T_cal"), np.full(n, np.max(T_cal)))
    for k, ts in enumerate(T_star):
        col = f"cbs_x_star{int(ts)}" if T_star.size > 1 else "cbs_x_star"
        assert np.array_equal(e["x_star"][k], g(col)), col
    assert e["elog_t"].size == g("elog_t").size == e["n_events"].sum()
    assert np.array_equal(e["elog_cust"], g("elog_cust"))
    devs["t_x"] = _rel_dev(e["t_x"], g("cbs_t_x"))
    devs["elog_t"] = _rel_dev(e["elog_t"], g("elog_t"))
    print(f"{name}: n = {n}, {e['elog_t'].size} events; largest relative deviation " +
          ", ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    for k, v in devs.items():
        assert v <= 1e-12, (k, v)
    # and run freely: the model's own (lambda, tau) decide the same events on clear customers
    e2 = A.gen_events(p["lam"], p["tau"], T_cal, T_star, seed)
    clear = e2["margin"] > A.RTOL
    assert clear.mean() >= 1 - A.BORDERLINE_CAP
    assert np.array_equal(e2["x"][clear], g("cbs_x")[clear]) and np.array_equal(e2["n_events"][clear], e["n_events"][clear])


@pytest.mark.parametrize("case", ["T1", "T2-113", "T2-225", "T3"])
def test_tracking_fixed_order_rate_is_the_exact_rate_to_rounding(case):
    """|fixed-order rate - exact rate| <= n_adds * eps * peak rate, with n_adds = 2 n + 65 min(112,
    n_times) from the shape (analysis_stream_ref.track_n_adds) and the peak of the draw's exact weekly
    rates; weeks whose exact rate is 0 have a model rate below that bound."""
    c = {"T1": A.track_case_t1, "T2-113": lambda: A.track_case_t2(113), "T2-225": lambda: A.track_case_t2(225),
         "T3": A.track_case_t3}[case]()
    rate = A.track_rates(c["level1"], c["birth"], c["times"])
    exact = A.track_exact_rates(c["level1"], c["birth"], c["times"])
    n, nt = c["level1"].shape[1], len(c["times"])
    bound = A.track_n_adds(n, nt) * np.finfo(np.float64).eps * exact.max(axis=1, keepdims=True)
    err = np.abs(rate - exact)
    print(f"{case}: largest |fixed-order - exact| {err.max():.2e} (bound {bound.min():.2e}); {int((exact == 0).sum())} "
          f"weeks of exact rate 0, largest model rate there {rate[exact == 0].max(initial=0.0):.2e}")
    assert (err <= bound).all()
    assert (rate >= 0).all()
    if case == "T3":
        assert (exact == 0).sum() >= 20 and exact.max() > 5e4
    if case.startswith("T2"):   # customers active across a pass boundary, tied neighbouring times
        t, b, end = c["times"], c["birth"], c["birth"] + c["level1"][0, :, 2]
        assert ((b < t[111]) & (end >= t[112])).sum() > 10 and (np.diff(t) == 0).sum() > 5
        assert np.isin(b, t).any() and np.isin(end, t).any()


def test_model_predict_matches_oracle_tau_star_and_zero_pattern():
    """tau_star and the pattern of zero means agree exactly with oracle.analysis_cpu (bi:538-540) on
    the reference's own draws; the reference's counts and the model's are 0 there."""
    f = np.load(f"{GOLDEN}/analysis_abe400.npz", allow_pickle=False)
    l1 = np.concatenate(list(f["bi_level1"]))
    T_cal = f["T_cal"]
    r = A.predict(l1, T_cal, 39.0, A.SEED_LO)
    ts = np.stack([oan.future_tau_star(T_cal, d, 39.0) for d in l1])
    assert np.array_equal(r["tau_star"], ts)
    zero = l1[..., 0] * ts == 0.0
    assert zero.any() and not zero.all()
    assert np.array_equal(r["mean"] == 0.0, zero)
    assert (r["x"][zero] == 0).all() and (f["xstar_bi"][zero] == 0).all()
    cbs = pd.DataFrame(dict(T_cal=T_cal))
    assert (oan.draw_future_transactions_bi(cbs, dict(level_1=list(f["bi_level1"])), 39.0, seed=1)[zero] == 0).all()
    # same distribution as the reference's counts: the totals are Poisson(sum of the means) samples
    sd = np.sqrt(r["mean"].sum())
    assert abs(r["x"].sum() - r["mean"].sum()) < 5 * sd and abs(f["xstar_bi"].sum() - r["mean"].sum()) < 5 * sd

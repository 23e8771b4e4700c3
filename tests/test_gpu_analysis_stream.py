"""Predictive, tracking and generator draws of the HIP kernels (csrc/analysis.hip predict_kernel /
track_kernel, csrc/elog.hip generate_kernel) against the float64 model of tests/analysis_stream_ref.py
(pinned without a GPU by tests/test_analysis_stream_cpu.py), value by value, and the exact statistics
(level1_summary, chain_total_loglik) at their edge shapes against plain numpy.

Every variate is a pure function of (seed, counter), so the model predicts every integer exactly and
every float to RTOL = 1e-12 relative.  A lane whose model decision margin is <= RTOL is set aside; at
most BORDERLINE_CAP = 0.1 % of a case's lanes may be (the CPU module asserts the model alone meets that
at exactly these inputs).  The generator is teacher-forced: the device's lambda_true, mu_true and
tau_true are first held to the model's own within RTOL, then fed to the model's event rules.  All
cases go through the host-array entries and use two seeds, one with a non-zero high key word.

Power: the same device outputs are compared with one thing wrong at a time in the model's inputs
(customer and draw swapped in the predict counter; the tracking stream for predict; spend slots based
at 2^20 - 1; the week index taken pass-relative; t >= b for t > b; gap slots from 15; the lifetime
read from (z, w)); each must fail on at least 1 % of the lanes.

Beyond one customer batch and one pass of the draw grid: the level-1 summary in batches of
CLV_SUMMARY_BATCH customers (float64 keys and the "summary+pct" sink's float32 keys), and
chain_total_loglik / weekly tracking at 2^20 + 3 draws, past the 2^20 workgroups their kernels launch.

Measured on MI355X: see DESIGN.md §2 ("Predictive, tracking and generator draws").
"""
import math

import numpy as np
import pandas as pd
import pytest
from scipy.special import gammaln

from tests import analysis_stream_ref as A

pytestmark = pytest.mark.gpu

POWER_MIN = 0.01
SEED_IDS = ["seed7", "seed_hi"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mcmc_clv_model_amd import _lib
    _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"


def _close(got, ref):
    return np.abs(got - ref) <= A.RTOL * np.abs(ref)


def _dev(got, ref, mask):
    if not np.any(mask):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / np.abs(ref)
    return float(np.nan_to_num(r[mask], nan=0.0).max())


def _report(name, fail, clear, **devs):
    lanes, aside = clear.size, int((~clear).sum())
    print(f"{name}: {lanes} lanes, {aside} set aside, {int((fail & clear).sum())} clear lanes differ" +
          "".join(f"; largest relative deviation of {k} {v:.2e}" for k, v in devs.items()))
    assert aside <= A.BORDERLINE_CAP * lanes, f"{name}: {aside} of {lanes} lanes set aside"
    assert not (fail & clear).any(), f"{name}: {int((fail & clear).sum())} clear lanes differ from the model"


def _power(name, share):
    print(f"{name}: power, share of lanes failing {share:.3f}")
    assert share >= POWER_MIN, (name, share)


# ---------------------------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------------------------
def _predict_dev(c, seed, spend=None, sigma_s=0.5):
    from mcmc_clv_model_amd.analysis import draw_future_transactions, draw_future_transactions_rfm_m
    cbs = pd.DataFrame(dict(T_cal=c["T_cal"]))
    draws = dict(level_1=[c["level1"]])
    if spend is None:
        return draw_future_transactions(cbs, draws, T_star=c["T_star"], seed=seed)
    return draw_future_transactions_rfm_m(cbs, draws, T_star=c["T_star"], simulate_spend=spend, sigma_s=sigma_s, seed=seed)


@pytest.mark.parametrize("seed", A.SEEDS, ids=SEED_IDS)
def test_predict_counts_p1(seed):
    """P1: n = 257, 3 draws, width 4; means {0, 0.3, 9.99, nextafter(10, 0), 10, 37.5, 600, 1e5} hit
    exactly, each under the four tau_star modes; z in {0, 0.5, 0.75, 1} against the threshold > 0.5."""
    c = A.predict_case_p1()
    x = _predict_dev(c, seed)
    r = A.predict(c["level1"], c["T_cal"], c["T_star"], seed)
    # the case reaches what it claims: every target mean in every mode that keeps it, the clip branch
    assert set(np.unique(r["mean"])) == set(A.P1_MEANS)
    for mode, ts in ((0, 32.0), (1, 0.0), (2, 16.0), (3, 32.0)):
        assert (r["tau_star"][c["mode"] == mode] == ts).all()
    for mode in (0, 2, 3):
        assert set(np.unique(r["mean"][c["mode"] == mode])) == set(A.P1_MEANS)
    assert (x[r["mean"] == 0.0] == 0).all()
    clear = r["margin"] > A.RTOL
    _report("P1", x != r["x"], clear)
    wrong = A.predict(c["level1"], c["T_cal"], c["T_star"], seed, swap_counter=True)
    _power("P1 customer <-> draw", ((x != wrong["x"]) & (wrong["margin"] > A.RTOL)).mean())
    wrong = A.predict(c["level1"], c["T_cal"], c["T_star"], seed, stream=A.STREAM_TRACK)
    _power("P1 stream 3", ((x != wrong["x"]) & (wrong["margin"] > A.RTOL)).mean())


@pytest.mark.parametrize("seed", A.SEEDS, ids=SEED_IDS)
def test_predict_spend_p2(seed):
    """P2: width 5 with spend; counts 0, 1, 2, 3 and about 600; sigma_s 0.5 and 0 (then spend is
    x exp(eta) to RTOL); eta in [-2, 3]; spend exactly 0 where x = 0; simulate_spend=False gives the
    same x."""
    c = A.predict_case_p2()
    eta = c["level1"][..., 4]
    assert eta.min() == -2.0 and eta.max() == 3.0
    x, sp = _predict_dev(c, seed, True, 0.5)
    r = A.predict(c["level1"], c["T_cal"], c["T_star"], seed, True, 0.5)
    assert {0, 1, 2, 3} <= set(np.unique(x)) and ((x > 500) & (x < 700)).any() and (x % 2 == 1).any()
    clear = r["margin"] > A.RTOL
    same = x == r["x"]
    assert (sp[x == 0] == 0.0).all()
    fail = ~same | (same & ~_close(sp, r["spend"]))
    _report("P2 sigma_s 0.5", fail, clear, spend=_dev(sp, r["spend"], clear & same & (x > 0)))
    x0, sp0 = _predict_dev(c, seed, True, 0.0)
    assert np.array_equal(x0, x)
    flat = x * np.exp(eta)
    _report("P2 sigma_s 0", ~_close(sp0, flat), clear, spend=_dev(sp0, flat, clear & (x > 0)))
    assert (sp0[x == 0] == 0.0).all()
    assert np.array_equal(_predict_dev(c, seed, False), x)
    assert np.array_equal(_predict_dev(c, seed), x)          # the bivariate entry on the same draws
    wrong = A.predict(c["level1"], c["T_cal"], c["T_star"], seed, True, 0.5, spend_slot0=A.SLOT_SPEND0 - 1)
    assert np.array_equal(wrong["x"], r["x"])
    _power("P2 spend slots from 2^20 - 1", (same & clear & ~_close(sp, wrong["spend"])).mean())


def test_predict_draw_stride_p3():
    """P3: n = 1 and 65,537 draws: the last draw is reached only by the stride over the grid's y extent."""
    c = A.predict_case_p3()
    x = _predict_dev(c, A.SEED_HI)
    r = A.predict(c["level1"], c["T_cal"], c["T_star"], A.SEED_HI)
    assert x.shape == (65537, 1)
    clear = r["margin"] > A.RTOL
    _report("P3", x != r["x"], clear)
    assert clear[0, 0] and clear[65535, 0] and clear[65536, 0]


# ---------------------------------------------------------------------------------------------
# track
# ---------------------------------------------------------------------------------------------
def _track_dev(c, seed):
    from mcmc_clv_model_amd.analysis import posterior_weekly_tracking
    return posterior_weekly_tracking(dict(level_1=[c["level1"]]), c["birth"], c["times"], seed=seed)


def _track_compare(name, c, seed, got, **wrong):
    r = A.track(c["level1"], c["birth"], c["times"], seed, **wrong)
    clear = (r["margin"] > A.RTOL).all(axis=0)           # a week is clear when every draw's count is
    fail = got.view(np.uint64) != r["inc_mean"].view(np.uint64)
    if not wrong:
        _report(name, fail, clear)
    return r, fail & clear


@pytest.mark.parametrize("seed", A.SEEDS, ids=SEED_IDS)
def test_track_window_ends_t1(seed):
    """T1: 1 draw, n = 130, weeks 1..78; births equal to a week (strict t > b), b + tau equal to a week
    (inclusive t <= b + tau), births before the first and after the last week.  Bitwise."""
    c = A.track_case_t1()
    b, t = c["birth"], c["times"]
    end = b + c["level1"][0, :, 2]
    assert np.isin(b, t).sum() > 20 and np.isin(end, t).sum() > 20 and (b < t[0]).any() and (b >= t[-1]).any()
    got = _track_dev(c, seed)
    r, _ = _track_compare("T1", c, seed, got)
    assert np.array_equal(got, r["inc"][0].astype(np.float64))
    assert r["rate"].max() >= 10.0 > r["rate"].min()     # both Poisson algorithms
    _, bad = _track_compare("T1", c, seed, got, birth_inclusive=True)
    _power("T1 t >= b", bad.mean())


@pytest.mark.parametrize("n_times", [113, 225])
def test_track_passes_t2(n_times):
    """T2: 113 / 225 weeks (two / three passes of 112), tied neighbouring times, customers active
    across the pass boundaries, 5 draws: inc_mean is bitwise the sequential sum over draws / n_draws."""
    c = A.track_case_t2(n_times)
    for seed in A.SEEDS:
        got = _track_dev(c, seed)
        r, _ = _track_compare(f"T2-{n_times}", c, seed, got)
        if n_times == 225:
            _, bad = _track_compare("T2-225", c, seed, got, pass_relative_week=True)
            _power("T2-225 pass-relative week index", bad.mean())


def test_track_large_rates_and_zero_weeks_t3():
    """T3: n = 1000, summed rates up to ~9e4 (PTRS), then weeks whose exact rate is 0: exactly 0 there."""
    c = A.track_case_t3()
    exact = A.track_exact_rates(c["level1"], c["birth"], c["times"])
    zero = (exact == 0.0).all(axis=0)
    assert zero.sum() >= 20 and exact.max() > 5e4
    for seed in A.SEEDS:
        got = _track_dev(c, seed)
        r, _ = _track_compare("T3", c, seed, got)
        clear = (r["margin"] > A.RTOL).all(axis=0)
        assert (got[zero & clear] == 0.0).all()


# ---------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------
def _gen_dev(c, seed):
    from mcmc_clv_model_amd.data import generate_pareto_abe
    return generate_pareto_abe(c["n"], c["T_cal"], c["T_star"], c["beta"], c["gamma"], covars=c["covars"], seed=seed)


def _star_cols(T_star):
    return [f"x_star{int(ts)}" if len(T_star) > 1 else "x_star" for ts in T_star]


def _gen_compare(name, c, seed, cbs, elog, report=True, **wrong):
    """Per customer: parameters against the model's own, then the model's event rules from the device's
    (lambda, tau).  Returns (fail, clear, devs)."""
    n, K = c["n"], c["beta"].shape[0]
    p = A.gen_params(n, c["beta"], c["gamma"], seed, c["covars"], lifetime_half=wrong.get("lifetime_half", 0))
    lam, mu, tau = (cbs[k].to_numpy() for k in ("lambda_true", "mu_true", "tau_true"))
    cov = np.column_stack([cbs[f"cov{j}"].to_numpy() for j in range(K)])
    fail = ~_close(lam, p["lam"]) | ~_close(mu, p["mu"]) | ~_close(tau, p["tau"])
    fail |= (cov.view(np.uint64) != p["cov"].view(np.uint64)).any(axis=1)      # pure arithmetic on u53: bitwise
    e = A.gen_events(lam, tau, c["T_cal"], c["T_star"], seed, gap_slot0=wrong.get("gap_slot0", A.GEN_SLOT_GAP0))
    clear = e["margin"] > A.RTOL
    fail |= (cbs["x"].to_numpy() != e["x"]) | (cbs["alive_true"].to_numpy() != e["alive"])
    for k, col in enumerate(_star_cols(c["T_star"])):
        fail |= cbs[col].to_numpy() != e["x_star"][k]
    fail |= ~_close(cbs["t_x"].to_numpy(), e["t_x"])
    assert np.array_equal(cbs["cust"].to_numpy(), np.arange(1, n + 1))
    assert (cbs["T_cal"].to_numpy() == np.max(c["T_cal"])).all()
    ec, et = elog["cust"].to_numpy(), elog["t"].to_numpy()
    assert (np.diff(ec) >= 0).all() and ec.min() >= 1 and ec.max() <= n      # customer-major, 1-based
    rows = np.bincount(ec.astype(np.int64) - 1, minlength=n)
    fail |= rows != e["n_events"]
    do, mo = np.concatenate([[0], np.cumsum(rows)]), np.concatenate([[0], np.cumsum(e["n_events"])])
    dev_t = 0.0
    for i in np.flatnonzero(rows == e["n_events"]):
        a, b = et[do[i]:do[i + 1]], e["elog_t"][mo[i]:mo[i + 1]]
        ok = _close(a, b)
        fail[i] |= not ok.all()
        if clear[i]:
            dev_t = max(dev_t, _dev(a, b, np.ones(a.size, bool)))
    devs = dict(lam=_dev(lam, p["lam"], clear), mu=_dev(mu, p["mu"], clear), tau=_dev(tau, p["tau"], clear),
                t_x=_dev(cbs["t_x"].to_numpy(), e["t_x"], clear & ~fail), elog_t=dev_t)
    if report:
        _report(name, fail, clear, **devs)
    return fail, clear, e


@pytest.mark.parametrize("seed", A.SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("name", list(A.gen_cases()))
def test_generator_matches_model(name, seed):
    """G1 K = 3 generated, scalar T_cal, two horizons; G2 K = 6 generated (three covariate blocks), a
    per-customer T_cal in {8, 20.5, 32}, eight unsorted horizons including 0; G3 supplied covariates
    with / without the ones column, and K = 1; G4 lambda ~ 50 over 104 weeks (thousands of gap blocks per customer)
    and a mu so large that only the t = 0 event survives."""
    c = A.gen_cases()[name]
    cbs, elog = _gen_dev(c, seed)
    fail, clear, e = _gen_compare(name, c, seed, cbs, elog)
    if name == "G2":
        assert set(np.unique(c["T_cal"])) == {8.0, 20.5, 32.0} and 0.0 in c["T_star"] and len(c["T_star"]) == 8
        assert (cbs["x_star0"] == 0).all() and (cbs["x_star64"] >= cbs["x_star32"]).all() and (cbs["x_star64"] > 0).any()
    if name == "G3_supplied":      # the wrapper adds the ones column: the same run as with it
        cbs1, elog1 = _gen_dev(A.gen_cases()["G3_supplied_ones"], seed)
        assert cbs.equals(cbs1) and elog.equals(elog1)
    if name == "G4_busy":
        assert np.median(e["n_events"]) > 4000 and e["n_events"].sum() == len(elog)   # > 2,000 gap blocks each
    if name == "G4_dead":
        T_zero = np.max(c["T_cal"]) - np.broadcast_to(c["T_cal"], (c["n"],))
        assert (cbs["x"] == 0).all() and np.array_equal(cbs["t_x"].to_numpy(), T_zero) and len(elog) == c["n"]
        assert np.array_equal(elog["t"].to_numpy(), T_zero) and not cbs["alive_true"].any()
    if name == "G1":
        bad, clr, _ = _gen_compare(name, c, seed, cbs, elog, report=False, gap_slot0=15)
        _power("G1 gap slots from 15", (bad & clr).mean())
        bad, clr, _ = _gen_compare(name, c, seed, cbs, elog, report=False, lifetime_half=1)
        _power("G1 lifetime from (z, w)", (bad & clr).mean())


# ---------------------------------------------------------------------------------------------
# exact statistics, no RNG
# ---------------------------------------------------------------------------------------------
def _summary_column(rng, nd, n):
    """(nd, n) values per customer kind i % 4: signed magnitudes 1e-300 .. 1e300; an all-equal
    segment; ties among three values (one negative); positive, well behaved.  No NaN, no zeros."""
    a = np.empty((nd, n))
    for i in range(n):
        kind = i % 4
        if kind == 0:
            a[:, i] = rng.choice([-1.0, 1.0], nd) * 10.0 ** rng.uniform(-300.0, 300.0, nd)
        elif kind == 1:
            a[:, i] = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-300.0, 300.0)
        elif kind == 2:
            a[:, i] = rng.choice(np.array([-0.25, 1.5, 1e300]) * rng.uniform(0.5, 1.0), nd)
        else:
            a[:, i] = np.exp(rng.normal(-3.0, 1.0, nd))
    return a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("nd", [1, 2, 3, 40, 41, 257])
def test_level1_summary_edge_shapes(nd):
    """n_draws in {1, 2, 3, 40, 41, 257} x n in {1, 255, 257} x widths 4 and 5 x mu_cap in {0.05, 1e-300,
    inf}: percentiles bitwise np.percentile(method="linear"), means bitwise the sequential sum over
    draws / n_draws (the order spelled out with np.add.accumulate)."""
    for n, w, a in _summary_cases(nd):
        for cap in SUMMARY_CAPS:
            _summary_check(a, cap, (nd, n, w, cap))


SUMMARY_CAPS = (0.05, 1e-300, math.inf)


def _summary_cases(nd):
    """(n, w, level-1 array (nd, n, w)) of test_level1_summary_edge_shapes, from one generator in order."""
    rng = np.random.default_rng(1000 + nd)
    for n in (1, 255, 257):
        for w in (4, 5):
            a = np.empty((nd, n, w))
            for col in range(w):
                a[..., col] = _summary_column(rng, nd, n)
            assert not np.isnan(a).any() and (a != 0).all()
            yield n, w, a


def _summary_check(a, cap, label):
    """level1_summary(a, cap): percentiles bitwise np.percentile(method="linear"), means bitwise the
    sequential sum over draws / n_draws.  Returns the number of (column, customer) entries compared."""
    from mcmc_clv_model_amd.analysis import level1_summary
    nd, _, w = a.shape
    mean = lambda v: np.add.accumulate(v, axis=0)[-1] / nd  # noqa: E731
    s = level1_summary(dict(level_1=[a]), mu_cap=cap)
    want = dict(mean_lambda=mean(a[..., 0]), mean_mu=mean(a[..., 1]), mean_tau=mean(a[..., 2]),
                mean_z=mean(a[..., 3]), mean_mu_capped=mean(np.minimum(a[..., 1], cap)),
                lambda_p025=np.percentile(a[..., 0], 2.5, axis=0, method="linear"),
                lambda_p975=np.percentile(a[..., 0], 97.5, axis=0, method="linear"),
                mu_p025=np.percentile(a[..., 1], 2.5, axis=0, method="linear"),
                mu_p975=np.percentile(a[..., 1], 97.5, axis=0, method="linear"))
    if w == 5:
        want["mean_eta"] = mean(a[..., 4])
    assert set(want) == set(s.columns)
    for k, v in want.items():
        bad = _bits(s[k].to_numpy()) != _bits(v)
        assert not bad.any(), (k, label, int(bad.sum()), np.flatnonzero(bad)[:5])
    return sum(v.size for v in want.values())


@pytest.mark.parametrize("batch", [1, 100, 256])
def test_level1_summary_customer_batches(monkeypatch, batch):
    """summary_dev<double> with more than one customer batch (CLV_SUMMARY_BATCH; the natural batch is
    2^27 / n_draws customers): the nd = 41, n = 257, width 5 case of test_level1_summary_edge_shapes in
    batches of 1 (257 batches), 100 (100, 100, 57: SegSorter::sort with nc != filled, offsets refilled and
    the temporary storage of the larger count reused) and 256 (a last batch of one).  i0 > 0 in
    gather_kernel and row0 = i0 in launch_percentiles.  Same reference, bit for bit."""
    from mcmc_clv_model_amd import _lib
    n, w, a = list(_summary_cases(41))[-1]
    assert (n, w) == (257, 5)
    monkeypatch.setenv(_lib.SUMMARY_BATCH_ENV, str(batch))
    count = sum(_summary_check(a, cap, (41, n, w, cap, batch)) for cap in SUMMARY_CAPS)
    monkeypatch.delenv(_lib.SUMMARY_BATCH_ENV)
    print(f"level1_summary CLV_SUMMARY_BATCH={batch}: {count} entries, 0 differ from numpy in any bit")


def test_summary_pct_sink_customer_batches(monkeypatch):
    """summary_dev<float> (the "summary+pct" sink's float32 keys, gather_q_kernel) at the D = 2
    configuration of test_summary_pct_sink_matches_full_sink, n = 1500, in batches of 1 and 100 customers:
    bitwise the same sampler's unbatched summary (which that test holds to the full sink)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    from tests.helpers import cdnow
    p = build_problem(cdnow("abe", 1500), ["first_sales_scaled"], D=2)
    with HipSampler(p, mcmc=301, burnin=40, thin=3, chains=3, seed=11, draw_sink="summary+pct") as s:
        s.run(341)
        whole = s.level1_summary(_lib.SUMMARY_MU_CAP)
        assert whole.shape == (1500, len(_lib.L1_STATS)) and np.isfinite(whole).all()
        lo, hi = whole[:, _lib.L1_STATS.index("lambda_p025")], whole[:, _lib.L1_STATS.index("lambda_p975")]
        assert (lo < hi).all() and len(np.unique(lo)) > 1400          # per-customer values, not one row repeated
        for batch in (1, 100):
            monkeypatch.setenv(_lib.SUMMARY_BATCH_ENV, str(batch))
            got = s.level1_summary(_lib.SUMMARY_MU_CAP)
            monkeypatch.delenv(_lib.SUMMARY_BATCH_ENV)
            diff = int((_bits(got) != _bits(whole)).sum())
            print(f"summary+pct CLV_SUMMARY_BATCH={batch}: {diff} of {whole.size} entries differ from the unbatched summary")
            assert diff == 0, batch


@pytest.mark.parametrize("n", [1, 255, 257])
def test_chain_total_loglik_edge_shapes(n):
    """n in {1, 255, 257}, 3 draws, x including 0 and 10,000: within RTOL * sum |component| of a
    math.fsum float64 reference."""
    from mcmc_clv_model_amd.analysis import chain_total_loglik
    rng = np.random.default_rng(2000 + n)
    nd = 3
    x = rng.integers(0, 40, n)
    x[::7] = 0
    x[::5] = 10_000
    T = rng.uniform(20.0, 40.0, n)
    a = np.empty((nd, n, 4))
    a[..., 0] = np.exp(rng.normal(-1.0, 2.0, (nd, n)))
    a[..., 1] = np.exp(rng.normal(-3.0, 2.0, (nd, n)))
    a[..., 2] = rng.uniform(0.0, 60.0, (nd, n))
    a[..., 3] = rng.choice([0.0, 0.5, 0.75, 1.0], (nd, n))
    totals, mags = [], []
    for d in range(nd):
        lam, mu, tau, z = a[d, :, 0], a[d, :, 1], a[d, :, 2], (a[d, :, 3] > 0.5).astype(np.float64)
        comp = [x * np.log(lam), (1 - z) * np.log(mu), -(lam * (z * T + (1 - z) * tau)), -(mu * (z * T + (1 - z) * tau)),
                -gammaln(x + 1.0)]
        totals.append(math.fsum(np.concatenate(comp)))
        mags.append(math.fsum(np.abs(np.concatenate(comp))))
    ref, mag = math.fsum(totals) / nd, math.fsum(mags) / nd
    got = chain_total_loglik([a], pd.DataFrame(dict(x=x, T_cal=T)))
    print(f"chain_total_loglik n = {n}: |got - ref| / sum |component| = {abs(got - ref) / mag:.2e}")
    assert abs(got - ref) <= A.RTOL * mag


# ---------------------------------------------------------------------------------------------
# more draws than workgroups: loglik_kernel and track_kernel launch min(n_draws, 2^20) workgroups and
# stride over the draws
# ---------------------------------------------------------------------------------------------
STRIDE_GRID = 1 << 20
STRIDE_DRAWS = STRIDE_GRID + 3


def test_chain_total_loglik_draw_stride():
    """2^20 + 3 draws, n = 2, width 4 (64 MiB): draws 2^20 .. 2^20 + 2 are reached only by the stride of
    loglik_kernel.  Their lambda is 100 times larger, so that their share of the mean exceeds the
    tolerance by orders of magnitude (asserted from the reference before the device runs).  Reference:
    float64 per-draw totals (10 terms each) combined with math.fsum; tolerance RTOL * sum |component|
    as in test_chain_total_loglik_edge_shapes."""
    from mcmc_clv_model_amd.analysis import chain_total_loglik
    rng = np.random.default_rng(2002)
    nd, n = STRIDE_DRAWS, 2
    x = rng.integers(0, 40, n)
    x[::7] = 0
    x[::5] = 10_000
    T = rng.uniform(20.0, 40.0, n)
    a = np.empty((nd, n, 4))
    a[..., 0] = np.exp(rng.normal(-1.0, 2.0, (nd, n)))
    a[..., 1] = np.exp(rng.normal(-3.0, 2.0, (nd, n)))
    a[..., 2] = rng.uniform(0.0, 60.0, (nd, n))
    a[..., 3] = rng.choice([0.0, 0.5, 0.75, 1.0], (nd, n))
    a[STRIDE_GRID:, :, 0] *= 100.0
    lam, mu, tau, z = a[..., 0], a[..., 1], a[..., 2], (a[..., 3] > 0.5).astype(np.float64)
    w = z * T + (1 - z) * tau
    comp = np.concatenate([x * np.log(lam), (1 - z) * np.log(mu), -(lam * w), -(mu * w),
                           np.broadcast_to(-gammaln(x + 1.0), (nd, n))], axis=1)
    assert comp.shape == (nd, 5 * n)
    totals, mags = comp.sum(axis=1), np.abs(comp).sum(axis=1)
    ref, mag = math.fsum(totals) / nd, math.fsum(mags) / nd
    tol = A.RTOL * mag
    # what the strided draws add to the mean, and what a kernel that left them at ordinary values would miss
    strided = abs(math.fsum(totals[STRIDE_GRID:])) / nd
    shift = abs(math.fsum(totals[STRIDE_GRID:]) - 3 * math.fsum(totals[:STRIDE_GRID]) / STRIDE_GRID) / nd
    print(f"chain_total_loglik stride: the three strided draws carry {strided:.3e} of the mean "
          f"({shift:.3e} more than three ordinary draws); tolerance {tol:.3e}")
    assert strided >= 1e3 * tol and shift >= 1e3 * tol
    got = chain_total_loglik([a], pd.DataFrame(dict(x=x, T_cal=T)))
    print(f"chain_total_loglik n_draws = 2^20 + 3: |got - ref| / sum |component| = {abs(got - ref) / mag:.2e}")
    assert abs(got - ref) <= tol


def test_track_draw_stride():
    """2^20 + 3 draws, n = 2, one week: tau = 0 everywhere (nobody is active, the rate and the increment
    are exactly 0) but in draws {0, 2^20 - 1, 2^20, 2^20 + 2}, whose summed rate is about 600.  The mean
    is the sum of those four Poisson draws of the model (counter (week 0, flat draw, attempt, 3)) over
    n_draws, bit for bit; the two draws past 2^20 are reached only by the stride of track_kernel and
    carry about half of it."""
    nd, n = STRIDE_DRAWS, 2
    special = np.array([0, STRIDE_GRID - 1, STRIDE_GRID, STRIDE_GRID + 2])
    lam, tau = np.full((nd, n), 0.25), np.zeros((nd, n))
    lam[special] = np.array([[280.0, 330.0], [295.5, 301.25], [310.0, 287.0], [305.75, 299.0]])
    tau[special] = 5.0
    c = dict(level1=A._l1_track(lam, tau), birth=np.zeros(n), times=np.array([1.0]))
    rate = A.track_rates(c["level1"][special], c["birth"], c["times"])
    others = np.array([1, STRIDE_GRID - 2, STRIDE_GRID + 1])
    assert (A.track_rates(c["level1"][others], c["birth"], c["times"]) == 0.0).all()
    assert rate.shape == (4, 1) and (rate > 550.0).all() and (rate < 650.0).all()
    inc, margin = A.poisson(rate, A.SEED_HI, 0, special[:, None], 0, A.STREAM_TRACK)
    assert (margin > A.RTOL).all() and (inc > 400).all()
    want = np.add.accumulate(inc[:, 0].astype(np.float64))[-1] / nd
    past = float(inc[2:, 0].sum()) / nd
    assert 0.4 * want < past < 0.6 * want
    got = _track_dev(c, A.SEED_HI)
    print(f"track n_draws = 2^20 + 3: the four active draws {inc[:, 0].tolist()}, mean got {got[0]!r}, want {want!r} "
          f"({past / want:.1%} of it past draw 2^20)")
    assert got.shape == (1,) and _bits(got)[0] == _bits(np.array([want]))[0]

"""Customer lifetime value and customer equity on the GPU (csrc/ltv.hip) against the float64 model
tests/ltv_ref.py.

The infinite horizon is multiply and divide only, so every statistic but survival_1yr must equal the
model bit for bit: per-customer sums in draw order, numpy's std and percentiles, per-draw sums in the
fixed order of pnbd_ref.device_sum.  The finite horizon and survival_1yr go through expm1 / exp,
where the device's and glibc's differ by a few ulp: bounds of 64 ulp (the project's standing floor,
tests/test_gpu_pnbd.py) relative to the scales named in ltv_ref.finite_horizon_errors.

Measured on an MI355X (finite horizon, N = 257, S = 1000, largest over H in {39, 520} and delta in
{0, log1p(0.15) / 52}; in ulp = 2^-52): value_mean 1.5, residual_mean 1.6, percentiles at most 1.8,
value_sd 0.9, residual_sd 1.2, equity 1.8, value_total 1.5, survival_1yr 1.4."""

import numpy as np
import pytest

from tests import ltv_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu

DELTA = float(np.log1p(0.15) / 52.0)
SURV = R.STATS.index("survival_1yr")
SD_COLS = [R.STATS.index("value_sd"), R.STATS.index("residual_sd")]
EXACT_COLS = [j for j in range(len(R.STATS)) if j != SURV]


def device(l1, **kw):
    """(customers, draws) arrays of analysis.lifetime_value on the stacked array l1 (as one chain)."""
    from mcmc_clv_model_amd.analysis import lifetime_value
    out = lifetime_value({"level_1": [l1]}, **kw)
    assert list(out["customers"].columns) == list(R.STATS) and list(out["draws"].columns) == list(R.DRAW_STATS)
    return out["customers"].to_numpy(), out["draws"].to_numpy()


def assert_exact(cust, draws, mc, md, S):
    cols = EXACT_COLS if S > 1 else [j for j in EXACT_COLS if j not in SD_COLS]
    for j in cols:
        assert np.array_equal(bits(cust[:, j]), bits(mc[:, j])), (R.STATS[j], np.abs(cust[:, j] - mc[:, j]).max())
    if S == 1:
        assert np.isnan(cust[:, SD_COLS]).all() and np.isnan(mc[:, SD_COLS]).all()
    for q in range(len(R.DRAW_STATS)):
        assert np.array_equal(bits(draws[:, q]), bits(md[:, q])), R.DRAW_STATS[q]
    # survival_1yr: the device's exp against glibc's, a mean of S terms in (0, 1]
    assert np.abs(cust[:, SURV] - mc[:, SURV]).max() <= 64 * R.ULP


def shapes():
    from mcmc_clv_model_amd import _lib
    t, b, t2 = _lib.LTV_TILE_DRAWS, _lib.LTV_BLOCK, _lib.LTV_SD_TILE_DRAWS
    out = [(n, s) for n in (1, b - 1, b, b + 1) for s in (1, 2, 37)]
    out += [(b + 1, s) for s in (t - 1, t, t + 1, 2 * t + 1) if s > 0]      # the transposing tile's edge
    out += [(b + 1, s) for s in (t2 - 1, t2, t2 + 1, 2 * t2 + 1) if s > 0]  # the sd kernel's tile edge
    out += [(65, t2 + 1), (63, 2 * t2)]                                     # its 64-customer wavefront's edge
    out += [(b * b + 1, 2)]                                                 # more than 256 block partials
    return sorted(set(out))


@pytest.mark.parametrize("variant", ["w4", "w4_monetary", "w5"])
@pytest.mark.parametrize("shape", shapes(), ids=lambda s: f"N{s[0]}-S{s[1]}")
def test_infinite_horizon_bit_for_bit(shape, variant):
    N, S = shape
    width = 5 if variant == "w5" else 4
    l1 = R.synth_level1(S, N, width, seed=7)
    monetary = np.random.default_rng(N).gamma(2.0, 20.0, N) if variant == "w4_monetary" else None
    omega2 = 0.3 if variant == "w5" else 0.0
    kw = dict(monetary=monetary) if monetary is not None else {}
    cust, draws = device(l1, omega2=omega2, **kw)
    mc, md = R.model(l1, DELTA, None, monetary, float(np.exp(omega2 / 2.0)))
    assert_exact(cust, draws, mc, md, S)


@pytest.fixture(scope="module")
def finite_l1():
    return R.synth_level1(1000, 257, 4, seed=21)


@pytest.mark.parametrize("rate", [0.0, 0.15])
@pytest.mark.parametrize("H", [39.0, 520.0])
def test_finite_horizon_and_survival(finite_l1, H, rate):
    delta = float(np.log1p(rate) / 52.0)
    cust, draws = device(finite_l1, horizon=H, discount_rate=rate)
    err, mc, md = R.finite_horizon_errors(cust, draws, finite_l1, delta, H)
    for k, v in err.items():
        print(f"H={H:g} delta={delta:.4g} {k}: {v / R.ULP:.2f} ulp")
    # the columns that do not pass through expm1 / exp stay exact
    for j in (R.STATS.index("p_alive"), R.STATS.index("lifetime_yrs")):
        assert np.array_equal(bits(cust[:, j]), bits(mc[:, j]))
    for q in (R.DRAW_STATS.index("n_alive"), R.DRAW_STATS.index("mu_share")):
        assert np.array_equal(bits(draws[:, q]), bits(md[:, q]))
    if rate == 0.0 and H == 39.0:   # the reference's xstar_pred formula per draw, through its posterior mean
        lam, mu, z = finite_l1[..., 0], finite_l1[..., 1], finite_l1[..., 3]
        xstar = (z * (lam / mu) * (1.0 - np.exp(-mu * 39.0))).mean(axis=0)
        assert np.allclose(cust[:, R.STATS.index("residual_mean")], xstar, rtol=1e-11, atol=0)
    for k, v in err.items():
        assert v <= 64 * R.ULP, (k, v / R.ULP)


def test_ties_and_point_masses():
    S, N = 37, 257
    l1 = R.synth_level1(S, N, 5, seed=3)
    l1[:, 5, :] = l1[0, 5, :]           # a customer whose draws are all the same
    dead, alive = l1.copy(), l1.copy()
    dead[..., 3], alive[..., 3] = 0.0, 1.0
    cd, dd = device(dead)
    assert np.array_equal(bits(cd[:, 5:10]), bits(np.zeros((N, 5)))) and np.all(cd[:, 10] == 0.0)
    assert np.array_equal(bits(dd[:, [0, 2]]), bits(np.zeros((S, 2))))
    ca, da = device(alive)
    assert np.array_equal(bits(ca[:, 5:10]), bits(ca[:, 0:5])) and np.all(ca[:, 10] == 1.0)
    assert np.array_equal(bits(da[:, 0]), bits(da[:, 1])) and np.all(da[:, 2] == float(N))
    v5 = l1[0, 5, 0] * l1[0, 5, 4] / (l1[0, 5, 1] + DELTA)
    c, _ = device(l1)
    mc, md = R.model(l1, DELTA)
    # S equal terms: the sequential sum rounds, so the mean is the model's (sum / S), the percentiles
    # are the value itself, and subtracting the mean first leaves an sd within the S adds' worst
    # rounding of the mean, S ulp (E[x^2] - mean^2 would leave about sqrt(S ulp) = 1e-7 of the value)
    assert bits(c[5, 0]) == bits(mc[5, 0]) and np.all(c[5, 2:5] == v5)
    assert bits(c[5, 1]) == bits(mc[5, 1]) and c[5, 1] <= S * R.ULP * v5
    assert_exact(c, _, mc, md, S)
    # a constant whose sum is exact: mean exact, sd exactly 0
    l1[:, 6, 0], l1[:, 6, 1], l1[:, 6, 4] = 0.5, 0.25, 8.0
    c, _ = device(l1, discount_rate=0.0)
    assert c[6, 0] == 16.0 and c[6, 1] == 0.0 and np.all(c[6, 2:5] == 16.0)


def test_extremes():
    S, N = 17, 300
    l1 = R.synth_level1(S, N, 4, seed=9)
    g = np.random.default_rng(4)
    l1[..., 1] = np.where(g.random((S, N)) < 0.5, np.exp(-70.0), np.exp(5.0))
    l1[..., 0] = np.where(g.random((S, N)) < 0.5, np.exp(-70.0), np.exp(70.0))
    from mcmc_clv_model_amd.analysis import lifetime_value
    out = lifetime_value({"level_1": [l1]}, discount_rate=0.0)
    cust, draws = out["customers"].to_numpy(), out["draws"].to_numpy()
    assert out["delta"] == 0.0
    mc, md = R.model(l1, 0.0)
    assert not np.isnan(cust).any() and not np.isnan(draws).any() and not np.isnan(mc).any()
    assert np.array_equal(np.isinf(cust), np.isinf(mc)) and np.array_equal(np.isinf(draws), np.isinf(md))
    assert np.all(draws[:, 3] == 1.0)                       # mu / (mu + 0)
    assert_exact(cust, draws, mc, md, S)
    one = lifetime_value({"level_1": [l1[:1]]}, discount_rate=0.0)["customers"].to_numpy()
    assert np.isnan(one[:, SD_COLS]).all() and not np.isnan(np.delete(one, SD_COLS, axis=1)).any()


def test_geometry_independence(monkeypatch):
    from mcmc_clv_model_amd import _lib
    b = _lib.LTV_BLOCK
    S, N = 37, 3 * b + 41
    l1 = R.synth_level1(S, N, 5, seed=13)
    c0, d0 = device(l1, horizon=520.0)
    for batch in (1, b, 2 * b):
        monkeypatch.setenv(_lib.LTV_BATCH_ENV, str(batch))
        c1, d1 = device(l1, horizon=520.0)
        assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(d0), bits(d1)), batch
    c2, d2 = device(l1)                                       # still batched: against the model
    monkeypatch.delenv(_lib.LTV_BATCH_ENV)
    mc, md = R.model(l1, DELTA)
    assert_exact(c2, d2, mc, md, S)


RUN = dict(mcmc=40, burnin=20, thin=2, chains=2, seed=5)


def frames_equal(a, b):
    for k in ("customers", "draws"):
        assert list(a[k].columns) == list(b[k].columns)
        assert np.array_equal(bits(a[k].to_numpy()), bits(b[k].to_numpy())), k
    assert a["delta"] == b["delta"] and a["horizon"] == b["horizon"]


@pytest.mark.parametrize("D", [2, 3])
def test_sampler_path_and_drop_in(D):
    from mcmc_clv_model_amd import _lib, mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    df = cdnow("abe", n=300)
    covs = ["gender_F"] if D == 3 else []
    kw = dict(horizon=104.0) if D == 2 else dict(omega2=0.2)
    p = build_problem(df, covs, D=D)
    with HipSampler(p, n_mh_steps=20, **RUN) as s:
        with pytest.raises(_lib.ClvError, match="-3"):       # CLV_ESTATE: the run has not stored its draws
            s.lifetime_value()
        s.run(60)
        dev = s.lifetime_value(**kw)
        l1, l2, _ = s.read_draws()
    draws = dict(level_1=list(l1), level_2=list(l2))
    host = A.lifetime_value(draws, **kw)
    frames_equal(dev, host)
    assert dev["customers"].shape == (300, 13) and dev["draws"].shape == (2 * 20, 4)
    assert np.isfinite(dev["customers"].to_numpy()).all() and np.isfinite(dev["draws"].to_numpy()).all()
    mc, md = R.model(np.concatenate(list(l1)), host["delta"], kw.get("horizon"), None,
                     float(np.exp(kw.get("omega2", 0.0) / 2.0)))
    if D == 3:
        assert_exact(host["customers"].to_numpy(), host["draws"].to_numpy(), mc, md, 40)
    fn = mcmc_draw_parameters_rfm_m if D == 3 else mcmc_draw_parameters
    out = fn(df, covs, trace=0, lifetime_value=kw, **RUN)
    assert np.array_equal(bits(np.stack(out["level_1"])), bits(l1))
    frames_equal(out["lifetime_value"], host)
    assert "lifetime_value" not in fn(df, covs, trace=0, **RUN)
    # several devices (here one device twice): the array path on devices[0], the same frames
    for shard in ("chains", "customers"):
        multi = fn(df, covs, trace=0, lifetime_value=kw, devices=[0, 0], shard=shard, **RUN)
        frames_equal(multi["lifetime_value"], host)
    with pytest.raises(ValueError):
        fn(df, covs, trace=0, draw_sink="summary", lifetime_value=True, **RUN)
    with HipSampler(p, n_mh_steps=20, draw_sink="summary", **RUN) as s:
        s.run(60)
        with pytest.raises(_lib.ClvError, match="-3"):
            s.lifetime_value()
    if D == 3:      # elasticities end to end: host arithmetic on the pinned device sums
        e = A.lifetime_value_elasticities(out, covs)
        l2s = np.concatenate(out["level_2"])
        md_inf = R.model(np.concatenate(out["level_1"]), DELTA)[1]
        want = R.elasticities(l2s, md_inf[:, R.DRAW_STATS.index("mu_share")], 1, 3)
        for comp in ("purchase_rate", "lifetime", "spend", "total"):
            v = want[1, comp]
            got = e.loc[("gender_F", comp)]
            assert bits(got["mean"]) == bits(v.mean())
            assert bits(got["p025"]) == bits(np.percentile(v, 2.5)) and bits(got["p975"]) == bits(np.percentile(v, 97.5))
        e2 = A.lifetime_value_elasticities(out, covs, ltv=A.lifetime_value(out))
        assert np.array_equal(bits(e.to_numpy()), bits(e2.to_numpy()))
        with pytest.raises(ValueError):
            A.lifetime_value_elasticities(out, covs, ltv=A.lifetime_value(out, horizon=52.0))
        ce = A.customer_equity(out["lifetime_value"])
        assert ce["mean"][0] == out["lifetime_value"]["draws"]["equity"].to_numpy().mean()

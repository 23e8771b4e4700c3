"""Rank-normalised diagnostics on the GPU (csrc/diag.hip: clv_rank_diagnostics, clv_debug_zscale)
against the numpy / scipy yardstick (tests/diagnostics_rank_ref.py).

Tolerances (derived, not guessed).  Ranks are exact (multiples of 0.5).  z is compared with scipy's
ndtri of the same argument within EPS_Z, four times the largest relative error measured over every
attainable rank, half-ranks included, for S in {16, 42, 64, 4000, 8192}
(test_zscale_error_over_every_attainable_rank; measured: see EPS_Z_MEASURED).  The truncation lag is
compared exactly (the yardstick's decision margins are >= 1e-6 on every input set,
tests/test_rank_diagnostics_cpu.py); hdi_lo, hdi_hi and the median bit for bit (picks, or one exact
average, of data values).  R-hats within relative 1e-11 + 4 EPS_Z; ess_q05, ess_q95, ess_sd, ess_tail
and mcse_sd within relative 1e-8 (the derivation of tests/test_gpu_diagnostics.py: their transformed
series are exact or carry one rounding); ess_bulk within relative 1e-8 + 32 h EPS_Z (the same
derivation with the error of z, relative EPS_Z on values of a few units, added to each rho(t)).

Logged series.  The statistics are functions of the logged values, and the device's log and numpy's
differ in the last bit for a few percent of arguments.  That is enough to move a pick (HDI, median)
by one ulp and, through a tie made or broken among |y - med|, a folded R-hat of 40 draws by 1e-4.  So
for logged series the yardstick is given the values the device ranks: ``device_logged`` reads the
device's own log of every logged draw back through the public entry (the median of a constant series
is that constant), and checks them against numpy's within 2 ulp.  Every comparison then holds as
stated above, bit-for-bit picks included."""
import ctypes
import functools

import numpy as np
import pytest

from tests import diagnostics_rank_ref as K
from tests import diagnostics_ref as R
from tests.helpers import bits, cdnow

pytestmark = pytest.mark.gpu

# Largest relative error of the device's z against scipy.special.ndtri over every attainable rank
# (Wichura's AS241 / PPND16 in csrc/fastmath.h), as printed by
# test_zscale_error_over_every_attainable_rank on an MI355X, and the bound the tests use.
EPS_Z_MEASURED = 8.9e-16
EPS_Z = 4 * EPS_Z_MEASURED
assert EPS_Z <= 1e-12

EXACT = (K.LAG_BULK,)
BITWISE = (K.HDI_LO, K.HDI_HI, K.MEDIAN)
RHATS = (K.RHAT, K.RHAT_BULK, K.RHAT_FOLDED)
ESS_PLAIN = (K.ESS_Q05, K.ESS_Q95, K.ESS_TAIL, K.ESS_SD, K.MCSE_SD)


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def gpu_rank(L, arr, period=1, log_mask=0, hdi_prob=0.94):
    """One clv_rank_diagnostics call on arr (m, n, n_series)."""
    from mcmc_clv_model_amd._lib import check, dptr
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    m, n, ns = arr.shape
    out = np.full((ns, len(K.STATS)), -7.0)
    check(L.clv_rank_diagnostics(-1, dptr(arr), m, n, ns, period, log_mask, hdi_prob, dptr(out)))
    return out


def gpu_zscale(L, arr, folded):
    """clv_debug_zscale on arr (m, n, n_series): (ranks, z), each (n_series, 2 m, h)."""
    from mcmc_clv_model_amd._lib import check, dptr
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    m, n, ns = arr.shape
    rk = np.full((ns, 2 * m, n // 2), -7.0)
    z = np.full((ns, 2 * m, n // 2), -7.0)
    check(L.clv_debug_zscale(-1, dptr(arr), m, n, ns, int(folded), dptr(rk), dptr(z)))
    return rk, z


def device_logged(L, arr, period, log_mask):
    """arr (m, n, n_series) with every series that log_mask selects replaced by the device's own log of
    it: each value goes through clv_rank_diagnostics as a constant, logged series of 1 x 8 draws, whose
    median is log(value) as the gather kernel computes it (NaN where that is not finite)."""
    arr = np.array(arr, dtype=np.float64)
    cols = [k for k in range(arr.shape[2]) if (log_mask >> (k % period)) & 1]
    if not cols:
        return arr
    vals = arr[:, :, cols].ravel()
    got = gpu_rank(L, np.broadcast_to(vals, (1, 8, vals.size)), period=1, log_mask=1)
    logged = got[:, K.MEDIAN]
    assert np.array_equal(bits(logged), bits(got[:, K.HDI_LO])) and np.array_equal(bits(logged), bits(got[:, K.HDI_HI]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.log(vals)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(logged), ok)
    ulp = np.abs(logged[ok] - ref[ok]) / np.spacing(np.abs(ref[ok]))
    print(f"device log: {vals.size} values, {float(np.mean(logged[ok] != ref[ok])):.2%} differ from numpy's, at most {ulp.max():.1f} ulp")
    assert ulp.max() <= 2.0
    arr[:, :, cols] = logged.reshape(arr.shape[0], arr.shape[1], len(cols))
    return arr


def unsplit(s, n, middle=0.5):
    """Inverse of K.split_chains: (2 m, h) -> (m, n), the middle draw of an odd n set to ``middle``."""
    M, h = s.shape
    y = np.full((M // 2, n), middle)
    y[:, :h] = s[0::2]
    y[:, n - h:] = s[1::2]
    return y


def z_rel_error(z, r, S):
    want = K.ndtri(K.zscale_arg(r, S))
    zero = want == 0
    assert (z[zero] == 0).all()  # the middle rank (S + 1) / 2 maps to exactly 0
    return float(np.max(np.abs(z[~zero] / want[~zero] - 1.0))) if (~zero).any() else 0.0


def assert_rank_parity(got, want, h, label):
    assert got.shape == want.shape
    for k, st in enumerate(K.STATS):
        assert np.array_equal(np.isnan(got[:, k]), np.isnan(want[:, k])), f"{label}: NaN pattern of {st}"
    rel = {}
    for k, st in enumerate(K.STATS):
        ok = ~np.isnan(want[:, k])
        g, w = got[ok, k], want[ok, k]
        if k in EXACT:
            rel[st] = int((g != w).sum())
        elif k in BITWISE:
            rel[st] = int((bits(g) != bits(w)).sum())
        else:
            rel[st] = float(np.max(np.abs(g / w - 1.0))) if len(w) else 0.0
    print(f"{label}: mismatches / max relative error", {s: (v if isinstance(v, int) else f"{v:.2e}") for s, v in rel.items()})
    for k, st in enumerate(K.STATS):
        ok = ~np.isnan(want[:, k])
        g, w = got[ok, k], want[ok, k]
        if k in EXACT:
            assert np.array_equal(g, w), f"{label}: {st}"
        elif k in BITWISE:
            assert np.array_equal(bits(g), bits(w)), f"{label}: {st}"
        elif k in RHATS:
            np.testing.assert_allclose(g, w, rtol=1e-11 + 4 * EPS_Z, atol=0, err_msg=f"{label}: {st}")
        elif k in ESS_PLAIN:
            np.testing.assert_allclose(g, w, rtol=1e-8, atol=0, err_msg=f"{label}: {st}")
        else:
            assert k == K.ESS_BULK
            np.testing.assert_allclose(g, w, rtol=1e-8 + 32 * h * EPS_Z, atol=0, err_msg=f"{label}: {st}")


def crafted_series():
    """[(label, y (m, n))]: the tie and shape cases of the rank transform."""
    rng = np.random.default_rng(23)
    blocks = np.repeat(np.arange(10.0), 4).reshape(2, 20)  # runs of 4 equal values; h = 10 cuts runs 2 and 7
    out = [("all equal", np.full((2, 16), 3.25)),
           ("binary", (rng.random((2, 16)) < 0.4).astype(float)),
           ("binary 4 x 250", (rng.random((4, 250)) < 0.1).astype(float)),
           ("tie blocks across the split boundary", blocks),
           ("tie blocks, shuffled within chains", rng.permuted(blocks, axis=1)),
           ("odd n, S = 42, ties", rng.integers(0, 9, (3, 15)).astype(float)),
           ("odd n, S = 42, distinct", rng.standard_normal((3, 15))),
           ("S = 64, one chain", rng.standard_normal((1, 64))),
           ("S = 64, ties", rng.integers(0, 20, (2, 32)).astype(float)),
           ("2 x 8", rng.standard_normal((2, 8))),
           ("2 x 8 ties", rng.integers(0, 3, (2, 8)).astype(float))]
    out += [(f"small (4, 250) #{k}", R.small_set()[(4, 250)][:, :, k]) for k in range(3)]
    out += [(f"small (2, 101) #{k}", R.small_set()[(2, 101)][:, :, k]) for k in range(3)]
    return out


@pytest.mark.parametrize("folded", [0, 1])
def test_ranks_and_z_of_crafted_series(L, folded):
    for label, y in crafted_series():
        s = K.split_chains(y)
        if folded:
            s = np.abs(s - np.median(s))
        want_r = K.average_ranks(s)
        rk, z = gpu_zscale(L, y[:, :, None], folded)
        assert rk.shape == (1,) + s.shape
        assert np.array_equal(rk[0], want_r), f"{label} (folded {folded}): ranks"
        assert np.array_equal(rk[0] * 2, np.round(rk[0] * 2))
        err = z_rel_error(z[0], want_r, s.size)
        print(f"{label} (folded {folded}): z max relative error {err:.2e}")
        assert err <= EPS_Z, label
    # several series in one call, one of them not finite: NaN in its rows alone
    arr = R.small_set()[(3, 16)][:, :, :5].copy()
    arr[2, 9, 3] = np.nan
    rk, z = gpu_zscale(L, arr, folded)
    assert np.isnan(rk[3]).all() and np.isnan(z[3]).all()
    for k in (0, 1, 2, 4):
        s = K.split_chains(arr[:, :, k])
        if folded:
            s = np.abs(s - np.median(s))
        assert np.array_equal(rk[k], K.average_ranks(s))


def test_zscale_error_over_every_attainable_rank(L):
    """Largest relative error of z against ndtri over every rank a pool of S values can give — 1, 1.5,
    2, ..., S — for S in {16, 42, 64, 4000, 8192} (8192 on the global-memory path): three series per S,
    all values distinct, tied in pairs, tied in pairs after the first.  Measured on an MI355X with
    AS241 (PPND16): 8.9e-16 at most (see EPS_Z_MEASURED); EPS_Z is four times that and must stay below
    1e-12."""
    from mcmc_clv_model_amd import _lib
    rng = np.random.default_rng(29)
    worst = 0.0
    for S, (m, n) in ((16, (2, 8)), (42, (3, 15)), (64, (1, 64)), (4000, (4, 1000)), (8192, (2, 4096))):
        assert 2 * m * (n // 2) == S and (m * n > _lib.RANK_LDS_ELEMS) == (S == 8192)
        perm = rng.permutation(S).astype(float)
        pools = [perm, np.floor(perm / 2), np.floor((perm + 1) / 2)]
        arr = np.stack([unsplit(p.reshape(2 * m, n // 2), n, middle=-3.0) for p in pools], axis=2)
        rk, z = gpu_zscale(L, arr, 0)
        seen = set()
        for k, p in enumerate(pools):
            want_r = K.average_ranks(p.reshape(2 * m, n // 2))
            assert np.array_equal(rk[k], want_r)
            seen.update(want_r.ravel().tolist())
            worst_k = z_rel_error(z[k], want_r, S)
            worst = max(worst, worst_k)
        assert seen == set((np.arange(2, 2 * S + 1) / 2).tolist())  # every attainable rank
        print(f"S = {S}: z max relative error so far {worst:.3e}")
    print(f"measured max relative error of z: {worst:.3e} (EPS_Z = {EPS_Z:.3e})")
    assert worst <= EPS_Z <= 1e-12


@functools.lru_cache(maxsize=None)
def input_set(name):
    """(array (m, n, n_series), period, log mask) of a diagnostics_rank_ref.reference name."""
    kind = name.split(":")
    if kind[0] in ("small", "min"):
        return (R.small_set() if kind[0] == "small" else R.min_set())[(int(kind[1]), int(kind[2]))], 1, 0
    if name == "long":
        return R.long_set(), 1, 0
    if kind[0] == "threshold":
        return K.threshold_set(int(kind[1])), 1, 0
    a, w, mask, _, _ = R.golden_level1(kind[1])
    return a.reshape(a.shape[0], a.shape[1], -1), w, mask


def parity(L, name):
    arr, period, mask = input_set(name)
    want, mg = K.reference(name)
    assert (mg >= 1e-6).all()
    got = gpu_rank(L, arr, period, mask)
    assert_rank_parity(got, want, arr.shape[1] // 2, name)
    return got, want


@pytest.mark.parametrize("shape", R.SMALL_SHAPES)
def test_parity_small_set(L, shape):
    parity(L, f"small:{shape[0]}:{shape[1]}")


@pytest.mark.parametrize("shape", R.MIN_SHAPES)
def test_parity_minimum_length_set(L, shape):
    got, want = parity(L, f"min:{shape[0]}:{shape[1]}")
    if shape[1] < 10:
        assert (want[:, K.LAG_BULK] == -1).all()  # h = 4: no pair is ever evaluated


def test_parity_long_set_global_memory_path(L):
    from mcmc_clv_model_amd import _lib
    arr = R.long_set()
    assert arr.shape[0] * arr.shape[1] > _lib.RANK_LDS_ELEMS
    parity(L, "long")


@pytest.mark.parametrize("extra", [0, 1])
def test_parity_on_both_sides_of_the_lds_threshold(L, extra):
    """2 x RANK_LDS_ELEMS / 2 draws fill the LDS budget exactly; one more draw per chain takes the
    global-memory scratch."""
    from mcmc_clv_model_amd import _lib
    n = _lib.RANK_LDS_ELEMS // 2 + extra
    assert (2 * n > _lib.RANK_LDS_ELEMS) == bool(extra)
    parity(L, f"threshold:{n}")


@pytest.mark.parametrize("kind", ["bi", "tri"])
def test_parity_real_draws(L, kind):
    """Real level-1 draws with lambda and mu logged, through clv_rank_diagnostics and
    level1_rank_diagnostics.  The NaN counts are the yardstick's: the customers whose z never changes
    (12 bi, 21 tri) in every rank statistic; 3 more tri customers whose z is one half of the time
    (folded and squared series constant); and wherever an indicator is constant (ess_q95 of every
    binary z)."""
    from mcmc_clv_model_amd.analysis import level1_rank_diagnostics
    a, w, mask, _, _ = R.golden_level1(kind)
    n = a.shape[2]
    arr = a.reshape(a.shape[0], a.shape[1], n * w)
    want, mg = K.rank_stats_many(device_logged(L, arr, w, mask))
    assert (mg >= 1e-6).all()
    got = gpu_rank(L, arr, w, mask)
    assert_rank_parity(got, want, a.shape[1] // 2, f"golden {kind}")
    counts = {s: int(c) for s, c in zip(K.STATS, np.isnan(want).sum(axis=0)) if c}
    assert counts == {"bi": dict(rhat=12, rhat_bulk=12, rhat_folded=12, ess_bulk=12, ess_tail=393, ess_q05=26,
                                 ess_q95=393, ess_sd=12, mcse_sd=12, lag_bulk=12),
                      "tri": dict(rhat=24, rhat_bulk=21, rhat_folded=24, ess_bulk=21, ess_tail=396, ess_q05=30,
                                  ess_q95=396, ess_sd=24, mcse_sd=24, lag_bulk=21)}[kind]
    df = level1_rank_diagnostics({"level_1": list(a)})
    params = ["log_lambda", "log_mu", "tau", "z"] + (["eta"] if w == 5 else [])
    assert list(df.columns) == [f"{s}_{p}" for p in params for s in K.STATS] and len(df) == n
    assert np.array_equal(bits(df.to_numpy().reshape(n * w, len(K.STATS))), bits(got))
    plain = level1_rank_diagnostics({"level_1": list(a)}, log_columns=())
    assert "rhat_lambda" in plain and "rhat_log_lambda" not in plain
    # ranks do not change under the log: the bulk R-hat and ESS keep their bits
    for st in ("rhat_bulk", "ess_bulk", "lag_bulk"):
        assert np.array_equal(bits(plain[f"{st}_lambda"]), bits(df[f"{st}_log_lambda"])), st
    assert np.array_equal(bits(plain["ess_tail_tau"]), bits(df["ess_tail_tau"]))


def test_hdi_probabilities(L):
    arr = R.small_set()[(2, 101)][:, :, :8]
    for p in (0.5, 0.94, 0.95, 0.999, 0.001):
        got = gpu_rank(L, arr, hdi_prob=p)
        for k in range(8):
            lo, hi = K.hdi(arr[:, :, k], p)
            assert bits(got[k, K.HDI_LO]) == bits(lo) and bits(got[k, K.HDI_HI]) == bits(hi), (p, k)
    y = np.arange(100.0).reshape(2, 50)[:, :, None]
    assert gpu_rank(L, y)[0, [K.HDI_LO, K.HDI_HI, K.MEDIAN]].tolist() == [0.0, 94.0, 49.5]  # the first of equal widths


def test_non_finite_series_is_nan_and_neighbours_untouched(L):
    arr = R.small_set()[(2, 101)][:, :, :70].copy()
    clean = gpu_rank(L, arr)
    arr[1, 57, 33] = np.inf
    got = gpu_rank(L, arr)
    assert np.isnan(got[33]).all()
    keep = np.arange(70) != 33
    assert np.array_equal(bits(got[keep]), bits(clean[keep])) and np.isfinite(clean).all()
    # a logged series with a non-positive value, period 3: series 1, 4, 7, ... are logged
    pos = np.exp(R.small_set()[(3, 16)][:, :, :9])
    pos[0, 2, 4] = -1.0
    got = gpu_rank(L, pos, period=3, log_mask=0b010)
    assert np.isnan(got[4]).all() and np.isfinite(got[np.arange(9) != 4]).all()
    want, mg = K.rank_stats_many(device_logged(L, pos, 3, 0b010))
    assert (mg >= 1e-6).all() and np.isnan(want[4]).all()
    assert_rank_parity(got, want, 8, "logged, period 3")


@pytest.mark.parametrize("D", [2, 3])
def test_sampler_route_equals_host_route_bitwise(L, D):
    """HipSampler.diagnostics(rank=True) on the draws in HBM == the host-array functions on the draws
    read back, bit for bit (n = 300 is no multiple of the 256-customer block)."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    p = build_problem(cdnow("abe", n=300), [], D=D)
    w = D + 2
    dp = ctypes.POINTER(ctypes.c_double)
    with HipSampler(p, mcmc=40, burnin=20, thin=1, chains=2, seed=5) as s:
        out = np.empty((300 * w, len(K.STATS)))
        assert L.clv_rank_diagnostics_sampler(s.h, 3, 0.94, out.ctypes.data_as(dp), None) == -3  # CLV_ESTATE
        assert L.clv_rank_diagnostics_sampler(s.h, 3, 0.94, None, out.ctypes.data_as(dp)) == -3
        s.run(60)
        plain = s.diagnostics()
        dev = s.diagnostics(rank=True)
        l1, l2, _ = s.read_draws()
    assert set(plain) == {"level_1", "level_2"}
    assert set(dev) == {"level_1", "level_2", "level_1_rank", "level_2_rank", "level_2_summary"}
    for k in plain:
        assert np.array_equal(bits(dev[k].to_numpy()), bits(plain[k].to_numpy()))
    draws = dict(level_1=list(l1), level_2=list(l2))
    host1, host2, hosts = A.level1_rank_diagnostics(draws), A.level2_rank_diagnostics(draws), A.level2_summary(draws)
    assert list(dev["level_1_rank"].columns) == list(host1.columns)
    assert dev["level_1_rank"].shape == (300, len(K.STATS) * w)
    assert np.array_equal(bits(dev["level_1_rank"].to_numpy()), bits(host1.to_numpy()))
    assert np.array_equal(bits(dev["level_2_rank"].to_numpy()), bits(host2.to_numpy()))
    assert list(dev["level_2_summary"].columns) == list(hosts.columns) and "hdi_3%" in hosts and "r_hat" in hosts
    assert np.array_equal(bits(dev["level_2_summary"].to_numpy()), bits(hosts.to_numpy()))
    assert dev["level_2_rank"].shape == (D + D * (D + 1) // 2, len(K.STATS))
    assert np.isfinite(dev["level_2_rank"].to_numpy()).all()
    # against the yardstick too (lambda, mu logged); series with a decision margin under 1e-6 in any
    # of the four ESS evaluations have no exactly comparable lag: left out
    want, mg = K.rank_stats_many(device_logged(L, l1.reshape(2, 40, 300 * w), w, 3))
    sure = (mg >= 1e-6).all(axis=1)
    print(f"D={D}: {int(sure.sum())} of {len(sure)} series compared")
    assert sure.mean() > 0.99
    assert_rank_parity(host1.to_numpy().reshape(300 * w, len(K.STATS))[sure], want[sure], 20, f"sampler draws D={D}")
    with HipSampler(p, mcmc=40, burnin=20, thin=1, chains=2, seed=5, draw_sink="summary") as s:
        s.run(60)
        assert L.clv_rank_diagnostics_sampler(s.h, 3, 0.94, out.ctypes.data_as(dp), None) == -3  # no level-1 draws
        with pytest.raises(_lib.ClvError):
            s.diagnostics(rank=True)
        only2 = s.diagnostics(level1=False, rank=True)
        l2s = s.read_draws(level1=False)[1]
    assert set(only2) == {"level_2", "level_2_rank", "level_2_summary"}
    d2 = dict(level_2=list(l2s))
    assert np.array_equal(bits(only2["level_2_rank"].to_numpy()), bits(A.level2_rank_diagnostics(d2).to_numpy()))
    assert np.array_equal(bits(only2["level_2_summary"].to_numpy()), bits(A.level2_summary(d2).to_numpy()))


def test_drop_in_keyword(L):
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd._lib import check, dptr
    df = cdnow("abe", n=300)
    kw = dict(mcmc=40, burnin=20, thin=1, chains=2, seed=5, trace=0)
    for fn in (mcmc_draw_parameters, mcmc_draw_parameters_rfm_m):
        a = fn(df, **kw)
        b = fn(df, diagnostics="rank", **kw)
        assert "diagnostics" not in a and set(b) == set(a) | {"diagnostics"}
        assert np.array_equal(bits(np.stack(a["level_1"])), bits(np.stack(b["level_1"])))
        assert np.array_equal(bits(np.stack(a["level_2"])), bits(np.stack(b["level_2"])))
        assert np.array_equal(bits(a["log_likelihood"]), bits(b["log_likelihood"]))
        d = b["diagnostics"]
        assert set(d) == {"level_1", "level_2", "level_1_rank", "level_2_rank", "level_2_summary"}
        assert np.array_equal(bits(d["level_1"].to_numpy()), bits(A.level1_diagnostics(a).to_numpy()))
        assert np.array_equal(bits(d["level_2"].to_numpy()), bits(A.level2_diagnostics(a).to_numpy()))
        assert np.array_equal(bits(d["level_1_rank"].to_numpy()), bits(A.level1_rank_diagnostics(a).to_numpy()))
        assert np.array_equal(bits(d["level_2_rank"].to_numpy()), bits(A.level2_rank_diagnostics(a).to_numpy()))
        assert len(d["level_1_rank"]) == 300
        # level2_summary == the nine columns assembled by hand from the two C calls
        l2 = np.ascontiguousarray(np.stack(a["level_2"]))
        P = l2.shape[2]
        six, rk = np.empty((P, 6)), np.empty((P, len(K.STATS)))
        check(L.clv_diagnostics(-1, dptr(l2), 2, 40, P, 1, 0, dptr(six)))
        check(L.clv_rank_diagnostics(-1, dptr(l2), 2, 40, P, 1, 0, 0.94, dptr(rk)))
        hand = np.stack([six[:, 0], six[:, 1], rk[:, K.HDI_LO], rk[:, K.HDI_HI], six[:, 2], rk[:, K.MCSE_SD],
                         rk[:, K.ESS_BULK], rk[:, K.ESS_TAIL], rk[:, K.RHAT]], axis=1)
        sm = A.level2_summary(a)
        assert list(sm.columns) == ["mean", "sd", "hdi_3%", "hdi_97%", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat"]
        assert np.array_equal(bits(sm.to_numpy()), bits(hand)) and np.isfinite(hand).all()
        assert np.array_equal(bits(d["level_2_summary"].to_numpy()), bits(hand))
        assert list(A.level2_summary(a, hdi_prob=0.95).columns[2:4]) == ["hdi_2.5%", "hdi_97.5%"]
        with pytest.raises(ValueError, match="draw_sink='full'"):
            fn(df, diagnostics="rank", draw_sink="summary", **kw)
        with pytest.raises(ValueError, match="diagnostics must be"):
            fn(df, diagnostics="ranks", **kw)

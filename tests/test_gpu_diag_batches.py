"""The diagnostics of csrc/diag.hip under batching: for_series_batches walks the series in batches of
batch_series, which a test can only lower with the environment variable CLV_DIAG_BATCH (the natural
threshold is 2^27 values, 1 GiB of input).  With more than one batch the s0 offsets of
diag_gather_kernel (read index and (s0 + c) % period of the log mask), the out + (s0 + sidx) offsets
of diag_kernel / rank_kernel / zscale_kernel / acf_kernel, the global-path scratch sized from
batch_series and a short last batch that is no multiple of the 32-wide tile are all in play.

The file header of diag.hip promises sums in an order fixed by (m, n) alone, so a batched call equals
the unbatched call bit for bit; the unbatched call is held to the existing yardsticks
(tests/diagnostics_ref.py, tests/diagnostics_rank_ref.py) at the existing tolerances
(tests/test_gpu_diagnostics.py, tests/test_gpu_rank_diagnostics.py).  No tolerance is new.

Fixed input: m = 2 chains x n = 40 draws x 70 series of AR(1) values (exp of them where logged),
period 4, log mask 0b0101 (series 0 and 2 of every four are logged).  CLV_DIAG_BATCH in {1, 5, 32,
33, 69}: a batch that is no multiple of the period, exactly one tile, a tile plus one, a last batch of
one series.

Measured on MI355X: see DESIGN.md §Diagnostics ("Batches")."""
import functools
import os

import numpy as np
import pytest

from tests import diagnostics_rank_ref as K
from tests import diagnostics_ref as R
from tests.helpers import bits, cdnow
from tests.test_gpu_diagnostics import assert_parity, gpu_stats
from tests.test_gpu_rank_diagnostics import (EPS_Z, assert_rank_parity, device_logged, gpu_rank, gpu_zscale,
                                             z_rel_error)

pytestmark = pytest.mark.gpu

M, N, NS, PERIOD, MASK, MAX_LAG = 2, 40, 70, 4, 0b0101, 7
BATCHES = (1, 5, 32, 33, 69)
assert 5 % PERIOD != 0 and NS % 5 == 0 and NS % 32 == 6 and NS % 33 == 4 and NS % 69 == 1  # what the batches claim
SEED = 43
NAN_SERIES = 37


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    assert _lib.DIAG_BATCH_ENV not in os.environ, "the unbatched calls need CLV_DIAG_BATCH unset"
    return lib


@functools.lru_cache(maxsize=None)
def fixed_input():
    """(2, 40, 70): series k is AR(1) at phi = (k % 8) / 8 * 0.95, exponentiated where the mask logs it."""
    rng = np.random.default_rng(SEED)
    a = np.stack([R.ar1(rng, M, N, (k % 8) / 8 * 0.95) for k in range(NS)], axis=2)
    logged = ((MASK >> (np.arange(NS) % PERIOD)) & 1).astype(bool)
    assert logged.sum() == NS // 2 and bin(MASK).count("1") == 2
    a[:, :, logged] = np.exp(a[:, :, logged])
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def gpu_acf(L, arr, max_lag):
    """One clv_autocorr call on arr (m, n, n_series): (m, n_series, max_lag + 1)."""
    from mcmc_clv_model_amd._lib import check, dptr
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    m, n, ns = arr.shape
    out = np.full((m, ns, max_lag + 1), -7.0)
    check(L.clv_autocorr(-1, dptr(arr), m, n, ns, max_lag, dptr(out)))
    return out


def run_all(L, arr, period=1, mask=0):
    """Every entry point of the batch loop on one array: name -> output."""
    z0, z1 = gpu_zscale(L, arr, 0), gpu_zscale(L, arr, 1)
    return dict(diag=gpu_stats(L, arr, period, mask), rank=gpu_rank(L, arr, period, mask),
                acf=gpu_acf(L, arr, MAX_LAG), ranks=z0[0], z=z0[1], ranks_folded=z1[0], z_folded=z1[1])


def assert_same_bits(got, want, label):
    """Every output of run_all bit for bit (NaN payloads included)."""
    assert set(got) == set(want)
    diff = {k: int((bits(got[k]) != bits(want[k])).sum()) for k in want}
    print(f"{label}: entries whose bits differ from the unbatched call", diff)
    assert not any(diff.values()), (label, diff)


def assert_yardstick(L, out, arr, period, mask, label):
    """The unbatched outputs of run_all against the numpy / scipy yardsticks, at their tolerances."""
    m, n, ns = arr.shape
    want, mg = R.stats_many(arr, log_mask=mask, period=period)
    assert mg.min() >= 1e-6, f"{label}: the yardstick's own lag margin {mg.min():.2e}"
    logged = ((mask >> (np.arange(ns) % period)) & 1).astype(bool)
    ymax = max(np.abs(np.log(arr[:, :, logged])).max() if logged.any() else 0.0, np.abs(arr[:, :, ~logged]).max())
    assert_parity(out["diag"], want, ymax, f"{label} diag")
    want_r, mg_r = K.rank_stats_many(device_logged(L, arr, period, mask))
    assert (mg_r >= 1e-6).all(), f"{label}: the rank yardstick's own lag margin {mg_r.min():.2e}"
    assert_rank_parity(out["rank"], want_r, n // 2, f"{label} rank")
    want_a = np.stack([R.autocorr(arr[:, :, s], MAX_LAG) for s in range(ns)], axis=1)
    print(f"{label} acf: max abs deviation {np.max(np.abs(out['acf'] - want_a)):.2e}")
    np.testing.assert_allclose(out["acf"], want_a, rtol=0, atol=1e-12)
    assert (out["acf"][..., 0] == 1.0).all()
    worst = 0.0
    for folded, rk, z in ((0, out["ranks"], out["z"]), (1, out["ranks_folded"], out["z_folded"])):
        for s in range(ns):
            sp = K.split_chains(arr[:, :, s])
            if folded:
                sp = np.abs(sp - np.median(sp))
            rr = K.average_ranks(sp)
            assert np.array_equal(rk[s], rr), f"{label}: ranks of series {s} (folded {folded})"
            worst = max(worst, z_rel_error(z[s], rr, sp.size))
    print(f"{label} zscale: ranks exact, z max relative error {worst:.2e}")
    assert worst <= EPS_Z


@pytest.fixture(scope="module")
def base(L):
    """The unbatched outputs on the fixed input, computed once and shared (read-only)."""
    out = run_all(L, fixed_input(), PERIOD, MASK)
    for v in out.values():
        v.setflags(write=False)
    return out


def test_unbatched_meets_the_yardsticks(L, base):
    assert_yardstick(L, base, fixed_input(), PERIOD, MASK, "2 x 40 x 70 unbatched")


@pytest.mark.parametrize("batch", BATCHES)
def test_batched_equals_unbatched_bitwise(L, base, monkeypatch, batch):
    from mcmc_clv_model_amd import _lib
    monkeypatch.setenv(_lib.DIAG_BATCH_ENV, str(batch))
    got = run_all(L, fixed_input(), PERIOD, MASK)
    monkeypatch.delenv(_lib.DIAG_BATCH_ENV)
    assert_same_bits(got, base, f"CLV_DIAG_BATCH={batch}")


def test_nan_stays_in_its_series_across_a_batch_boundary(L, base, monkeypatch):
    """A NaN in series 37 (batch 7 of batches of 5, third of its batch): its rows are NaN, every other
    row keeps the bits of the clean, unbatched call.  clv_autocorr is per chain: the NaN is in chain 1."""
    from mcmc_clv_model_amd import _lib
    arr = fixed_input().copy()
    arr[1, 17, NAN_SERIES] = np.nan
    monkeypatch.setenv(_lib.DIAG_BATCH_ENV, "5")
    got = run_all(L, arr, PERIOD, MASK)
    monkeypatch.delenv(_lib.DIAG_BATCH_ENV)
    keep = np.arange(NS) != NAN_SERIES
    for k in ("diag", "rank", "ranks", "z", "ranks_folded", "z_folded"):
        assert np.isnan(got[k][NAN_SERIES]).all(), k
    assert np.isnan(got["acf"][1, NAN_SERIES]).all()
    assert np.array_equal(bits(got["acf"][0]), bits(base["acf"][0]))
    assert_same_bits({k: (v[:, keep] if k == "acf" else v[keep]) for k, v in got.items()},
                     {k: (v[:, keep] if k == "acf" else v[keep]) for k, v in base.items()}, "NaN in series 37, batches of 5")
    assert all(np.isfinite(v).all() for v in base.values())


def test_global_memory_paths_batched(L, monkeypatch):
    """One shape just past each kernel's LDS threshold (2 x 4097 for diag / acf, 2 x (RANK_LDS_ELEMS / 2
    + 1) for rank / zscale), 5 series in batches of 2: the only place where the rank scratch
    scratch + sidx * 2 * N is sized for fewer series than the call has."""
    from mcmc_clv_model_amd import _lib
    for n, names in ((4097, ("diag", "acf")), (_lib.RANK_LDS_ELEMS // 2 + 1, ("rank", "ranks", "z", "ranks_folded", "z_folded"))):
        rng = np.random.default_rng(17)
        arr = np.ascontiguousarray(np.stack([R.ar1(rng, 2, n, 0.9) for _ in range(5)], axis=2))
        assert 2 * n > (8192 if "diag" in names else _lib.RANK_LDS_ELEMS)
        whole = run_all(L, arr)
        monkeypatch.setenv(_lib.DIAG_BATCH_ENV, "2")
        got = run_all(L, arr)
        monkeypatch.delenv(_lib.DIAG_BATCH_ENV)
        assert_same_bits(got, whole, f"global path 2 x {n} x 5, batches of 2")
        if "diag" in names:
            want, mg = R.stats_many(arr)
            assert mg.min() >= 1e-6
            assert_parity(whole["diag"], want, np.abs(arr).max(), f"global path 2 x {n} diag")
            want_a = np.stack([R.autocorr(arr[:, :, s], MAX_LAG) for s in range(5)], axis=1)
            print(f"global path 2 x {n} acf: max abs deviation {np.max(np.abs(whole['acf'] - want_a)):.2e}")
            np.testing.assert_allclose(whole["acf"], want_a, rtol=0, atol=1e-12)
        else:
            want_r, mg_r = K.rank_stats_many(arr)
            assert (mg_r >= 1e-6).all()
            assert_rank_parity(whole["rank"], want_r, n // 2, f"global path 2 x {n} rank")
            for s in range(5):
                assert np.array_equal(whole["ranks"][s], K.average_ranks(K.split_chains(arr[:, :, s])))


def test_sampler_route_batched(L, monkeypatch):
    """clv_diagnostics_sampler / clv_rank_diagnostics_sampler on the draws in HBM (D = 2, n = 300: 1200
    series of width 4) in batches of 7 series, which cut through a customer's four columns."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem
    p = build_problem(cdnow("abe", n=300), [], D=2)
    with HipSampler(p, mcmc=40, burnin=20, thin=1, chains=2, seed=5) as s:
        s.run(60)
        whole = s.diagnostics(rank=True)
        monkeypatch.setenv(_lib.DIAG_BATCH_ENV, "7")
        got = s.diagnostics(rank=True)
        monkeypatch.delenv(_lib.DIAG_BATCH_ENV)
    assert set(whole) == {"level_1", "level_2", "level_1_rank", "level_2_rank", "level_2_summary"}
    assert whole["level_1"].shape == (300, 6 * 4) and np.isfinite(whole["level_2"].to_numpy()).all()
    assert_same_bits({k: v.to_numpy() for k, v in got.items()}, {k: v.to_numpy() for k, v in whole.items()},
                     "sampler route, batches of 7")

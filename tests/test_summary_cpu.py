"""The summary sink without a GPU: its float64 model (tests/summary_ref.py) against math.fsum and
against itself, the preconditions the GPU cases and their power checks rely on, the names and the
layout of the sums (include/clvmcmc.h, _lib, sampler._assemble), and analysis.summary_rhat on the
model's sums against the R-hat of the draws."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import pytest

from tests import summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_CASES = R.POWER_CASES   # one trivariate (K = 3) and one bivariate (K = 9) case, N = 257, 5 stored draws


@pytest.fixture(scope="module")
def draws():
    """{case: [(stored draws, log-scale states) per chain]} of the model's free runs, computed once."""
    out = {}
    for name in MODEL_CASES:
        c = R.CASES[name]
        out[name] = [R.model_draws(c, c["chain_first"] + k) for k in range(c["chains"])]
    return out


@pytest.mark.parametrize("name", MODEL_CASES)
def test_sequential_sums_agree_with_fsum(draws, name):
    """Every plane of sums_from_draws within n 2^-53 sum |terms| of the exactly rounded sum."""
    l1 = draws[name][0][0]
    n, N, w = l1.shape
    assert N == 257 and n == 5
    got = R.sums_from_draws(l1)
    lam, mu, tau, z = (l1[..., k] for k in range(4))
    terms = {"lambda": lam, "mu": mu, "z": z, "log_lambda": np.log(lam), "log_mu": np.log(mu), "lambda2": lam * lam,
             "mu2": mu * mu, "mu_capped": np.minimum(mu, 0.05), "tau": tau}
    if w == 5:
        terms.update(eta=l1[..., 4], log_eta=np.log(l1[..., 4]))
    for k, nm in enumerate(R.SUM_STATS):
        if nm not in terms:
            assert not got[k].any(), nm     # the bivariate eta planes: zeros, as on the device
            continue
        t = terms[nm]
        exact = np.array([math.fsum(t[:, i]) for i in range(N)])
        slack = n * R.U * np.abs(t).sum(axis=0)
        assert np.all(np.abs(got[k] - exact) <= slack), nm
        assert np.isfinite(got[k]).all() and got[k].any(), nm


@pytest.mark.parametrize("name", MODEL_CASES)
def test_inputs_meet_the_preconditions_of_the_gpu_cases(draws, name):
    """What makes the exact comparisons and every power mutation bite, on the model's run of the very
    cases the device is held to: mu on both sides of the cap — beyond it for more than half of the
    customers in some stored draw, so a cap of 0.5 changes their sum — z of both values, tau varying,
    and, bivariate, mu_capped and tau planes that differ from each other and from zero (a shift by two
    planes is visible)."""
    for l1, _ in draws[name]:
        mu, tau, z = l1[..., 1], l1[..., 2], l1[..., 3]
        assert (mu < R.MU_CAP).any() and (mu > R.MU_CAP).any()
        assert (mu > R.MU_CAP).any(axis=0).mean() > 0.5 and (mu < 0.5).all(axis=0).mean() > 0.5
        assert set(np.unique(z)) == {0.0, 1.0}
        assert (np.ptp(tau, axis=0) > 0).mean() > 0.5
        s = R.sums_from_draws(l1)
        cap, ta = s[R.SUM_STATS.index("mu_capped")], s[R.SUM_STATS.index("tau")]
        assert (cap != ta).all() and (cap != 0).all() and (ta != 0).all()
        assert (l1[..., 0] != 1.0).all()                  # lambda2 from lam
        assert (l1[..., 0] != l1[..., 1]).all()           # mu2 from lam * mu; the logs exchanged


@pytest.mark.parametrize("name", MODEL_CASES)
def test_every_wrong_model_fails_against_the_right_one(draws, name):
    """check_sums on the model's own sums passes everywhere; with one thing wrong in the model it fails
    for more than half of the customers (the GPU module does the same with the device's sums)."""
    l1 = draws[name][0][0]
    D = l1.shape[2] - 2
    good = R.sums_from_draws(l1)
    bad, ratio = R.check_sums(good, l1)
    assert not R.any_bad(bad).any() and all(not r.any() for r in ratio.values())
    for wrong in R.WRONG:
        if wrong == "d2_shifted_by_two" and D == 3:
            continue
        assert R.any_bad(R.check_sums(good, l1, wrong=wrong)[0]).mean() > 0.5, wrong
    assert R.any_bad(R.check_sums(good, l1, mu_cap=0.5)[0]).mean() > 0.5


@pytest.mark.parametrize("name", MODEL_CASES)
def test_log_bound_covers_exp_then_log_of_the_models_states(draws, name):
    """The device's side of the log sums is the sum of the states, the model's the sum of np.log of
    the draw: the model's states through np.exp (within 1 ulp, inside exp_fast's 2.5) and np.log stay
    inside log_sum_bound — over all stored draws, over every prefix, and for a single draw."""
    for l1, states in draws[name]:
        for nm, st in states.items():
            col = R.LOG_COLUMN[nm]
            d = np.exp(st)
            assert np.array_equal(d, l1[..., col]) or np.allclose(d, l1[..., col], rtol=1e-15)
            for k in range(1, st.shape[0] + 1):
                dev = R.seq_sum(st[:k])
                mod = R.seq_sum(np.log(d[:k]))
                bound = R.log_sum_bound(d[:k])
                assert np.all(np.abs(dev - mod) <= bound), (nm, k, (np.abs(dev - mod) / bound).max())
            one = R.log_sum_bound(d[:1])
            assert np.allclose(one, (1 + 2.0 ** -20) * R.U * (5.0 + 2.0 * np.abs(np.log(d[0]))), rtol=1e-15)


def test_log_bound_is_not_slack_by_orders_of_magnitude():
    """A state moved by 64 ulp of the draw (2^-46 relative: 32 times exp_fast's figure) leaves the
    bound for every customer: the bound is a few units of 2^-53 per draw, not a loose tolerance."""
    rng = np.random.default_rng(5)
    st = rng.uniform(-6.0, -1.0, (5, 257))
    d = np.exp(st)
    dev = R.seq_sum(st + 2.0 ** -46)
    assert np.all(np.abs(dev - R.seq_sum(np.log(d))) > R.log_sum_bound(d))


# ---------------------------------------------------------------------------------------------
def test_names_and_layout_match_the_header():
    from mcmc_clv_model_amd import _lib
    with open(os.path.join(ROOT, "include", "clvmcmc.h")) as f:
        text = f.read()
    m = re.search(r"enum\s*\w*\s*\{\s*(CLV_SUM_LAMBDA\s*=\s*0.*?)CLV_N_SUM_STATS", text, re.S)
    assert m, "the CLV_SUM_* enum was not found in include/clvmcmc.h"
    names = [t.split("=")[0].strip() for t in m.group(1).split(",") if t.strip()]
    assert [n[len("CLV_SUM_"):].lower() for n in names] == list(_lib.SUM_STATS)
    assert len(names) == _lib.N_SUM_STATS == 11
    assert _lib.SUM_STATS == R.SUM_STATS
    assert set(R.EXACT_STATS) | set(R.LOG_STATS) == set(R.SUM_STATS) and len(R.EXACT_STATS) == 8
    cap = re.search(r"#define\s+CLV_SUMMARY_MU_CAP\s+([0-9.eE+-]+)", text)
    assert cap and float(cap.group(1)) == 0.05 == _lib.SUMMARY_MU_CAP == R.MU_CAP
    import inspect
    from mcmc_clv_model_amd.analysis import level1_summary
    from mcmc_clv_model_amd.sampler import HipSampler
    assert inspect.signature(level1_summary).parameters["mu_cap"].default == 0.05
    assert inspect.signature(HipSampler.level1_summary).parameters["mu_cap"].default == 0.05


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("sink", ["summary", "summary+pct"])
def test_assemble_gives_every_name_its_own_plane(D, sink):
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.sampler import _assemble
    C, N, k = 2, 3, 4
    consts = np.array([3.0, 5.0, 7.0, 11.0, 13.0, 17.0, 19.0, 23.0, 29.0, 31.0, 37.0])   # eleven distinct planes
    sums = np.empty((C, 11, N))
    for c in range(C):
        for i in range(N):
            sums[c, :, i] = consts * (1 + c) + i / 64.0
    l2, ll = np.zeros((C, k, D + D * (D + 1) // 2)), np.zeros((C, k))

    def no_level1():
        raise AssertionError("level-1 statistics are not asked for before every draw is stored")

    out = _assemble(D, C, None, l2, ll, sums, k, k + 1, sink, no_level1)
    sm = out["summary"]
    want = [nm for nm in _lib.SUM_STATS if D == 3 or nm not in ("eta", "log_eta")]
    assert sorted(sm) == sorted(want + ["n_draws"]) and sm["n_draws"] == k
    if D == 2:
        assert "eta" not in sm and "log_eta" not in sm
    for nm in want:
        assert np.array_equal(sm[nm], sums[:, _lib.SUM_STATS.index(nm), :] / k), nm
        assert sm[nm].shape == (C, N)
    zero = _assemble(D, C, None, l2[:, :0], ll[:, :0], np.zeros_like(sums), 0, k, sink, no_level1)["summary"]
    assert zero["n_draws"] == 0
    for nm in want:
        assert np.array_equal(zero[nm], np.zeros((C, N))), nm   # k = 0: no division by zero
    assert _assemble(D, C, None, l2, ll, None, 0, k, "full", None).get("summary") is None


# ---------------------------------------------------------------------------------------------
def _summary_dict(chains):
    n = chains[0].shape[0]
    sums = np.stack([R.sums_from_draws(l1) for l1 in chains]) / n
    return dict(summary=dict(n_draws=n, **{nm: sums[:, k] for k, nm in enumerate(R.SUM_STATS)}))


def test_summary_rhat_agrees_with_the_rhat_of_the_draws(draws):
    from mcmc_clv_model_amd.analysis import summary_rhat
    chains = [l1 for l1, _ in draws[R.CONSUMER_CASE]]
    assert len(chains) >= 3
    got = summary_rhat(_summary_dict(chains))
    ref, tol = R.rhat_from_draws(chains), R.rhat_tolerance(chains)
    for nm in R.RHAT_COLUMNS:
        assert np.isfinite(tol[nm]).all() and np.isfinite(ref[nm]).all(), nm
        err = np.abs(got[nm].to_numpy() - ref[nm])
        print(f"{nm}: largest error / tolerance {np.max(err / tol[nm]):.3f}, largest tolerance {tol[nm].max():.2e}")
        assert np.all(err <= tol[nm]), nm
        assert tol[nm].max() < 1e-9 and (ref[nm] > 0.5).all()   # the tolerance is rounding, not slack
        wrong = got[nm].to_numpy() * (1.0 + 1e-6)
        assert np.all(np.abs(wrong - ref[nm]) > tol[nm])


def test_summary_rhat_is_nan_for_a_constant_series(draws):
    from mcmc_clv_model_amd.analysis import summary_rhat
    chains = [l1.copy() for l1, _ in draws[R.CONSUMER_CASE]]
    for c, l1 in enumerate(chains):
        l1[:, 7, 0] = 0.25 * (1 + c)      # customer 7's lambda constant within each chain
        l1[:, 9, 1] = 0.03125             # customer 9's mu the same constant in every chain
    got = summary_rhat(_summary_dict(chains))
    assert np.isnan(got["rhat_lambda"][7]) and np.isnan(got["rhat_mu"][9])
    keep = np.ones(len(got), bool)
    keep[[7, 9]] = False
    assert np.isfinite(got["rhat_lambda"][keep]).all() and np.isfinite(got["rhat_mu"][keep]).all()
    assert np.isinf(R.rhat_tolerance(chains)["rhat_lambda"][7])

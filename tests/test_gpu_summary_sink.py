"""The summary sinks' running sums (cust_store in csrc/kernels.hip, shared by every sweep kernel)
against the float64 model of the sink (tests/summary_ref.py) on the stored draws of the same problem
and seed run with the full sink — on every sweep path: one launch per sweep (prefetch_sums / SumsPre
and its D = 2 slot remap), the persistent kernel's block, split and relay layouts, and batch_fit_kernel.

Every case first shows that the two runs are one trajectory (level-2 records, log-likelihood and the
carried state equal to the bit); then the eight exact sums are compared by their bits — no tolerance,
no lane set aside — and the three log sums within summary_ref.log_sum_bound, whose measured / bound
ratio is printed.  The kernel is asserted through launch_info() before each run."""
import numpy as np
import pytest

from tests import summary_ref as R
from tests.helpers import bits, cdnow, with_covariates

pytestmark = pytest.mark.gpu

IDX = {nm: k for k, nm in enumerate(R.SUM_STATS)}


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


_problems, _pairs = {}, {}


def _problem(case):
    from mcmc_clv_model_amd.sampler import build_problem
    key = (case["D"], case["K"], case["n"])
    if key not in _problems:
        _problems[key] = build_problem(R.case_frame(case), case["covs"], case["D"])
    return _problems[key]


def _open(monkeypatch, case, sink, **over):
    """A handle of ``case`` under its kernel (the environment is read at create), the kernel asserted."""
    from mcmc_clv_model_amd.sampler import HipSampler
    mode = case["mode"]
    for v in ("CLV_PERSISTENT", "CLV_PERSIST_LAYOUT", "CLV_SPLIT_RELAY"):
        monkeypatch.delenv(v, raising=False)
    if mode == "fused":
        monkeypatch.setenv("CLV_PERSISTENT", "0")
    else:
        monkeypatch.setenv("CLV_PERSISTENT", "1")
        monkeypatch.setenv("CLV_PERSIST_LAYOUT", "block" if mode == "block" else "split")
        if mode != "block":
            monkeypatch.setenv("CLV_SPLIT_RELAY", "1" if mode == "relay" else "0")
    kw = dict(mcmc=case["mcmc"], burnin=case["burnin"], thin=case["thin"], chains=case["chains"],
              chain_first=case["chain_first"], seed=case["seed"], n_mh_steps=case["S"], draw_sink=sink)
    kw.update(over)
    s = HipSampler(_problem(case), **kw)
    info = s.launch_info()
    assert info["persistent"] == (mode != "fused"), info
    assert info["layout"] == {"fused": None, "block": "block", "split": "split", "relay": "split"}[mode], info
    assert (info["relay_steps"] > 0) == (mode == "relay"), info
    return s


def _trajectory(s, full):
    l1, l2, ll = s.read_draws(level1=full)
    return dict(l1=l1, l2=l2, ll=ll, state=s.get_state())


def _same_trajectory(a, b, what):
    assert np.array_equal(bits(a["l2"]), bits(b["l2"])), (what, "level-2 records")
    assert np.array_equal(bits(a["ll"]), bits(b["ll"])), (what, "log-likelihood")
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(bits(x), bits(y)), (what, "carried state")
    assert a["l2"].any() and np.isfinite(a["l2"]).all(), what


def _assert_sums(sums, l1, what, upto=None):
    """Every chain's sums [C][11][N] against the model of l1 [C][n][N][D + 2] (its first ``upto`` draws);
    returns the largest measured / bound ratio of each log sum."""
    worst = {}
    for c in range(sums.shape[0]):
        bad, ratio = R.check_sums(sums[c], l1[c] if upto is None else l1[c][:upto])
        for nm in R.SUM_STATS:
            assert not bad[nm].any(), f"{what}, chain {c}: {nm} differs for {int(bad[nm].sum())} of {bad[nm].size} customers"
        for nm, r in ratio.items():
            if r.size and np.isfinite(r).any():
                worst[nm] = max(worst.get(nm, 0.0), float(np.nanmax(r)))
    return worst


def _pair(monkeypatch, name):
    """``name``'s problem and seed run with the full sink and with its summary sink, once per module."""
    if name in _pairs:
        return _pairs[name]
    case = R.CASES[name]
    sweeps = case["burnin"] + case["mcmc"]
    with _open(monkeypatch, case, "full") as s:
        s.run(sweeps)
        full = _trajectory(s, True)
    with _open(monkeypatch, case, case["sink"]) as s:
        s.run(sweeps)
        summ = _trajectory(s, False)
        summ["sums"], summ["k"] = s.read_summary()
        if case["sink"] == "summary+pct":
            from mcmc_clv_model_amd import _lib
            summ["level1"] = s.level1_summary(_lib.SUMMARY_MU_CAP)
    _same_trajectory(full, summ, name)
    _pairs[name] = (case, full, summ)
    return _pairs[name]


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["sink"] == "summary"])
def test_sums_equal_the_model_of_the_stored_draws(L, monkeypatch, name):
    case, full, summ = _pair(monkeypatch, name)
    n_draws = len(R.stored_sweeps(case["burnin"], case["mcmc"], case["thin"]))
    assert summ["k"] == n_draws == full["l1"].shape[1] and full["l1"].shape[2] == case["n"]
    assert summ["l1"] is None and summ["sums"].shape == (case["chains"], 11, case["n"])
    worst = _assert_sums(summ["sums"], full["l1"], name)
    print(f"{name}: log sums, largest measured / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert set(worst) == {"log_lambda", "log_mu"} | ({"log_eta"} if case["D"] == 3 else set())


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["sink"] == "summary+pct"])
def test_summary_pct_under_launch_per_sweep(L, monkeypatch, name):
    """"summary+pct" on the launch-per-sweep kernel: the sums as above; the percentiles bit-equal to
    numpy's 'linear' percentile of the float32-rounded draws pooled over chains; the pooled means the
    sums added in chain order, divided by chains x draws (sums_mean_kernel)."""
    from mcmc_clv_model_amd import _lib
    case, full, summ = _pair(monkeypatch, name)
    C, n_draws = case["chains"], full["l1"].shape[1]
    assert summ["k"] == n_draws
    worst = _assert_sums(summ["sums"], full["l1"], name)
    print(f"{name}: log sums, largest measured / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    pooled = np.concatenate(list(full["l1"]), axis=0)
    col = {nm: k for k, nm in enumerate(_lib.L1_STATS)}
    got = summ["level1"]
    for c, nm in ((0, "lambda"), (1, "mu")):
        x32 = pooled[:, :, c].astype(np.float32).astype(np.float64)
        for q, tag in ((2.5, "p025"), (97.5, "p975")):
            assert np.array_equal(bits(got[:, col[f"{nm}_{tag}"]]), bits(np.percentile(x32, q, axis=0))), (nm, tag)
    means = [("mean_lambda", "lambda"), ("mean_mu", "mu"), ("mean_mu_capped", "mu_capped"), ("mean_z", "z"),
             ("mean_tau", "tau")] + ([("mean_eta", "eta")] if case["D"] == 3 else [])
    for out_nm, nm in means:
        ref = R.seq_sum(np.stack([R.sums_from_draws(full["l1"][c])[IDX[nm]] for c in range(C)])) / float(C * n_draws)
        assert np.array_equal(bits(got[:, col[out_nm]]), bits(ref)), out_nm


# ---------------------------------------------------------------------------------------------
# call patterns
# ---------------------------------------------------------------------------------------------
CALLS = (3, 3, 2, 1, 1, 4, 1)   # stored sweeps 6, 9, 12, 15: a call ending on one, one that is only one, two
PATTERN = dict(burnin=5, thin=3, mcmc=11)   # without any, one across the burn-in boundary; 15 of 16 sweeps


@pytest.mark.parametrize("mode,D", [("fused", 2), ("block", 3)])
def test_partial_sums_after_every_call_and_rollback(L, monkeypatch, mode, D):
    """read_summary() after each call equals the sums over the draws stored so far (zero before the
    first; k = n_draws - 1 and three draws' sums after the sixth call, one sweep short of the last
    stored draw).  Persistent kernel: rollback() after a call that held a stored sweep returns sums and
    count to the previous call's bits and the call redone gives the straight run's; the launch-per-sweep
    path has nothing to roll back (include/clvmcmc.h: persistent path only) and says so, sums untouched."""
    case = dict(R.make_case(D, 2, 257, 2, 0, mode, 8200 + D), **PATTERN)
    assert R.stored_sweeps(5, 11, 3) == [6, 9, 12, 15]
    with _open(monkeypatch, case, "full") as s:
        s.run(sum(CALLS))
        full = _trajectory(s, True)
    assert full["l1"].shape[1] == 4 and full["l1"][:, 3].any()
    with _open(monkeypatch, case, "summary") as s:
        sums, k = s.read_summary()
        assert k == 0 and not sums.any()
        done, seen = 0, []
        for j, n in enumerate(CALLS):
            prev = (sums.copy(), k)
            s.run(n)
            done += n
            sums, k = s.read_summary()
            assert k == len(R.stored_sweeps(5, 11, 3, upto=done)), (j, k)
            _assert_sums(sums, full["l1"], f"{mode} after call {j}", upto=k)
            seen.append(k)
            if k > prev[1]:   # the call held a stored sweep
                if mode == "fused":
                    with pytest.raises(Exception, match="nothing to roll back"):
                        s.rollback()
                    again, k2 = s.read_summary()
                else:
                    s.rollback()
                    back, kb = s.read_summary()
                    assert kb == prev[1] and np.array_equal(bits(back), bits(prev[0])), f"rollback of call {j}"
                    s.run(n)
                    again, k2 = s.read_summary()
                assert k2 == k and np.array_equal(bits(again), bits(sums)), f"call {j} redone"
        assert seen == [0, 1, 1, 2, 2, 3, 4]
        _same_trajectory(full, _trajectory(s, False), mode)


@pytest.mark.parametrize("mode", ["fused", "block"])
def test_one_stored_draw(L, monkeypatch, mode):
    """mcmc = 1, burnin = 0: each exact plane is the draw itself (or its square, its capped value);
    each log plane within the single-draw bound of log(draw)."""
    case = R.make_case(3, 1, 257, 2, 0, mode, 8300, burnin=0, mcmc=1, thin=1)
    with _open(monkeypatch, case, "full") as s:
        s.run(1)
        full = _trajectory(s, True)
    with _open(monkeypatch, case, "summary") as s:
        s.run(1)
        summ = _trajectory(s, False)
        sums, k = s.read_summary()
    _same_trajectory(full, summ, mode)
    assert k == 1 and full["l1"].shape[1] == 1
    d = full["l1"][:, 0]   # [C][N][5]
    for nm, col in (("lambda", 0), ("mu", 1), ("tau", 2), ("z", 3), ("eta", 4)):
        assert np.array_equal(bits(sums[:, IDX[nm]]), bits(d[..., col])), nm
    assert np.array_equal(bits(sums[:, IDX["lambda2"]]), bits(d[..., 0] * d[..., 0]))
    assert np.array_equal(bits(sums[:, IDX["mu2"]]), bits(d[..., 1] * d[..., 1]))
    assert np.array_equal(bits(sums[:, IDX["mu_capped"]]), bits(np.minimum(d[..., 1], 0.05)))
    for nm, col in R.LOG_COLUMN.items():
        t = np.log(d[..., col])
        err = np.abs(sums[:, IDX[nm]] - t)
        bound = (1 + 2.0 ** -20) * R.U * (5.0 + 2.0 * np.abs(t))
        print(f"one draw, {mode}: {nm} largest measured / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), nm
    _assert_sums(sums, full["l1"], mode)


# ---------------------------------------------------------------------------------------------
# the batch kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_batch_kernel_summary_means(L, D):
    """batch_fit_kernel's summary sink: every name of out[j]["summary"] against sums_from_draws / k of
    the same call with the full sink, fits of 255, 256 and 257 customers (a block less one lane, a full
    block, a block plus one lane) starting at a row with x > 0.  The exact stats by their bits (one
    division by k on either side); the log means within log_sum_bound / k plus the two divisions'
    roundings, 2^-53 of either mean."""
    from mcmc_clv_model_amd import mcmc_draw_parameters_many, mcmc_draw_parameters_rfm_m_many
    many = mcmc_draw_parameters_many if D == 2 else mcmc_draw_parameters_rfm_m_many
    data = with_covariates(cdnow("full"), 1)
    assert data["x"].iloc[2] > 0
    ns = (255, 256, 257)
    fits = [data.iloc[2:2 + n].reset_index(drop=True) for n in ns]
    kw = dict(seeds=[8401, 8402, 8403], mcmc=10, burnin=3, thin=3, chains=2, n_mh_steps=20, return_info=True)
    full, info = many(fits, ["c1"], draw_sink="full", **kw)
    assert list(info["path"]) == ["batch"] * 3 and list(info["blocks"]) == [1, 1, 2]
    summ, info = many(fits, ["c1"], draw_sink="summary", **kw)
    assert list(info["path"]) == ["batch"] * 3
    names = [nm for nm in R.SUM_STATS if D == 3 or nm not in ("eta", "log_eta")]
    for j, n in enumerate(ns):
        f, sm = full[j], summ[j]
        assert sm["level_1"] is None and len(f["level_1"]) == 2 and f["level_1"][0].shape == (4, n, D + 2)
        for c in range(2):
            assert np.array_equal(bits(sm["level_2"][c]), bits(f["level_2"][c])), (n, c)
        assert np.array_equal(bits(np.float64(sm["log_likelihood"])), bits(np.float64(f["log_likelihood"])))
        assert sorted(sm["summary"]) == sorted(names + ["n_draws"]) and sm["summary"]["n_draws"] == 4
        for c in range(2):
            l1 = f["level_1"][c]
            ref = R.sums_from_draws(l1) / 4.0
            for nm in names:
                got = sm["summary"][nm][c]
                if nm in R.LOG_STATS:
                    bound = R.log_sum_bound(l1[..., R.LOG_COLUMN[nm]]) / 4.0 + R.U * (np.abs(got) + np.abs(ref[IDX[nm]]))
                    err = np.abs(got - ref[IDX[nm]])
                    print(f"batch D = {D}, N = {n}, chain {c}: {nm} largest measured / bound {np.max(err / bound):.3f}")
                    assert np.all(err <= bound), (n, c, nm)
                else:
                    assert np.array_equal(bits(got), bits(ref[IDX[nm]])), (n, c, nm, int((got != ref[IDX[nm]]).sum()))


# ---------------------------------------------------------------------------------------------
# consumers of the sums
# ---------------------------------------------------------------------------------------------
def test_summary_rhat_and_envelope_means_on_device_sums(L, monkeypatch):
    """What reads the sums downstream, on the three-chain bivariate case: analysis.summary_rhat of the
    assembled result against the R-hat of the full run's draws within the derived tolerance, and the
    four summary means test_gpu_statistics._run_envelope takes (log_lambda, log_mu, z, lambda) against
    their draws-based counterparts of the same function: the sink's own bound (exact / log_sum_bound)
    over n, plus what a mean of n terms taken in another order may differ by, 2 n 2^-53 mean |terms|."""
    from mcmc_clv_model_amd.analysis import summary_rhat
    from mcmc_clv_model_amd.sampler import _assemble
    case, full, summ = _pair(monkeypatch, R.CONSUMER_CASE)
    C, n = case["chains"], summ["k"]
    assert C >= 3 and case["D"] == 2
    res = _assemble(case["D"], C, None, summ["l2"], summ["ll"], summ["sums"], n, n, "summary", None)
    sm = res["summary"]
    assert sm["n_draws"] == n and "eta" not in sm
    chains = list(full["l1"])
    got, ref, tol = summary_rhat(res), R.rhat_from_draws(chains), R.rhat_tolerance(chains)
    for nm in R.RHAT_COLUMNS:
        assert np.isfinite(tol[nm]).all() and np.isfinite(ref[nm]).all() and tol[nm].max() < 1e-9, nm
        err = np.abs(got[nm].to_numpy() - ref[nm])
        print(f"{nm}: largest error / tolerance {np.max(err / tol[nm]):.3f}")
        assert np.all(err <= tol[nm]), nm
    l1 = full["l1"]
    order = lambda t: 2.0 * n * R.U * np.abs(t).mean(axis=1)  # noqa: E731
    assert np.array_equal(bits(sm["z"]), bits(l1[..., 3].mean(axis=1)))          # small integers: any order
    assert np.all(np.abs(sm["lambda"] - l1[..., 0].mean(axis=1)) <= order(l1[..., 0]))
    for nm, col in (("log_lambda", 0), ("log_mu", 1)):
        t = np.log(l1[..., col])
        bound = np.stack([R.log_sum_bound(l1[c][..., col]) for c in range(C)]) / n + order(t) + R.U * np.abs(sm[nm])
        assert np.all(np.abs(sm[nm] - t.mean(axis=1)) <= bound), nm


# ---------------------------------------------------------------------------------------------
# power: the comparison fails when the model is wrong (no further GPU run)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.POWER_CASES)
def test_a_wrong_model_fails_for_most_customers(L, monkeypatch, name):
    case, full, summ = _pair(monkeypatch, name)
    wrongs = [dict(wrong=w) for w in R.WRONG if case["D"] == 2 or w != "d2_shifted_by_two"] + [dict(mu_cap=0.5)]
    assert len(wrongs) == (7 if case["D"] == 2 else 6)
    for kw in wrongs:
        for c in range(case["chains"]):
            frac = R.any_bad(R.check_sums(summ["sums"][c], full["l1"][c], **kw)[0]).mean()
            print(f"{name}, chain {c}, {kw}: fails for {frac:.3f} of the customers")
            assert frac > 0.5, (kw, c, frac)

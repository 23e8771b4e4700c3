"""Production parity, deterministic: whole Philox-mode sweeps of the HIP sampler against the float64
model of tests/philox_sweep_ref.py (pinned to the reference by tests/test_philox_sweep_cpu.py), value
by value, through the Python API and the debug ABI only.

Procedure per case (the table is philox_sweep_ref.CASES): run HipSampler in Philox mode with the full
sink, read back the level-1 draws, the level-2 records, the log-likelihood and get_state() where the
case takes it.  For every chain and sweep s the device exposes on both sides:

* the device's own variates of (seed, chain_first + c, s) come from clv_debug_variates (t_l, t_m,
  log2 U, u_z, u_tau, -log U', the eta normal);
* the model runs from the DEVICE's state entering sweep s (lambda, mu of sweep s - 1: a stored draw,
  get_state, or init_state for s = 1) and the (beta, Sigma) the device recorded for that sweep's MH
  (bivariate: the draw belonging to sweep s; trivariate: the draw after sweep s - 1, the prior's
  beta_0 / gamma_00 for s = 1) — teacher forcing, so a borderline flip cannot cascade;
* z is compared exactly and tau, lambda, mu, eta and the stored log-likelihood value to the
  tolerances below, on every lane whose model decision margin is clear;
* the level-2 model is rerun on the device's own level-1 output (Y = log of it) with oracle.philox's
  hyper variates and compared with the record that draw belongs to: the bivariate draw after sweep s
  is sweep s + 1's, the first from init_state.

Tolerances (philox_sweep_ref.RTOL, tau_atol, L2_RTOL / L2_ATOL):

* lambda, mu, eta, the log-likelihood value: rtol 1e-12, the project's replay-parity figure.  The
  values are ll + Sigma_dd * t summed over <= 23 accepted steps (an fma against two roundings,
  ~1e-16 each) and one exp at <= 2 ulp: ~1e-15 in all.
* tau: rtol 1e-12 plus 8 * 2^-52 / (lambda + mu) absolute: the churned draw is -log(arg) / ml, and as
  arg -> 1 the log's condition number 1 / |log arg| turns arg's relative rounding (two exps at <= 3
  ulp between table and libm, two products and a sum at 3, the log at 2: 8 ulp) into an absolute
  error of tau of that many ulp of 1 divided by ml.
* level-2 record: rtol 1e-10, atol 1e-12 (test_replay_trajectory_matches_reference: S_n summed in
  another order).  Here the hyper variates agree with the oracle's only to <= 1e-12
  (test_device_hyper_variates_match_oracle) and Y is the device's log-scale state, within 2 ulp of
  the log of the stored draw: on the CPU model a 1e-12 relative perturbation of the variates with a
  2-ulp one of Y moves beta and Sigma by at most 6.9e-13 relative beyond the 1e-12 absolute term at
  these shapes (3.8e-11 elementwise on the entries near zero the absolute term is for), so ten times
  that stays below 1e-10 and the project's figures hold unchanged.

The cap: at most 0.1% of compared lanes per case may be set aside as borderline (model margin <=
1e-12); the CPU module asserts the model alone meets it at exactly these shapes (expected: none).
A lane set aside is dropped for that sweep only.

Measured on MI355X (all nine variants): no lane set aside; largest relative deviations tau 4.2e-15,
lambda 3.5e-15, mu 3.6e-15, eta 1.9e-15, log-likelihood 2.3e-16, beta 4.6e-13, Sigma 7.2e-12
elementwise (1.4e-10 on a Sigma01 near zero of the S = 0 case, inside the absolute term: 0 beyond it).

Power: the same device outputs are compared again with one thing wrong at a time in the model's
inputs (variates of sweep s + 1; chain key + 1; t_l and t_m swapped; the tau variate's branches
swapped; the bivariate level-2 draw's variates of sweep s instead of s + 1; the beta normals' slots
shifted by one); each must fail for more than half the customers, or the level-2 record outright.

The same comparison is pointed at the rest of the kernel by two more tables of philox_sweep_ref:

* INSTANCE_CASES (test_every_instance_matches_model): one case per compiled (D, K), D in {2, 3}, K in
  1..9, at N = 257 / 512 / 256, under the kernel the library picks and under CLV_PERSISTENT=0 (never
  =1).  launch_info()["persistent"] is asserted where capi.hip documents the instance's scratch (bi K
  <= 8, tri K <= 4: persistent; tri K = 9: never) and printed for bi K = 9 and tri K = 5..8 (MI355X
  build: bi 9 and tri 5 persistent, tri 6..8 launch per sweep).  The coverage events asserted per
  case are exactly those of INSTANCE_COVERAGE, which the CPU module pins to the model's free run.
  Measured over the 36 runs: no lane set aside; tau 2.8e-15, lambda 2.9e-15, mu 3.5e-15, eta 2.0e-15,
  log-likelihood 2.6e-16, beta 6.5e-12, Sigma 2.5e-11 elementwise, 0 beyond the absolute term.
* GRID_CASES (test_reduction_paths_match_model): 300 and 600 blocks per chain and 2 / 8 / 16 blocks per
  unit on the full CDNOW CBS tiled cyclically — the second slot of the level-2 workgroup's lanes, the
  strided unit loop, the unit arrival counters and batched unit sums over a partly filled last unit,
  customer indices >= 65,536.  Each case asserts its geometry before the run.  Power on the model's
  side: one block's rows (block 0, 256, 512, the one-customer last block) or the whole last unit left
  out of the level-2 model and of the log-likelihood's sum must fail both; the next chain key's
  variates must fail more than half the customers with index >= 65,536.  Measured over the 9 runs: 2
  of 306,690 lanes set aside at g_bi2_600u, none elsewhere; tau 6.8e-15, lambda 2.7e-15, mu 3.6e-15,
  eta 2.0e-15, log-likelihood 2.6e-16, level-2 record 5.4e-13 beyond the absolute term (beta 1.0e-10,
  Sigma 9.6e-10 elementwise on entries near zero).  All 45 runs together take 5 s.
  Seven more rows (philox_sweep_ref.SHARD_EDGE_GRID, 12 runs) are the unsharded side of
  tests/test_gpu_shard_edges.py, which holds every sharded exchange to them bit for bit: 1, 2, 6 and 10
  blocks with a last block of 1 / 256 / 44 / 53 lanes, and blocks_per_unit 4 and 2 at 6 and 5 blocks.
"""
import ctypes

import numpy as np
import pytest

from oracle import ref_cpu as orc
from tests import philox_sweep_ref as M

pytestmark = pytest.mark.gpu

# per chain: (sweeps compared at level 1, level-2 draws compared) — so a case cannot silently shrink
EXPECT = {"bi_k1": (6, 6), "bi_k2": (4, 4), "bi_k5": (7, 8), "tri_k3": (6, 6), "tri_k9": (5, 5), "bi_k1_s0": (6, 6)}


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _device_variates(L, seed, chain, sweep, n, S):
    """The sweep kernels' own variates of one (chain, sweep) (clv_debug_variates)."""
    tl, tm, ua, l2u = (np.zeros(max(n * S, 1), np.float32) for _ in range(4))
    uz, ut, ea, ez = (np.zeros(n) for _ in range(4))
    assert L.clv_debug_variates(seed, chain, sweep, n, S, _fp(tl), _fp(tm), _fp(ua), _dp(uz), _dp(ut), _dp(ea),
                                _dp(ez), _fp(l2u)) == 0
    sh = lambda a: a[: n * S].reshape(S, n)  # noqa: E731
    return dict(u_z=uz, u_tau=ut, e_alive=ea, eta_z=ez, t_l=sh(tl), t_m=sh(tm), log2_u=sh(l2u))


class Device:
    """What one run of a case left on the device, indexed by sweep."""

    def __init__(self, L, case, mp, persistent, blocks_per_unit=0, geometry=None, on_info=None):
        """``persistent``: the launch_info flag asserted (None: whatever the build chose, kept in
        self.persistent); ``geometry``: (blocks, blocks per unit, units per rank, global units) asserted
        against the handle before the run; ``on_info``: called with launch_info() and "before" / "after"
        ahead of the first launch and again after the last."""
        from mcmc_clv_model_amd.sampler import HipSampler, build_problem
        self.case, self.mp = case, mp
        self.C, self.T = case["chains"], M.n_sweeps_of(case)
        p = build_problem(M.case_frame(case), case["covs"], case["D"])
        assert p.N == mp.N and p.K == mp.K
        self.states = {}
        with HipSampler(p, mcmc=case["mcmc"], burnin=case["burnin"], thin=case["thin"], chains=self.C,
                        seed=case["seed"], n_mh_steps=case["S"], draw_sink="full",
                        chain_first=case["chain_first"], blocks_per_unit=blocks_per_unit) as s:
            self.persistent = s.launch_info()["persistent"]
            assert persistent is None or self.persistent == persistent
            if geometry is not None:
                nb, bpu, upr, units = geometry
                assert blocks_per_unit or L.clv_default_blocks_per_unit(mp.N) == bpu
                # the handle's own plan: launch_info counts the customer workgroups (+ 1 level-2 workgroup
                # per chain when persistent), partials() the unit partials [chain][stride][units per rank]
                assert s.launch_info()["workgroups"] == (nb + self.persistent) * self.C
                _, nd, stride = s.partials()
                assert stride == mp.K * mp.D + mp.D * (mp.D + 1) // 2 + 1 and nd == self.C * stride * upr
                assert upr == units == -(-nb // bpu)  # world size 1: every unit is this rank's
            if on_info is not None:
                on_info(s.launch_info(), "before")
            for act in case["drive"]:
                if act[0] == "run":
                    s.run(act[1])
                else:
                    self.states[s.sweeps_done] = s.get_state()
            assert s.sweeps_done == self.T
            if on_info is not None:
                on_info(s.launch_info(), "after")
            self.l1, self.l2, self.ll = s.read_draws()
        # the device's variates of every (chain, sweep), one sweep beyond the run and, for chain 0,
        # of the next chain key (the power checks' wrong inputs)
        cf = case["chain_first"]
        self.var = {(c, t): _device_variates(L, case["seed"], cf + c, t, mp.N, case["S"])
                    for c in range(self.C) for t in range(1, self.T + 2)}
        self.var_next_key = {t: _device_variates(L, case["seed"], cf + 1, t, mp.N, case["S"])
                             for t in range(1, self.T + 1)}

    def stored(self, s):
        c = self.case
        return 1 <= s <= c["burnin"] + c["mcmc"] and orc.is_stored(s, c["burnin"], c["thin"])

    def idx(self, s):
        return (s - 1 - self.case["burnin"]) // self.case["thin"]

    def post(self, c, s):
        """(lambda, mu) after sweep s as the device holds them, or None."""
        if s == 0:
            return self.mp.lam0, self.mp.mu0
        if self.stored(s):
            return self.l1[c, self.idx(s), :, 0], self.l1[c, self.idx(s), :, 1]
        if s in self.states:
            return self.states[s][0][c], self.states[s][1][c]
        return None

    def hyper_of(self, c, hs):
        """(beta, Sigma) of the level-2 draw belonging to sweep hs (see philox_sweep_ref.hyper_variates)."""
        D, K = self.mp.D, self.mp.K
        if D == 3 and hs == 0:
            return self.mp.hyper["beta_0"], self.mp.hyper["gamma_00"]
        at = hs - 1 if D == 2 else hs  # the get_state that shows it: taken after this sweep
        rec = M.l2_unpack(self.l2[c, self.idx(hs)], D, K) if self.stored(hs) else None
        st = (self.states[at][2][c], self.states[at][3][c]) if at in self.states else None
        if rec is not None and st is not None:  # one draw, two windows: the same bits
            assert np.array_equal(rec[0], st[0]) and np.array_equal(rec[1][np.triu_indices(D)], st[1][np.triu_indices(D)])
        return rec if rec is not None else st


def _close(got, ref, atol=0.0):
    """Within RTOL (+ atol) of a finite model value; a non-finite one (a power check's wrong model) is
    matched by the same value only."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(ref), np.abs(got - ref) <= M.RTOL * np.abs(ref) + atol, got == ref)


def compare(dev, chains, var_of=None, swap_t=False, swap_tau_branch=False, l2_sweep_shift=0, beta_slot_shift=0,
            l1_cache=None, drop=None, level2=True, model_kw=None, on_sweep=None):
    """Model against device over the given chains.  Returns dict(fail (chain, customer) mask, l2_fail, ll_fail,
    lanes, set_aside, n_l1, n_l2, dev_* largest relative deviations, edge counts).
    ``l1_cache``: a dict that keeps the level-1 model's results per (chain, sweep) between calls with the
    same level-1 inputs; ``drop`` (power checks only): a customer mask left out of the level-2 model's X
    and Y (nu_n unchanged) and of the log-likelihood's sum (still divided by N) — what a unit missing
    from the reduction would give; ``level2=False`` skips the level-2 comparison; ``model_kw`` (power
    checks only): further wrong-model switches of philox_sweep_ref.sweep_level1; ``on_sweep``: called for
    every stored sweep compared with (chain, sweep, entering state, leaving state, the stored level-1 row,
    the model's result, the lanes that differ before the margin gate, the lanes whose margin is clear)."""
    mp, case = dev.mp, dev.case
    D, N = mp.D, mp.N
    var_of = var_of or (lambda c, s: dev.var[c, s])
    out = dict(fail=np.zeros((len(chains), N), bool), l2_fail=False, ll_fail=False, lanes=0, set_aside=0, n_l1=0, n_l2=0,
               tau=0.0, lam=0.0, mu=0.0, eta=0.0, loglik=0.0, beta=0.0, Sigma=0.0, l2_net=0.0,
               x0=0, near_tx=0, near_T=0, clip=0, cap=0, z_lanes=0)

    def dev_max(key, got, ref, mask):
        if mask.any():
            out[key] = max(out[key], float((np.abs(got - ref) / np.abs(ref))[mask].max()))

    for ci, c in enumerate(chains):
        for s in range(1, dev.T + 1):
            ent, hyp, post = dev.post(c, s - 1), dev.hyper_of(c, s if D == 2 else s - 1), dev.post(c, s)
            if ent is not None and hyp is not None and post is not None:
                v = dict(var_of(c, s))
                if swap_t:
                    v["t_l"], v["t_m"] = v["t_m"], v["t_l"]
                r = l1_cache.get((c, s)) if l1_cache is not None else None
                if r is None:
                    r = mp.level1(ent[0], ent[1], hyp[0], hyp[1], v, swap_tau_branch=swap_tau_branch, **(model_kw or {}))
                    if l1_cache is not None:
                        l1_cache[c, s] = r
                clear = r["margin"] > M.RTOL
                out["n_l1"] += ci == 0
                out["lanes"] += N
                out["set_aside"] += int((~clear).sum())
                bad = ~_close(post[0], r["lam"]) | ~_close(post[1], r["mu"])
                dev_max("lam", post[0], r["lam"], clear)
                dev_max("mu", post[1], r["mu"], clear)
                out["x0"] += int((clear & (mp.x == 0) & (mp.t_x == 0)).sum())
                out["clip"] += int((clear & r["hit_clip"]).sum())
                out["cap"] += int((clear & r["hit_cap"]).sum())
                if dev.stored(s):
                    row = dev.l1[c, dev.idx(s)]
                    z_dev = row[:, 3] != 0.0
                    assert np.isin(row[:, 3], (0.0, 1.0)).all()
                    bad |= z_dev != r["z"]
                    bad |= ~_close(row[:, 2], r["tau"], M.tau_atol(ent[0], ent[1]))
                    dev_max("tau", row[:, 2], r["tau"], clear)
                    edges = M.near_edges(mp, z_dev, row[:, 2])
                    out["near_tx"] += int((clear & edges[0]).sum())
                    out["near_T"] += int((clear & edges[1]).sum())
                    out["z_lanes"] += int(clear.sum())
                    if D == 3:
                        bad |= ~_close(row[:, 4], r["eta"])
                        dev_max("eta", row[:, 4], r["eta"], clear)
                    # the stored value is the mean of the likelihood term (bi:423-428); a lane set
                    # aside contributes the term of the device's own draw
                    lik = np.where(clear, r["lik"], orc.lik_terms(mp.x, mp.T_cal, row[:, 0], row[:, 1], z_dev, row[:, 2]))
                    ll_dev, ll_ref = dev.ll[c, dev.idx(s)], lik.mean() if drop is None else lik[~drop].sum() / N
                    out["loglik"] = max(out["loglik"], abs(ll_dev - ll_ref) / abs(ll_ref))
                    if not _close(ll_dev, ll_ref):
                        out["ll_fail"] = True
                    if on_sweep is not None:
                        on_sweep(c, s, ent, post, row, r, bad, clear)
                out["fail"][ci] |= bad & clear
        # level 2: the draw belonging to sweep hs, from the device's own level-1 output
        for hs in range(1, dev.T + 2 if level2 else 0):
            rec = dev.hyper_of(c, hs) if (D == 2 or hs <= dev.T) else None
            if D == 2:
                src = dev.post(c, hs - 1)
                Y = None if src is None else np.log(np.column_stack(src))
            else:
                Y = np.log(dev.l1[c, dev.idx(hs)][:, [0, 1, 4]]) if dev.stored(hs) else None
            if rec is None or Y is None:
                continue
            out["n_l2"] += ci == 0
            l2 = mp.level2(case["seed"], case["chain_first"] + c, hs, Y, hsweep_of_variates=hs + l2_sweep_shift,
                           beta_slot_shift=beta_slot_shift, rows=None if drop is None else ~drop)
            for k, got in (("beta", rec[0]), ("Sigma", rec[1])):
                out[k] = max(out[k], float((np.abs(got - l2[k]) / np.abs(l2[k])).max()))
                net = float(M.l2_deviation(got, l2[k]).max())  # what the comparison bounds by L2_RTOL
                out["l2_net"] = max(out["l2_net"], net)
                if net > M.L2_RTOL:
                    out["l2_fail"] = True
    return out


# every case with the default kernel choice — the persistent kernel wherever its grid fits, except the
# trivariate K = 9 instance, whose private segment is above the bound for a persistent grid
# (capi.hip PERSIST_SCRATCH_MAX): launch per sweep either way — and three again with CLV_PERSISTENT=0
LAUNCH_PER_SWEEP_BY_DEFAULT = {"tri_k9"}
VARIANTS = [(n, "default") for n in M.CASES] + [(n, "launch_per_sweep") for n in ("bi_k2", "tri_k3", "tri_k9")]


@pytest.mark.parametrize("name,mode", VARIANTS, ids=[f"{n}-{m}" for n, m in VARIANTS])
def test_production_sweep_matches_model(L, monkeypatch, name, mode):
    case = M.CASES[name]
    if mode == "launch_per_sweep":
        monkeypatch.setenv("CLV_PERSISTENT", "0")
    else:
        monkeypatch.delenv("CLV_PERSISTENT", raising=False)
    persistent = mode == "default" and name not in LAUNCH_PER_SWEEP_BY_DEFAULT
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    dev = Device(L, case, mp, persistent)
    r = compare(dev, range(dev.C))
    print(f"{name} ({'persistent' if persistent else 'launch per sweep'}): {r['n_l1']} sweeps and {r['n_l2']} level-2 "
          f"draws per chain x {dev.C} chains, {r['lanes']} lanes compared, {r['set_aside']} set aside; largest relative "
          f"deviation tau {r['tau']:.2e} lambda {r['lam']:.2e} mu {r['mu']:.2e} eta {r['eta']:.2e} "
          f"log-lik {r['loglik']:.2e} beta {r['beta']:.2e} Sigma {r['Sigma']:.2e} (elementwise; {r['l2_net']:.2e} beyond the "
          f"absolute term); x = 0 lanes {r['x0']}, churned tau "
          f"near t_x {r['near_tx']} / near T {r['near_T']} of {r['z_lanes']}, clip lanes {r['clip']}, cap lanes {r['cap']}")
    assert (r["n_l1"], r["n_l2"]) == EXPECT[name]
    assert r["set_aside"] <= M.BORDERLINE_CAP * r["lanes"]
    assert not r["fail"].any(), f"{r['fail'].sum()} (chain, customer) lanes differ from the model"
    assert not r["ll_fail"], "a stored log-likelihood value differs from the model"
    assert not r["l2_fail"], "a level-2 record differs from the model"
    # the customers that go wrong first are among the compared lanes
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0
    if case["D"] == 3:  # sweep 1 proposes with gamma_00's variances: the clip and the cap are hit
        assert r["clip"] > 0 and r["cap"] > 0

    # ---- power: one thing wrong at a time in the model's inputs, same device outputs, chain 0
    def l1_share(**kw):
        return compare(dev, [0], **kw)["fail"].mean()

    shares = dict(next_sweep=l1_share(var_of=lambda c, s: dev.var[c, s + 1]),
                  next_chain_key=l1_share(var_of=lambda c, s: dev.var_next_key[s]),
                  tau_branch=l1_share(swap_tau_branch=True))
    if case["S"] > 0:
        shares["t_swapped"] = l1_share(swap_t=True)
    print(f"{name}: power, share of customers failing: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v > 0.5, (k, v)
    assert compare(dev, [0], beta_slot_shift=1)["l2_fail"]
    if case["D"] == 2:
        assert compare(dev, [0], l2_sweep_shift=-1)["l2_fail"]


# ---------------------------------------------------------------------------------------------
# every compiled instance (philox_sweep_ref.INSTANCE_CASES) and the level-2 reduction paths
# (GRID_CASES): the same comparison, pointed at the rest of the kernel
# ---------------------------------------------------------------------------------------------
def _report(name, dev, r):
    print(f"{name} ({'persistent' if dev.persistent else 'launch per sweep'}): {r['n_l1']} sweeps and {r['n_l2']} level-2 "
          f"draws per chain x {dev.C} chains, {r['lanes']} lanes compared, {r['set_aside']} set aside; largest relative "
          f"deviation tau {r['tau']:.2e} lambda {r['lam']:.2e} mu {r['mu']:.2e} eta {r['eta']:.2e} "
          f"log-lik {r['loglik']:.2e} beta {r['beta']:.2e} Sigma {r['Sigma']:.2e} (elementwise; {r['l2_net']:.2e} beyond the "
          f"absolute term); x = 0 lanes {r['x0']}, churned tau "
          f"near t_x {r['near_tx']} / near T {r['near_T']} of {r['z_lanes']}, clip lanes {r['clip']}, cap lanes {r['cap']}")


def _assert_parity(r, expect):
    assert (r["n_l1"], r["n_l2"]) == expect
    assert r["set_aside"] <= M.BORDERLINE_CAP * r["lanes"]
    assert not r["fail"].any(), f"{r['fail'].sum()} (chain, customer) lanes differ from the model"
    assert not r["ll_fail"], "a stored log-likelihood value differs from the model"
    assert not r["l2_fail"], "a level-2 record differs from the model"


def _set_kernel(monkeypatch, mode):
    """The kernel the library picks by itself, or the opt-out — never CLV_PERSISTENT=1: forcing a
    spilling instance into a resident grid makes workgroups wait out their bound (capi.hip)."""
    if mode == "launch_per_sweep":
        monkeypatch.setenv("CLV_PERSISTENT", "0")
    else:
        monkeypatch.delenv("CLV_PERSISTENT", raising=False)


# (sweeps, level-2 draws) per chain of every instance case: one run(3), every sweep stored
INSTANCE_EXPECT = {name: (3, 3) for name in M.INSTANCE_CASES}


def instance_persistent_by_default(D, K):
    """The instances capi.hip documents with 0 B of scratch run persistently; trivariate K = 9 (768 B
    per lane) never; bivariate K = 9 and trivariate K = 5..8: what the build's scratch gives (None)."""
    if (D == 2 and K <= 8) or (D == 3 and K <= 4):
        return True
    return False if (D, K) == (3, 9) else None


INSTANCE_RUNS = [(n, m) for n in M.INSTANCE_CASES for m in ("default", "launch_per_sweep")]


@pytest.mark.parametrize("name,mode", INSTANCE_RUNS, ids=[f"{n}-{m}" for n, m in INSTANCE_RUNS])
def test_every_instance_matches_model(L, monkeypatch, name, mode):
    case = M.INSTANCE_CASES[name]
    _set_kernel(monkeypatch, mode)
    persistent = instance_persistent_by_default(case["D"], len(case["covs"]) + 1) if mode == "default" else False
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    dev = Device(L, case, mp, persistent)
    if persistent is None:
        print(f"{name}: the build runs this instance {'persistently' if dev.persistent else 'launch per sweep'} by default")
    r = compare(dev, range(dev.C))
    _report(name, dev, r)
    _assert_parity(r, INSTANCE_EXPECT[name])
    # exactly the coverage events the model's free run of this case shows (asserted on the CPU)
    for ev in M.INSTANCE_COVERAGE[name]:
        assert r[ev] > 0, ev
    if mode != "default":
        return

    # ---- power: one thing wrong at a time in the model's inputs, same device outputs, chain 0
    def l1_share(**kw):
        return compare(dev, [0], level2=False, **kw)["fail"].mean()

    shares = dict(next_sweep=l1_share(var_of=lambda c, s: dev.var[c, s + 1]),
                  next_chain_key=l1_share(var_of=lambda c, s: dev.var_next_key[s]),
                  t_swapped=l1_share(swap_t=True))
    print(f"{name}: power, share of customers failing: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v > 0.5, (k, v)
    assert compare(dev, [0], beta_slot_shift=1)["l2_fail"]


GRID_EXPECT = {name: (2, 2) for name in M.GRID_CASES}  # one run(2), both sweeps stored
FIRST_LARGE_INDEX = 65536  # customer indices from here on need more than 16 bits of the Philox counter word


@pytest.mark.parametrize("name,mode", M.GRID_RUNS, ids=[f"{n}-{m}" for n, m in M.GRID_RUNS])
def test_reduction_paths_match_model(L, monkeypatch, name, mode):
    case = M.GRID_CASES[name]
    _set_kernel(monkeypatch, mode)
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    # the geometry this case is meant to reach, from N and blocks_per_unit by the plan rule
    assert M.grid_geometry(case) == case["geometry"]
    dev = Device(L, case, mp, case["modes"][mode], blocks_per_unit=case["blocks_per_unit"], geometry=case["geometry"])
    l1 = {}
    r = compare(dev, range(dev.C), l1_cache=l1)
    _report(name, dev, r)
    _assert_parity(r, GRID_EXPECT[name])
    assert r["x0"] > 0 and r["near_tx"] > 0 and r["near_T"] > 0

    # ---- power, on the model's side: a block (or the last unit) missing from the reduction breaks
    # the level-2 record and the log-likelihood; wrong variates break the large customer indices
    for what, (lo, hi) in case["drop"].items():
        assert 0 <= lo < hi <= mp.N
        drop = np.zeros(mp.N, bool)
        drop[lo:hi] = True
        d = compare(dev, [0], l1_cache=l1, drop=drop)
        print(f"{name}: power, customers [{lo}, {hi}) ({what}) left out: level-2 record off by {d['l2_net']:.1e}, "
              f"log-likelihood by {d['loglik']:.1e}")
        assert d["l2_fail"] and d["ll_fail"], what
    fail = compare(dev, [0], var_of=lambda c, s: dev.var_next_key[s], level2=False)["fail"][0]
    large = fail[FIRST_LARGE_INDEX:] if mp.N > FIRST_LARGE_INDEX else fail
    print(f"{name}: power, next_chain_key fails {large.mean():.2f} of the {large.size} customers with index >= "
          f"{FIRST_LARGE_INDEX if mp.N > FIRST_LARGE_INDEX else 0}")
    assert large.mean() > 0.5

"""The production sweep on customers far from CDNOW, against the float64 model of tests/philox_sweep_ref.py
value by value: the comparison of tests/test_gpu_production_sweep.py (its Device, compare, tolerances and
borderline cap, imported) pointed at the code the CDNOW cases never reach — cust_ztau's 700 cap on
ml (T - t_x), ml t_x and ml T with the division-free z test, tau = 700 / ml below t_x when both of tau's
exponents are capped, T == t_x, a span of 2^-40 T, t_x = 1e-9 T, T from 0.01 to 3650, x up to 20,000 in
log_post_fast's expanded quadratic, and a state accepted at the +-70 clip that goes back through log_fast
and exp_fast (lambda up to 1e8 and beyond, mu = e^-70, Sigma11 in the hundreds).

The frame is tests/helpers.edge_cbs (41 archetypes, tiled); the cases are philox_sweep_ref.EDGE_CASES:
e_bi1 (K = 1, N = 385, S = 20, 2 chains, 4 + 4 sweeps with a state read between), e_bi2 (K = 2, N = 385, S
= 13, 6 sweeps) and e_tri1 (trivariate, N = 257, S = 20, 2 chains, 6 sweeps).  N = 385 is two blocks and
two split workgroups, the second of either with one live lane.  Each case runs under the kernel the
library picks, under CLV_PERSISTENT=0 and, bivariate, under the forced split layout with CLV_SPLIT_RELAY=1
and =0; launch_info() is asserted before the run and after it.  The CPU module pins the same cases to the
reference (oracle_pin_edge.json, bitwise through the oracle) and asserts the model's own borderline
share (none) and coverage.

Compared per (chain, sweep), teacher forced from the device's own state with the device's own variates:
z exactly; tau (700 / ml below t_x included), lambda, mu, eta and the stored log-likelihood to RTOL and
tau_atol; the level-2 record to L2_RTOL / L2_ATOL; get_state() where the drive takes it, against the model
and bit for bit against the draw stored for the same sweep.

Tolerances, unchanged (derived before any device run):

* RTOL = 1e-12 on lambda, mu: lambda = exp(ll), so its relative error is ll's absolute one.  ll is
  log(lambda) of the entering state (log_fast against libm: <= 2 ulp of |ll| <= 70, ulp = 2^-46 = 1.4e-14)
  plus at most S = 20 accepted steps, each an fma on the device against a product and a sum in the model
  (<= 1 ulp of |ll| apart): <= 22 x 1.4e-14 = 3.1e-13 in the worst case of a walk that stays in |ll| >=
  64, and the exp's own 3 ulp.  Below RTOL; nothing regime-specific to add.
* tau_atol = 8 x 2^-52 / ml: its derivation (the relative error of the log's argument, over ml) does not
  depend on the regime; at the double cap the argument is e^-700 on both sides, log gives -700 to 2 ulp
  and tau = 700 / ml to ~1e-15 relative.
* the log-likelihood (a mean of x ll + (1 - z) lm - (lambda + mu) w over the customers) inherits
  lambda's bound where one term lambda w ~ 1e11 dominates the sum; the terms do not cancel to 1e-12.
* level 2: ten times the sensitivity measured on the CPU model for these cases (1.1e-12 / 2.4e-12 /
  3.1e-12 beyond the absolute term) stays below L2_RTOL = 1e-10, so the CDNOW figure carries over.

Coverage, from the device's own state (philox_sweep_ref.edge_events): exactly the events of EDGE_COVERAGE
on at least EDGE_MIN_LANES lanes each — x0, near_tx, clip, cap, cap_tx, cap_T, zz700, span0, tau_lt_tx,
clip_state.  |log eta| > 70 cannot be reached within the prior (see EDGE_EVENTS), so the eta draw's
|xe| <= 700 guard is exercised on its taken side only.

Power, on the model's side (same device outputs, one thing wrong in the model; the lanes are those the
correct model's margin leaves clear):

* no 700 cap in tau's exponents (the uncapped argument underflows to log 0): must fail on more than half
  of the cap_tx lanes;
* the clip at +-69: must fail every clip_state lane whose state changed in the sweep by more than RTOL (a
  lane that enters at the clip and accepts nothing is the same under any clip, up to the log_fast /
  exp_fast round trip of its state);
* P(alive)'s exponential from ml (t_x - T): the swapped form gives P >= 1, so it must fail every churned
  lane with 0 < ml (T - t_x) <= 700 (beyond 709 the swapped exponential overflows to NaN, which decides
  "churned" as the right formula does).

Measured on MI355X over the 10 runs (the four kernels of a case give the same figures): no lane of
40,048 set aside; largest relative deviations tau 3.0e-14, lambda 3.6e-15, mu 1.4e-14 (one ulp of 70 in
lm), eta 1.1e-15, log-likelihood 2.9e-16, beta 4.4e-15 and Sigma 6.8e-14 elementwise, level-2 record
1.4e-15 beyond the absolute term.  Coverage lanes, e_bi1 / e_bi2 / e_tri1, equal to the model's free
run: x0 784 / 294 / 396, near_tx 2544 / 970 / 1263, near_T 0 / 0 / 5, clip 5600 / 1997 / 2587, cap 6133 /
2281 / 2987, cap_tx 320 / 95 / 320, cap_T 1143 / 352 / 798, zz700 1078 / 339 / 734, span0 768 / 288 /
384, tau_lt_tx 320 / 95 / 320, clip_state 3212 / 979 / 289.  Power: no 700 cap fails 320 / 95 / 320 of
320 / 95 / 320 cap_tx lanes; the swapped span 1695 / 727 / 732 of as many churned lanes; the clip at 69
2608 / 964 / 168 lanes.  The module takes 4.6 s of wall time, 2.2 s of it loading the library and
creating the first handle; the slowest run is e_bi1 under CLV_PERSISTENT=0 at 0.24 s.  exp_fast on
[-700, 700] (test_gpu_parity.test_device_fast_exp_accuracy): at most 1 ulp from numpy.
"""
import numpy as np
import pytest

from tests import philox_sweep_ref as M
from tests.test_gpu_production_sweep import Device, _assert_parity, _close, _report, compare
from tests.test_gpu_split_model import L, R, _layout_check, _set_env  # noqa: F401  (L, R: fixtures)

pytestmark = pytest.mark.gpu

EXPECT = {"e_bi1": (8, 8), "e_bi2": (6, 6), "e_tri1": (6, 6)}  # (sweeps, level-2 draws) compared per chain
MODES = ("default", "launch_per_sweep", "split_relay", "split_helpers")
RUNS = [(n, m) for n, c in M.EDGE_CASES.items() for m in MODES if c["D"] == 2 or not m.startswith("split")]

_SEEN = dict(runs=0, lanes=0, set_aside=0, tau=0.0, lam=0.0, mu=0.0, eta=0.0, loglik=0.0, beta=0.0, Sigma=0.0, l2_net=0.0)


def _record(r):
    _SEEN["runs"] += 1
    for k in ("lanes", "set_aside"):
        _SEEN[k] += r[k]
    for k in ("tau", "lam", "mu", "eta", "loglik", "beta", "Sigma", "l2_net"):
        _SEEN[k] = max(_SEEN[k], r[k])
    print("module so far: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in _SEEN.items()))


def _kernel(mode, case, R):
    """(environment, launch_info() entries asserted before and after the run) of a kernel mode."""
    nb, C = -(-case["data"][1] // M.BLOCK), case["chains"]
    if mode == "default":  # bivariate K <= 8 and trivariate K <= 4 run persistently by themselves
        return {}, dict(persistent=True, workgroups=(nb + 1) * C)
    if mode == "launch_per_sweep":
        return {"CLV_PERSISTENT": "0"}, dict(persistent=False, layout=None, workgroups=nb * C)
    relay = mode == "split_relay"
    assert case["S"] > R
    return ({"CLV_PERSISTENT": "1", "CLV_PERSIST_LAYOUT": "split", "CLV_SPLIT_RELAY": "1" if relay else "0"},
            dict(persistent=True, layout="split", workgroups=(nb + 1) * C, physical_workgroups=(M.split_wgs(nb) + 1) * C,
                 relay_steps=R if relay else 0))


class _Lanes:
    """compare()'s on_sweep hook: per (chain, sweep) the lanes that differ from the model, the lanes whose
    margin is clear and the edge events computed from the device's own state and draw."""

    def __init__(self, mp):
        self.mp, self.bad, self.clear, self.ev, self.moved = mp, {}, {}, {}, {}

    def __call__(self, c, s, ent, post, row, r, bad, clear):
        self.bad[c, s], self.clear[c, s] = bad.copy(), clear.copy()
        self.ev[c, s] = M.edge_events(self.mp, ent[0], ent[1], row[:, 3] != 0.0, row[:, 2], post[0], post[1])
        self.ev[c, s]["zz"] = (ent[0] + ent[1]) * (self.mp.T_cal - self.mp.t_x)
        # the state changed by more than the log / exp round trip of a sweep that accepts nothing
        self.moved[c, s] = ~_close(post[0], ent[0]) | ~_close(post[1], ent[1])

    def count(self, event):
        return int(sum(e[event].sum() for e in self.ev.values()))


def _power(name, base, wrong, lanes_of):
    """(lanes, failing lanes) of a wrong model over the lanes ``lanes_of(key)`` gives, margin clear."""
    n = bad = 0
    for key in base.ev:
        lanes = lanes_of(key) & base.clear[key]
        n += int(lanes.sum())
        bad += int((lanes & wrong.bad[key]).sum())
    return n, bad


@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_edge_sweep_matches_model(L, R, monkeypatch, name, mode):
    case = M.EDGE_CASES[name]
    env, want = _kernel(mode, case, R)
    _set_env(monkeypatch, env)
    mp = M.ModelProblem(M.case_frame(case), case["covs"], case["D"])
    assert mp.N == case["data"][1]
    checks = []

    def on_info(info, when):
        _layout_check(L, f"{name}-{mode}", want)(info, when)
        checks.append(when)

    dev = Device(L, case, mp, want["persistent"], on_info=on_info)
    assert checks == ["before", "after"]
    base, l1 = _Lanes(mp), {}
    r = compare(dev, range(dev.C), l1_cache=l1, on_sweep=base)
    _report(f"{name}-{mode}", dev, r)
    _record(r)
    _assert_parity(r, EXPECT[name])
    assert len(base.ev) == dev.C * dev.T

    # the state read between the launches: the model's, and the very draw stored for that sweep
    for s, st in dev.states.items():
        for c in range(dev.C):
            m, clear = l1[c, s], l1[c, s]["margin"] > M.RTOL
            assert _close(st[0][c], m["lam"])[clear].all() and _close(st[1][c], m["mu"])[clear].all()
            assert np.array_equal(st[0][c], dev.l1[c, dev.idx(s), :, 0]) and np.array_equal(st[1][c], dev.l1[c, dev.idx(s), :, 1])
    assert (len(dev.states) > 0) == any(a[0] == "state" for a in case["drive"])

    # ---- coverage, from the device's own state: exactly the model's events, each on enough lanes
    n = {k: r[k] for k in M.CDNOW_EVENTS}
    n.update({k: base.count(k) for k in M.EDGE_EVENTS})
    print(f"{name}-{mode}: coverage lanes " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert {k for k, v in n.items() if v > 0} - set(M.EDGE_UNASSERTED) == set(M.EDGE_COVERAGE[name])
    assert min(n[k] for k in M.EDGE_COVERAGE[name]) >= M.EDGE_MIN_LANES
    assert np.isfinite(dev.l1).all() and np.isfinite(dev.l2).all() and np.isfinite(dev.ll).all()

    # ---- power: one thing wrong in the model at a time, same device outputs
    def wrong(**kw):
        w = _Lanes(mp)
        with np.errstate(all="ignore"):
            compare(dev, range(dev.C), level2=False, model_kw=kw, on_sweep=w)
        return w

    n_cap, bad_cap = _power(name, base, wrong(no_cap700=True), lambda k: base.ev[k]["cap_tx"])
    n_clip, bad_clip = _power(name, base, wrong(clip=69.0), lambda k: base.ev[k]["clip_state"] & base.moved[k])
    n_span, bad_span = _power(name, base, wrong(swap_span=True),
                              lambda k: ~(dev.l1[k[0], dev.idx(k[1]), :, 3] != 0.0) & (base.ev[k]["zz"] > 0)
                              & (base.ev[k]["zz"] <= 700.0))
    print(f"{name}-{mode}: power, failing lanes: no 700 cap {bad_cap} of {n_cap} cap_tx lanes, clip at 69 {bad_clip} of "
          f"{n_clip} clip_state lanes that moved, swapped span {bad_span} of {n_span} churned lanes with 0 < zz <= 700")
    assert n_cap >= M.EDGE_MIN_LANES and bad_cap > 0.5 * n_cap
    assert n_clip >= M.EDGE_MIN_LANES and bad_clip == n_clip
    assert n_span >= M.EDGE_MIN_LANES and bad_span == n_span

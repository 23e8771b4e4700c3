"""Every sharded exchange against the unsharded run, bit for bit, at the shard plan's edges
(tests/shard_edge_cases.py; the plans, the kernel choice and the model cases of the unsharded side are
asserted without a GPU in tests/test_shard_edges_cpu.py, and the unsharded runs themselves are held to
the float64 model by test_gpu_production_sweep.test_reduction_paths_match_model, rows
philox_sweep_ref.SHARD_EDGE_GRID).

Coverage: 7 plans — 4 with empty ranks (1, 2, 1 and 3 of them: N a multiple of the block on 2 ranks,
300 customers on 4, 1,281 on 4, the 2,357-customer sample on 8), 2 with a rank of one customer, 2 with a
partly filled last unit of blocks_per_unit 4 / 2 on a rank other than rank 0 — times 6 routes:

  (a) the sharded C path (sweep, copy_partials, synchronize, hyper), the gathered buffer preset to 7.0;
  (b) the in-process group's copy exchange, and for two_empty / abe_world8 the drop-in entry points
      (devices=[0] * world, shard="customers"; "full", and for the sample "summary+pct");
  (c) the group with exchange="auto" and "p2p" (a world with an empty rank is declined at creation);
  (d) the fused mail exchange (CLV_PERSISTENT=0; one host thread per rank);
  (e) the persistent peer exchange where no rank is empty, and the same driver with the default
      environment where one is: every rank must then have taken the fused exchange;
  (f) ShardedSampler on two processes over gloo, exact_empty, exchange="rccl" and "auto".

Per rank: get_state() (the lambda and mu slices, beta, Sigma), the level-2 records and the log-likelihood,
the level-1 draws ("full") or the summary sums ("summary"), and sweeps_done; an empty rank returns
zero-column level-1 arrays and everything else as every other rank.  8 sweeps (3 burn-in, 3 stored
draws), 2 chains, 6 MH steps, in calls of 1, 3 and 4 wherever the route takes run(n).  Every mail wait is
bounded by 2 s (CLV_WAIT_TIMEOUT_MS) and every thread is joined with a timeout: a missing unit is a wait
record in the failure message, never a silent stall.

Measured on an MI355X: the module's 47 tests take 29 s; the longest, 3.5 s, are the ones that start
processes — route (f)'s two ranks, and the mail routes of worlds of more than three ranks (see _mail).
The same figures and the defects this module found are in DESIGN.md §6, "The plan's edges"."""
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import shard_edge_cases as E
from tests.helpers import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(E.CASES)
WITH_EMPTY = [n for n in ALL if E.EMPTY_RANKS[n]]


def _kw(case, sink=None):
    return dict(E.RUN, seed=case["seed"], draw_sink=sink or case["sink"])


class _Refs(dict):
    """The unsharded run of each (case, sink), made once and only read afterwards."""

    def __missing__(self, key):
        from mcmc_clv_model_amd.sampler import HipSampler, build_problem
        name, sink = key
        case = E.CASES[name]
        p = build_problem(E.frame(case), E.covariates(case), case["D"])
        with HipSampler(p, blocks_per_unit=case["blocks_per_unit"], **_kw(case, sink)) as s:
            for n in E.CHUNKS:
                s.run(n)
            assert s.sweeps_done == E.SWEEPS
            st = s.get_state()
            sums = s.read_summary()[0] if sink == "summary" else None
            l1, l2, ll = s.read_draws(level1=sink == "full")
        for a in (*st, sums, l1, l2, ll):
            if a is not None:
                a.setflags(write=False)
        assert np.isfinite(l2).all() and np.isfinite(ll).all() and l2.shape[1] == 3
        self[key] = dict(p=p, state=st, sums=sums, l1=l1, l2=l2, ll=ll)
        return self[key]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


@pytest.fixture(autouse=True)
def _bounded_waits(monkeypatch):
    monkeypatch.setenv("CLV_WAIT_TIMEOUT_MS", "2000")
    monkeypatch.delenv("CLV_PERSISTENT", raising=False)


def _shards(case, p, sink=None):
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.sampler import HipSampler, make_prior
    plan = E.plan_of(case)
    prior = make_prior(p, p.N)
    out = []
    try:
        for r in range(case["world"]):
            b, e = plan.shard(r)
            assert (b, e) == case["shards"][r]
            out.append(HipSampler(Dm.slice_problem(p, b, e), n_global=p.N, shard_begin=r * plan.blocks_per_rank * E.BLOCK,
                                  world_size=case["world"], rank=r, blocks_per_rank=plan.blocks_per_rank,
                                  blocks_per_unit=plan.blocks_per_unit, prior=prior, device=0, **_kw(case, sink)))
    except Exception:
        for sh in out:
            sh.close()
        raise
    return out


def _check(case, shards, ref, sink=None):
    sink = sink or case["sink"]
    C, nd, D = E.RUN["chains"], 3, case["D"]
    for r, sh in enumerate(shards):
        b, e = case["shards"][r]
        assert sh.sweeps_done == E.SWEEPS, r
        lam, mu, beta, sigma = sh.get_state()
        assert lam.shape == mu.shape == (C, e - b), r
        assert np.array_equal(bits(lam), bits(ref["state"][0][:, b:e])), r
        assert np.array_equal(bits(mu), bits(ref["state"][1][:, b:e])), r
        assert np.array_equal(bits(beta), bits(ref["state"][2])) and np.array_equal(bits(sigma), bits(ref["state"][3])), r
        l1, l2, ll = sh.read_draws(level1=sink == "full")
        assert np.array_equal(bits(l2), bits(ref["l2"])) and np.array_equal(bits(ll), bits(ref["ll"])), r
        if sink == "full":
            assert l1.shape == (C, nd, e - b, D + 2), r
            assert np.array_equal(bits(l1), bits(ref["l1"][:, :, b:e])), r
        else:
            sums, k = sh.read_summary()
            assert k == nd and sums.shape == ref["sums"][:, :, b:e].shape and sums.shape[2] == e - b, r
            assert np.array_equal(bits(sums), bits(ref["sums"][:, :, b:e])), r


def _close(shards, group=None):
    if group is not None:  # the group before its shards (clv_group_destroy touches the shards)
        group.close()
    for sh in shards:
        sh.close()


# ---- (a) the sharded C path -------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_sharded_c_path(refs, name):
    """As test_gpu_parity.test_sharded_path_bitwise_equals_unsharded, with the gathered buffer preset to
    7.0: every rank, an empty one too, writes its whole slice at every exchange, and an empty rank's sweep
    enqueues nothing, still counts, and its level-2 draw is everyone's."""
    import torch
    case, ref = E.CASES[name], refs[name, E.CASES[name]["sink"]]
    shards = _shards(case, ref["p"])
    try:
        nd = shards[0].partials()[1]
        assert all(sh.partials()[1] == nd for sh in shards)
        gathered = torch.full((nd * case["world"],), 7.0, dtype=torch.float64, device="cuda")

        def exchange():
            for r, sh in enumerate(shards):
                sh.copy_partials(gathered.data_ptr() + r * nd * 8)
                sh.synchronize()
            for sh in shards:
                sh.hyper(gathered.data_ptr())

        if case["D"] == 2:
            exchange()  # bivariate: the draw of sweep 1 from the initial state
            assert not bool((gathered == 7.0).any())
        for _ in range(E.SWEEPS):
            for sh in shards:
                sh.sweep()
            exchange()
        for sh in shards:
            sh.synchronize()
        assert not bool((gathered == 7.0).any())
        for r in E.EMPTY_RANKS[name]:  # an empty rank's unit partials are zeros
            assert not bool(gathered[r * nd:(r + 1) * nd].any())
        _check(case, shards, ref)
    finally:
        _close(shards)


# ---- (b), (c) the in-process group -------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["copy", "auto", "p2p"])
@pytest.mark.parametrize("name", ALL)
def test_group(refs, name, exchange):
    """"copy" and "auto" finish with the unsharded bits and report the exchange used (shards sharing a
    card: the copy exchange).  "p2p" is declined when the group is created for a world with an empty
    rank, with clv_group_create's message; elsewhere it runs the peer stores between the resident grids
    and must keep them to the end — a fallback to copies would mean a wait ran out its bound."""
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd.sampler import HipGroup
    case, ref = E.CASES[name], refs[name, E.CASES[name]["sink"]]
    shards = _shards(case, ref["p"])
    g = None
    try:
        if exchange == "p2p" and E.EMPTY_RANKS[name]:
            with pytest.raises(_lib.ClvError, match="peer exchange not possible"):
                HipGroup(shards, "p2p")
            assert not any(sh.p2p_info()["connected"] for sh in shards)
            return
        g = HipGroup(shards, exchange)
        assert g.exchange == ("p2p" if exchange == "p2p" else "copy")
        for n in E.CHUNKS:
            g.run(n)
        assert g.exchange == ("p2p" if exchange == "p2p" else "copy")
        _check(case, shards, ref)
    finally:
        _close(shards, g)


@pytest.mark.parametrize("name,sink", [("two_empty", "full"), ("abe_world8", "full"), ("abe_world8", "summary+pct")])
def test_drop_in_over_empty_shards(name, sink):
    """mcmc_draw_parameters(..., devices=[0] * world, shard="customers") builds the empty shards itself:
    read_draws, read_summary, level1_summary and fit_multi's concatenations over zero-column arrays."""
    from mcmc_clv_model_amd import mcmc_draw_parameters, mcmc_draw_parameters_rfm_m
    from tests.test_gpu_multidevice import _same
    case = E.CASES[name]
    fn = mcmc_draw_parameters if case["D"] == 2 else mcmc_draw_parameters_rfm_m
    df, covs = E.frame(case), E.covariates(case)
    kw = dict(E.RUN, seed=case["seed"], trace=0, draw_sink=sink)
    one = fn(df, covs, **kw)
    many = fn(df, covs, devices=[0] * case["world"], shard="customers", **kw)
    assert many.pop("exchange") == "copy"
    _same(one, many)
    if sink == "full":
        assert all(a.shape == (3, case["N"], case["D"] + 2) for a in many["level_1"])
    else:
        assert many["summary"]["n_draws"] == 3 and many["summary"]["level1"].shape[0] == case["N"]
        assert many["summary"]["lambda"].shape == (E.RUN["chains"], case["N"])


# ---- (d), (e) the mail exchanges: one host thread per rank --------------------------------------
def _run_threads(shards, n):
    errs = []

    def go(sh):
        try:
            sh.run(n)
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(e)

    th = [threading.Thread(target=go, args=(sh,)) for sh in shards]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in th)
    assert not errs, "\n".join(str(e) for e in errs)  # (a wait that ran out its bound names what it waited for)


def _mail_run(case, ref, persistent):
    """Connect the shards' mail by device pointers and run the chunks; ``persistent``: what every rank's
    p2p_info must report before the run (the exchange clv_run then takes)."""
    import torch
    shards = _shards(case, ref["p"])
    try:
        info = [sh.p2p_info() for sh in shards]
        assert all(i["capable"] and not i["connected"] for i in info), info
        assert [i["persistent"] for i in info] == [persistent] * case["world"], info
        if case["D"] == 2:  # the initial draw from the initial state, through the all-gather path
            nd = shards[0].partials()[1]
            gathered = torch.full((nd * case["world"],), 7.0, dtype=torch.float64, device="cuda")
            for r, sh in enumerate(shards):
                sh.copy_partials(gathered.data_ptr() + r * nd * 8)
                sh.synchronize()
            for sh in shards:
                sh.hyper(gathered.data_ptr())
                sh.synchronize()
        ptrs = [i["mail_ptr"] for i in info]
        for sh in shards:
            sh.p2p_connect(ptrs=ptrs)
        assert all(sh.p2p_info()["connected"] for sh in shards)
        for n in E.CHUNKS:
            _run_threads(shards, n)
        _check(case, shards, ref)
    finally:
        _close(shards)


# Every rank's launch of a sweep spins on the other ranks' units, so the ranks' launches must run at the same
# time, each from its own stream, and streams beyond the process's hardware queues share a queue and run one
# after another (a wait would then run out its bound: csrc/group.hip).  A process opens 4 queues unless
# GPU_MAX_HW_QUEUES says otherwise, and reads it when it initialises the GPU: a world of more than three ranks
# on the one card runs in a fresh child process with 24.
MAIL_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CLV_ROOT"])
from tests import shard_edge_cases as E
from tests import test_gpu_shard_edges as T
name, persistent = sys.argv[1], sys.argv[2] == "1"
case = E.CASES[name]
T._mail_run(case, T._Refs()[name, case["sink"]], persistent)
print("MAIL_OK", flush=True)
"""


def _mail(refs, name, persistent):
    case = E.CASES[name]
    if case["world"] <= 3:
        return _mail_run(case, refs[name, case["sink"]], persistent)
    env = dict(os.environ, CLV_ROOT=ROOT, GPU_MAX_HW_QUEUES="24")  # (with this test's CLV_* settings)
    r = subprocess.run([sys.executable, "-c", MAIL_CHILD, name, "1" if persistent else "0"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("MAIL_OK"), r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", ALL)
def test_fused_mail_exchange(refs, monkeypatch, name):
    """CLV_PERSISTENT=0: one sweep launch per sweep and rank.  A rank without customers launches one
    workgroup per chain that draws its level 2 from its mail; the ranks with customers hold each launch
    until it has caught up (nobody waits for its units, so nothing else would)."""
    monkeypatch.setenv("CLV_PERSISTENT", "0")
    _mail(refs, name, persistent=False)


@pytest.mark.parametrize("name", E.PERSISTENT_CASES)
def test_persistent_peer_exchange(refs, name):
    case = E.CASES[name]
    assert not E.EMPTY_RANKS[name] and case["world"] <= 3 and all(c == "peer" for c in case["choice"])
    _mail(refs, name, persistent=True)


@pytest.mark.parametrize("name", WITH_EMPTY)
def test_world_with_an_empty_rank_agrees_on_one_exchange(refs, name):
    """The default environment: the ranks with customers could keep a persistent grid, the empty rank
    cannot.  Every rank decides from the plan alone, so all of them report, and take, the fused exchange."""
    case = E.CASES[name]
    assert "peer" in case["choice"] and "fused" in case["choice"]  # per rank the rule would differ
    _mail(refs, name, persistent=False)


# ---- (f) ShardedSampler, two processes over gloo -----------------------------------------------
WORKER = r"""
import json, os, sys
sys.path.insert(0, os.environ["CLV_ROOT"])
import numpy as np
import torch.distributed as dist
from tests import shard_edge_cases as E
from tests.helpers import bits
from mcmc_clv_model_amd.sampler import HipSampler, build_problem
from mcmc_clv_model_amd.distributed import ShardedSampler
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
case = E.CASES["exact_empty"]
p = build_problem(E.frame(case), E.covariates(case), case["D"])
kw = dict(E.RUN, seed=case["seed"], draw_sink=case["sink"])
with HipSampler(p, **kw) as s:  # the unsharded reference
    s.run(E.SWEEPS)
    ref = s.get_state()
    ref_sums = s.read_summary()[0]
    _, ref_l2, ref_ll = s.read_draws(level1=False)
dist.init_process_group("gloo")
ss = ShardedSampler(p, rank=rank, world=world, device=0, exchange=os.environ["CLV_EXCHANGE"], verify_sweeps=2, **kw)
for n in E.CHUNKS:
    ss.step(n)
ss.synchronize()
b, e = ss.begin, ss.end
got = ss.s.get_state()
_, l2, ll = ss.s.read_draws(level1=False)
sums, k = ss.s.read_summary()
ok = ((b, e) == case["shards"][rank] and ss.s.sweeps_done == E.SWEEPS and k == 3
      and got[0].shape == (kw["chains"], e - b) and sums.shape[2] == e - b
      and all(np.array_equal(bits(x), bits(y[:, b:e] if i < 2 else y)) for i, (x, y) in enumerate(zip(got, ref)))
      and np.array_equal(bits(sums), bits(ref_sums[:, :, b:e]))
      and np.array_equal(bits(l2), bits(ref_l2)) and np.array_equal(bits(ll), bits(ref_ll)))
print(json.dumps(dict(rank=rank, ok=bool(ok), n=e - b, exchange=ss.exchange, note=ss.p2p_note)), flush=True)
ss.close()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("exchange", ["rccl", "auto"])
def test_sharded_sampler_two_processes_empty_rank(exchange):
    """exact_empty: rank 1 owns no customer, cannot leave its job, and steps, verifies and returns rank
    0's level-2 bits — through the all-gather path, and through "auto", which must land on the fused
    exchange on both ranks, verified bitwise against the all-gather path."""
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), CLV_ROOT=ROOT, CLV_EXCHANGE=exchange, CLV_WAIT_TIMEOUT_MS="2000")
        env.pop("CLV_PERSISTENT", None)
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    for pr in procs:
        try:
            out, err = pr.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((pr.returncode, out, err))
    for r, (rc, out, err) in enumerate(outs):
        assert rc == 0, err[-3000:]
        res = json.loads(out.strip().splitlines()[-1])
        assert res["ok"] and res["rank"] == r and res["n"] == (256, 0)[r], res
        if exchange == "rccl":
            assert res["exchange"] == "rccl" and res["note"] is None, res
        else:
            assert res["exchange"] == "p2p", res
            assert res["note"] == "fused exchange verified bitwise against RCCL over 2 sweeps", res

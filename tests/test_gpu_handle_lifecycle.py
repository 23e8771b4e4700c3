"""Sampler handles give back what they took: free device memory (hipMemGetInfo) before and after
twenty create / destroy cycles, for every family of buffers clv_create can allocate — replay mode,
the persistent block layout (D = 3, K = 2, summary + percentile sink), the split layout, its relay
instance, the launch-per-sweep path with the full sink, a world-size-2 shard (the peer mail and the
peers table), and three creates that fail: two on a rejected environment value (with the stream
open and the sweep path decided, before the buffers), one on a percentile store larger than the card
(CLV_ENOMEM on the last allocation, with every other buffer of the handle live).  No sweep is run.

After three warming cycles free memory is F0; one further cycle measures the handle's footprint
(free before clv_create minus free after it); twenty more cycles end at F1.  The test fails if
F0 - F1 reaches one footprint.  Shapes: 4 chains and the largest customer count that keeps the
variant on its path (4 x 126 workgroups of the 504 the block layout admits on 256 CUs; 4 x 63 of the
split layout's 252), so that a footprint is tens of megabytes, far above the allocator's granularity:
a handle that leaks one of its large buffers on every cycle cannot stay under the bound.

What this cannot see: a buffer below the allocator's granularity (a forgotten 8-byte control word
moves no reading).  That class of leak is excluded by construction instead: every allocation of the
handle belongs to a member that frees it (csrc/internal.h DevPtr).
"""
import ctypes

import pytest

from tests.helpers import cdnow_tiled, with_covariates

pytestmark = pytest.mark.gpu

CHAINS = 4
N_BLOCK = 125 * 256  # (125 + 1) x 4 = 504 workgroups: the most the block layout admits on 256 CUs
N_SPLIT = 93 * 256   # (ceil(2 x 93 / 3) + 1) x 4 = 252 one-per-CU workgroups: the split layout's most
KNOBS = ("CLV_PERSISTENT", "CLV_PERSIST_LAYOUT", "CLV_SPLIT_RELAY", "CLV_DEFER", "CLV_MAIL_ALLOC",
         "CLV_WAIT_TIMEOUT_MS")

# name -> (D, K, customers, HipSampler keywords, environment, launch_info / p2p_info to expect,
#          what makes a failing create fail (an environment variable or a HipSampler keyword, its
#          value, the message), or None)
VARIANTS = {
    "replay": (2, 1, N_BLOCK, dict(rng="replay", mcmc=10, draw_sink="full"), {}, dict(persistent=False), None),
    "block_d3_k2_pct": (3, 2, N_BLOCK, dict(mcmc=40, draw_sink="summary+pct"), {"CLV_PERSIST_LAYOUT": "block"},
                        dict(persistent=True, layout="block"), None),
    "split": (2, 1, N_SPLIT, dict(mcmc=10, draw_sink="full"), {"CLV_PERSIST_LAYOUT": "split", "CLV_SPLIT_RELAY": "0"},
              dict(persistent=True, layout="split", relay_steps=0), None),
    "relay": (2, 1, N_SPLIT, dict(mcmc=10, draw_sink="full"), {"CLV_PERSIST_LAYOUT": "split", "CLV_SPLIT_RELAY": "1"},
              dict(persistent=True, layout="split", relay=True), None),
    "fused_full": (2, 1, N_BLOCK, dict(mcmc=10, draw_sink="full"), {"CLV_PERSISTENT": "0"},
                   dict(persistent=False), None),
    "world2": (2, 1, 2 * N_BLOCK, dict(mcmc=10, draw_sink="summary", world=2), {}, dict(p2p=True), None),
    "fail_wait_timeout": (2, 1, N_BLOCK, dict(mcmc=10, draw_sink="full"), {}, dict(persistent=True),
                          ("CLV_WAIT_TIMEOUT_MS", "nan", "CLV_WAIT_TIMEOUT_MS must be a finite decimal number of ms")),
    "fail_layout": (2, 1, N_SPLIT, dict(mcmc=10, draw_sink="full"), {}, dict(persistent=True),
                    ("CLV_PERSIST_LAYOUT", "bogus", "CLV_PERSIST_LAYOUT must be block or split")),
    # 4 chains x 400,000 draws x 32,000 customers x 8 B = 410 GB of (lambda, mu) pairs: more than the card has
    "fail_pct_store": (2, 1, N_BLOCK, dict(mcmc=10, draw_sink="summary+pct"), {}, dict(persistent=True),
                       ("mcmc", 400_000, "percentile store: ")),
}


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"
    return lib


@pytest.fixture(scope="module")
def free_bytes(L):
    """hipMemGetInfo's free bytes on the current device, from the HIP runtime the library loaded."""
    hip = ctypes.CDLL(None)
    if not hasattr(hip, "hipMemGetInfo"):
        hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipMemGetInfo.restype = ctypes.c_int

    def read():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return int(free.value)
    return read


def _maker(D, K, n, kw):
    """A function creating the variant's handle (rank 0 of the world for a sharded one)."""
    from mcmc_clv_model_amd import distributed as Dm
    from mcmc_clv_model_amd.sampler import HipSampler, build_problem, make_prior
    kw = dict(kw)
    world = kw.pop("world", 1)
    df = with_covariates(cdnow_tiled(n), K - 1) if K > 1 else cdnow_tiled(n)
    p = build_problem(df, [f"c{k}" for k in range(1, K)], D)
    kw.update(burnin=0, thin=1, chains=CHAINS, seed=1)
    if world > 1:
        plan = Dm.plan(p.N, world)
        b, e = plan.shard(0)
        kw.update(n_global=p.N, shard_begin=0, world_size=world, rank=0, blocks_per_rank=plan.blocks_per_rank,
                  blocks_per_unit=plan.blocks_per_unit, prior=make_prior(p, p.N))
        p = Dm.slice_problem(p, b, e)
    return lambda **over: HipSampler(p, **dict(kw, **over))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_twenty_cycles_return_the_memory(L, free_bytes, monkeypatch, name):
    D, K, n, kw, env, expect, bad = VARIANTS[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    make = _maker(D, K, n, kw)

    by_env = bool(bad) and bad[0].startswith("CLV_")

    def good_create():
        """(footprint, launch facts) of one create that succeeds, destroyed again."""
        if by_env:
            monkeypatch.delenv(bad[0])
        before = free_bytes()
        s = make()
        taken = before - free_bytes()
        info = dict(s.launch_info(), p2p=s.p2p_info()["capable"])
        s.close()
        if by_env:
            monkeypatch.setenv(bad[0], bad[1])
        return taken, info

    def cycle():
        if not bad:
            make().close()
            return
        with pytest.raises((ValueError, RuntimeError)) as err:  # CLV_EINVAL; any other code (ClvError)
            make(**({} if by_env else {bad[0]: bad[1]}))
        assert bad[2] in str(err.value)
        assert bad[2] in L.clv_last_error().decode()  # the failed create's message stands

    if by_env:
        monkeypatch.setenv(bad[0], bad[1])
    _, info = good_create()  # the variant is on the path it is meant to cover
    for key, want in expect.items():
        if key == "relay":
            assert info["relay_steps"] > 0, info
        else:
            assert info[key] == want, (key, info)
    for _ in range(3):
        cycle()
    f0 = free_bytes()
    footprint, _ = good_create()
    for _ in range(20):
        cycle()
    f1 = free_bytes()
    print(f"{name}: footprint {footprint / 2**20:.1f} MiB, F0 - F1 = {(f0 - f1) / 2**20:.3f} MiB")
    assert footprint >= 10 << 20, f"a footprint of {footprint} bytes is too small to tell a leak from noise"
    assert f0 - f1 < footprint, f"{f0 - f1} bytes lost over twenty cycles (one handle: {footprint})"

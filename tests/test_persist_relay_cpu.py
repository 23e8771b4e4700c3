"""The relay instance of the split layout, host side: clv_debug_split_relay_plan, the one function of
(S, R) from which the kernel takes which wavefront of a relayed row runs — and draws the variates of —
which of a sweep's S MH steps.  No GPU.

For every S in 0..20 and every supported relay point R: the owner's and the relay wavefront's step
ranges are contiguous, disjoint and together 0 .. S-1; each draws exactly the variates of the steps it
runs; the hand-over falls on a whole variate chunk (4 steps: a lane-column of the pool is written and
read by one wavefront only); and a sweep of S <= R steps is not relayed at all."""
import ctypes

import numpy as np
import pytest

RELAY_POINTS = (8, 12)
MH_CHUNK = 4
PRE_STEPS = 20


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    return _lib.lib()


def plan(L, S, R):
    out = np.full(8, -7, np.int32)
    assert L.clv_debug_split_relay_plan(S, R, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("R", RELAY_POINTS)
@pytest.mark.parametrize("S", range(PRE_STEPS + 1))
def test_plan_partitions_the_steps(L, S, R):
    ob, oe, rb, re_, odb, ode, rdb, rde = plan(L, S, R)
    own, relay = list(range(ob, oe)), list(range(rb, re_))
    assert ob <= oe and rb <= re_  # contiguous ranges
    assert not set(own) & set(relay)
    assert own + relay == list(range(S))  # together 0 .. S-1, the owner first
    assert list(range(odb, ode)) == own and list(range(rdb, rde)) == relay  # drawn = run
    if S > R:
        assert (oe, rb) == (R, R) and R % MH_CHUNK == 0
    else:
        assert relay == [] and own == list(range(S))


@pytest.mark.parametrize("S", range(PRE_STEPS + 1))
def test_relay_point_zero_is_no_relay(L, S):
    assert plan(L, S, 0) == [0, S, S, S, 0, S, S, S]


@pytest.mark.parametrize("S,R", [(-1, 8), (21, 8), (20, 10), (20, 4), (20, -8), (20, 16)])
def test_plan_rejects_what_is_not_built(L, S, R):
    out = np.zeros(8, np.int32)
    assert L.clv_debug_split_relay_plan(S, R, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0

"""The relay instance's draw plan, host side: clv_debug_split_draw_plan, the table from which the kernel
takes which wavefront draws which chunk of the next sweep's MH variates, and in which slot of the
current sweep.  No GPU.

Slots in time order: gap 1 (the relay wavefront's idle time between the (beta, Sigma) barrier and its
row's flag), gap 2 (between its row's reduction and the reduction's barrier), the window (after that
barrier).  A gap ends with the event after it, so a gap chunk may stay undrawn; the table names its
first drawer and its reader, which is the fallback in the window.  Checked for relay points 8 and 12
and every share the library can be built with (0..5):

  * every (row, chunk) with chunk * 4 < S has exactly one drawer, whether its gap got to it or not, for
    every S in R + 1 .. 20;
  * a gap-1 chunk of rows 4 / 5 lies below the relay wavefront's first chunk (an owner chunk);
  * a gap-2 chunk is one of the relay wavefront's own;
  * nothing is drawn into a pool column before its reader's last read of sweep s unless it is staged;
  * the fallback in the window is the chunk's reader."""
import ctypes
import itertools

import numpy as np
import pytest

RELAY_POINTS = (8, 12)
SHARES = (0, 1, 2, 3, 4, 5)  # 1..3 with gap 2; gap-1 chunks per helped row: 0, 0, 1, 2, 1, 2
MH_CHUNK = 4
PRE_STEPS = 20
NQ = PRE_STEPS // MH_CHUNK
ROWS = 6
WINDOW, GAP1, GAP2 = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    return _lib.lib()


def draw_plan(L, R, share):
    out = np.full((ROWS, NQ, 4), -7, np.int32)
    assert L.clv_debug_split_draw_plan(R, share, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return out


def relay_plan(L, S, R):
    out = np.full(8, -7, np.int32)
    assert L.clv_debug_split_relay_plan(S, R, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return [int(v) for v in out]


def reader_of(L, S, R, row, q):
    """The wavefront that runs chunk q of `row` in a sweep of S steps, from the relay plan."""
    if row < 4:
        return row
    ob, oe, rb, re_ = relay_plan(L, S, R)[:4]
    steps = set(range(q * MH_CHUNK, min((q + 1) * MH_CHUNK, S)))
    if steps <= set(range(ob, oe)):
        return row
    assert steps <= set(range(rb, re_)), "the cut falls between chunks"
    return row + 2


def test_built_share_is_one_of_the_table(L):
    out = np.full(1, -7, np.int32)
    assert L.clv_debug_split_draw_plan(8, -1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    assert int(out[0]) in SHARES


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("R", RELAY_POINTS)
def test_every_chunk_has_exactly_one_drawer(L, R, share):
    pl = draw_plan(L, R, share)
    gap_chunks = [(r, q) for r in range(ROWS) for q in range(NQ) if pl[r, q, 1] != WINDOW]
    for S in range(R + 1, PRE_STEPS + 1):
        live = [(r, q) for r in range(ROWS) for q in range(NQ) if q * MH_CHUNK < S]
        live_gap = [rq for rq in gap_chunks if rq in live]
        # either path of every gap chunk: its gap got to it (drawn there) or not (drawn in the window)
        subsets = itertools.chain.from_iterable(itertools.combinations(live_gap, k) for k in (0, 1, len(live_gap)))
        for reached in map(set, subsets):
            for r, q in live:
                wave, slot, staged, reader = (int(v) for v in pl[r, q])
                drawers = []
                if slot != WINDOW and (r, q) in reached:
                    drawers.append((wave, slot))
                if slot == WINDOW or (r, q) not in reached:
                    drawers.append((reader, WINDOW))  # the reader draws what its mask shows undrawn
                assert len(drawers) == 1
                assert reader == reader_of(L, S, R, r, q)  # the fallback is the chunk's reader
                if slot == WINDOW:
                    assert wave == reader and not staged


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("R", RELAY_POINTS)
def test_gap_chunks_are_where_they_may_be(L, R, share):
    pl = draw_plan(L, R, share)
    qr = R // MH_CHUNK
    n_gap1 = {0: 0, 1: 0, 2: 1, 3: 2, 4: 1, 5: 2}[share]
    for r in range(ROWS):
        for q in range(NQ):
            wave, slot, staged, reader = (int(v) for v in pl[r, q])
            assert 0 <= wave < 8 and 0 <= reader < 8 and slot in (WINDOW, GAP1, GAP2)
            if slot == GAP1:
                assert wave in (6, 7) and r in (wave - 6, wave - 2)  # the two rows on the owner's SIMD
                assert q < qr  # rows 4 / 5: an owner chunk (rows 0 / 1 too: the shares stay below it)
                assert staged  # its reader still reads sweep s's column: never into the pool
                assert reader == r
            elif slot == GAP2:
                assert r >= 4 and wave == r + 2 == reader and q >= qr  # the relay wavefront's own range
                assert not staged  # after its own last read of the column: straight into the pool
            else:
                assert not staged
            # before the reduction's barrier a pool column is written by its own reader only, and only
            # after that reader's last read of it (gap 2 follows the row's reduction)
            if slot != WINDOW and not staged:
                assert slot == GAP2 and wave == reader
        got = [q for q in range(NQ) if pl[r, q, 1] == GAP1]
        assert got == (list(range(n_gap1)) if r in (0, 1, 4, 5) else [])
        got2 = [q for q in range(NQ) if pl[r, q, 1] == GAP2]
        # gap 2: the first of the relay wavefront's chunks, as many as the library was built to try
        assert got2 == list(range(qr, qr + len(got2))) and (len(got2) >= 1) == (r >= 4 and 1 <= share <= 3)


@pytest.mark.parametrize("R", RELAY_POINTS)
def test_share_zero_is_the_window_only(L, R):
    pl = draw_plan(L, R, 0)
    assert (pl[:, :, 1] == WINDOW).all() and (pl[:, :, 0] == pl[:, :, 3]).all()


@pytest.mark.parametrize("R,share", [(0, 1), (10, 1), (8, 6), (8, -2), (16, 0)])
def test_plan_rejects_what_is_not_built(L, R, share):
    out = np.zeros(ROWS * NQ * 4, np.int32)
    assert L.clv_debug_split_draw_plan(R, share, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0

"""The split layout of the persistent sweep, host side (capi.hip persist_split_layout / _fits / _pays)
and the arithmetic it rests on.  No GPU.

A chain's 4 nb wave rows (64 customers each; a logical block = 4 rows = 256 customers) are dealt six
at a time, in order, to 512-thread workgroups of six customer wavefronts.  Dealt that way it is the
blocks b % 3 == 1 that fall across two workgroups, always 2 + 2 (rows 0-1 | rows 2-3): b = 1, 4, 7, ...
(the issue's text calls them "odd" blocks; block 4 is the first that shows the difference).  The level-2
lane pairing follows from it: row 3 of block b is polled by lane b + 1, or by lane b - 1 where b is its
wavefront's last lane (b % 64 == 63) — never across a wavefront, never by the lane of another split block.
"""
import ctypes

import numpy as np
import pytest

CASES = [(1, 1), (1, 2), (4, 3), (4, 7), (4, 93), (3, 93), (4, 94), (1, 256)]


@pytest.fixture(scope="module")
def L():
    from mcmc_clv_model_amd import _lib
    lib = _lib.lib()
    i32 = ctypes.c_int32
    lib.clv_debug_split_fits.argtypes = [i32, i32, i32, i32]
    lib.clv_debug_split_choice.argtypes = [i32, i32, i32, i32]
    lib.clv_debug_split_layout.argtypes = [i32, i32, ctypes.POINTER(i32)]
    for f in (lib.clv_debug_split_fits, lib.clv_debug_split_choice, lib.clv_debug_split_layout):
        f.restype = i32
    return lib


def layout(L, chains, nb):
    nwg = -(-2 * nb // 3)
    out = np.full((chains * (nwg + 1), 8), -7, np.int32)
    assert L.clv_debug_split_layout(chains, nb, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return nwg, out


@pytest.mark.parametrize("chains,nb", CASES)
def test_layout_hosts_every_row_once(L, chains, nb):
    nwg, tab = layout(L, chains, nb)
    assert tab.shape[0] == chains * (nwg + 1) and nwg == -(-4 * nb // 6)
    hosted = np.zeros((chains, nb, 4), int)
    l2 = np.zeros(chains, int)
    pieces = {}  # (chain, block) -> list of (first row in block, rows) per hosting workgroup
    for c, r0, n_rows, *_ in tab:
        if r0 < 0:
            l2[c] += 1
            continue
        assert r0 % 6 == 0 and 1 <= n_rows <= 6 and (n_rows == 6 or r0 + n_rows == 4 * nb)
        for r in range(r0, r0 + n_rows):
            hosted[c, r // 4, r % 4] += 1
        for b in sorted({r // 4 for r in range(r0, r0 + n_rows)}):
            rows = [r % 4 for r in range(r0, r0 + n_rows) if r // 4 == b]
            pieces.setdefault((c, b), []).append((rows[0], len(rows)))
    assert (hosted == 1).all() and (l2 == 1).all()
    for (c, b), pc in pieces.items():
        if b % 3 == 1:
            assert sorted(pc) == [(0, 2), (2, 2)], (c, b, pc)  # split, and always 2 + 2
        else:
            assert pc == [(0, 4)], (c, b, pc)                   # whole


@pytest.mark.parametrize("chains,nb", CASES)
def test_record_table(L, chains, nb):
    """Every block's slot is written exactly once (kind 1 whole, kind 2 the prefix of a split block),
    every split block's two extension records exactly once, by the workgroup hosting those rows."""
    nwg, tab = layout(L, chains, nb)
    n_rec = nb + 2 * ((nb + 1) // 3)
    writes = np.zeros((chains, n_rec), int)
    for c, r0, n_rows, k0, b0, k1, b1, ext in tab:
        if r0 < 0:
            assert (k0, b0, k1, b1, ext) == (-1,) * 5
            continue
        rows = set(range(r0, r0 + 6))  # (rows past the chain's end are inactive lanes: stored as 0.0)
        for kind, b in ((k0, b0), (k1, b1)):
            if kind < 0:
                assert b < 0 or b >= nb
                continue
            assert 0 <= b < nb
            if kind == 1:
                assert {4 * b + q for q in range(4)} <= rows and b % 3 != 1
                writes[c, b] += 1
            elif kind == 2:
                assert {4 * b, 4 * b + 1} <= rows and 4 * b + 2 not in rows and b % 3 == 1
                writes[c, b] += 1
            else:
                assert kind == 3 and {4 * b + 2, 4 * b + 3} <= rows and 4 * b + 1 not in rows and b % 3 == 1
                assert ext == nb + 2 * (b // 3) and ext + 1 < n_rec
                writes[c, ext] += 1
                writes[c, ext + 1] += 1
        if k0 != 3:
            assert ext == -1
    assert (writes == 1).all()


@pytest.mark.parametrize("nb", [1, 2, 3, 7, 64, 65, 93, 94, 127, 128, 191, 192, 255, 256])
def test_level2_lane_pairing(nb):
    """The level-2 workgroup's second slots (persist_level2, SPLIT): lane b polls row 2 of its own
    split block, one neighbour of the same wavefront row 3; no lane is asked for two records."""
    second = {}
    for b in range(nb):
        if b % 3 != 1:
            continue
        partner = b + 1 if b % 64 != 63 else b - 1
        assert partner // 64 == b // 64 and 0 <= partner < 256 and partner % 3 != 1
        for lane, rec in ((b, nb + 2 * (b // 3)), (partner, nb + 2 * (b // 3) + 1)):
            assert lane not in second
            second[lane] = rec
    n_ext = 2 * ((nb + 1) // 3)
    assert sorted(second.values()) == list(range(nb, nb + n_ext))


def test_eligibility(L):
    ok = lambda C, nb, n_cu=256, bpc=1: bool(L.clv_debug_split_choice(C, nb, bpc, n_cu))  # noqa: E731
    fits = lambda C, nb, n_cu=256, bpc=1: bool(L.clv_debug_split_fits(C, nb, bpc, n_cu))  # noqa: E731
    assert ok(4, 93) and fits(4, 93)              # c2 (bivariate; the trivariate c3, on the same customers,
                                                  # never takes this layout): 4 x (62 + 1) = 252 of 256 CUs, margin 4
    assert not ok(4, 94) and not fits(4, 94)      # 4 x (63 + 1) = 256
    assert not ok(1, 496) and not fits(1, 496)    # one level-2 lane per block: nb <= 256
    assert not ok(4, 257) and not fits(1, 257)
    assert not ok(4, 40) and fits(4, 40)          # the block layout does not double up: 164 <= 256
    assert ok(1, 129) is False and fits(1, 129)   # nor do 130: the model test of nb = 129 has to force the layout
    assert fits(1, 256) and ok(1, 256)            # 172 CUs; its 257 block workgroups double up on 256
    assert ok(1, 256, 200) and not fits(1, 256, 173) and fits(1, 256, 174)  # margin max(1, n_cu / 64)
    assert not fits(4, 93, 256, 0) and not fits(0, 93) and not fits(4, 0)


def test_prefix_and_rows_sum_to_the_block_partial_bitwise():
    """The split hand-off: first half stores p = r0 + r1, second half r2 and r3, the level-2 lane forms
    (p + r2) + r3 — the block layout's ((r0 + r1) + r2) + r3, bit for bit (same operations, same
    order), on doubles of mixed magnitude and sign, zeros of both signs included."""
    rng = np.random.default_rng(20261020)
    r = rng.standard_normal((4, 200_000)) * 10.0 ** rng.integers(-12, 13, (4, 200_000))
    r[:, :64] = 0.0
    r[2, :32] = -0.0
    r[:, 64:128] = np.array([1e308, 1e308, -1e308, 1.0])[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        prefix = r[0] + r[1]
        split = (prefix + r[2]) + r[3]
        whole = ((r[0] + r[1]) + r[2]) + r[3]
        other = (r[0] + r[1]) + (r[2] + r[3])
    assert np.array_equal(split.view(np.uint64), whole.view(np.uint64))
    # and it is the order that matters: another association differs somewhere on this data
    assert not np.array_equal(other.view(np.uint64), whole.view(np.uint64))
    # the level-2 lane's accumulator starts from 0.0, as for a whole block: 0.0 + x
    assert np.array_equal((0.0 + split).view(np.uint64), (0.0 + whole).view(np.uint64))

"""The two launch tables that decide whether a persistent sweep can finish, checked without a GPU.

csrc/placement.cpp holds them as pure functions: det_slot_table (the split deterministic sweep's
slot table: a block past the co-resident limit never starts and the ticket sweep waits for it) and
place_by_load / sys_iso_pad / check_placement (the systolic fast sweep's block -> wave map: a wave
missing from it stalls its neighbours).  The library's own functions run here, through
mf_debug_det_slot_table and mf_debug_sys_placement, on random inputs from a fixed seed.
"""
import ctypes as C

import numpy as np
import pytest

from mfhip import _lib as L

SINGLE, HELPER = 1, 2  # plan.hpp kDetWaveSingleItem, kDetWaveHelper


# ---------------------------------------------------------------------------------------------
# the systolic sweep's block -> wave map

def sys_placement(load, cap, iso):
    nw = len(load)
    load = np.ascontiguousarray(load, dtype=np.float64)
    place = np.full(nw + 24 * iso, -2, dtype=np.int32)  # -2: never written
    pad = C.c_int32(-1)
    L.check(L.lib().mf_debug_sys_placement(L.ptr(load, C.c_double), nw, cap, iso, C.byref(pad), L.ptr(place, C.c_int32)))
    n = nw + 8 * pad.value
    assert (place[n:] == -2).all(), "entries written past nw + 8 pad"
    return pad.value, place[:n]


def xcd_range(nw, x):
    """The contiguous wave range of XCD x: (base, length)."""
    return x * (nw // 8) + min(x, nw % 8), nw // 8 + (x < nw % 8)


PLACEMENT_NW = [1, 3, 7, 8, 9, 31, 255, 256, 257, 263, 511, 512, 520, 600, 1004, 1100]


@pytest.mark.parametrize("nw", PLACEMENT_NW)
def test_sys_placement_invariants(nw):
    rng = np.random.default_rng(1000 + nw)
    for cap in (1024, 2048):
        if nw > cap:
            continue  # such a superstep is never one systolic launch
        for iso in (0, 1, 2, 8):
            load = rng.uniform(1.0, 1e6, nw)
            pad, place = sys_placement(load, cap, iso)
            case = f"nw={nw} cap={cap} iso={iso} pad={pad}"
            assert pad >= 0 and len(place) == nw + 8 * pad, case
            assert nw + 8 * pad <= cap, case
            assert (place == -1).sum() == 8 * pad, case
            assert sorted(place[place >= 0].tolist()) == list(range(nw)), case
            if iso == 0 or nw < 512:
                # <= 256 waves: an XCD holds <= 32, its emptiest CU slot one; 257..511: sys_iso_pad gives 0
                assert pad == 0, case
            for x in range(8):
                base, length = xcd_range(nw, x)
                mine = place[x::8]
                waves = mine[mine >= 0]
                assert len(mine) == (length + pad if length else 0), case
                assert ((waves >= base) & (waves < base + length)).all(), (case, x)
                if length == 0:
                    continue
                # Block x + 8 kk sits on CU slot kk % 32 of the XCD.  The heaviest wave is the first
                # member of the first of the slots holding the fewest blocks: slot 0 when every slot
                # holds equally many (n <= 32 or a multiple of 32), else slot n % 32.
                n = length + pad
                slot = 0 if n <= 32 else n % 32
                heaviest = base + int(np.argmax(load[base:base + length]))
                assert mine[slot] == heaviest, (case, x)
                if pad > 0:  # ... and the empty blocks leave it alone on that CU
                    assert (mine[slot + 32::32] == -1).all(), (case, x)


@pytest.mark.parametrize("nw,cap,iso,pad", [(nw, cap, iso, iso) for nw in (520, 600) for cap in (1024, 2048)
                                            for iso in (1, 2, 8)] +
                         [(512, cap, iso, 0) for cap in (1024, 2048) for iso in (1, 2, 8)] +
                         [(1100, 2048, 1, 3), (1100, 2048, 2, 6), (1100, 2048, 8, 0)])
def test_sys_iso_pad_pinned(nw, cap, iso, pad):
    """sys_iso_pad's values on the shapes the benchmarks reach (the pad > 0 branch of the placement).
    65 to 95 blocks per XCD: one empty block per isolated wave.  512 waves are exactly two per CU, so
    any empty block would make a three-block CU: none.  1100 (138 per XCD, four on the emptiest
    slot): three per isolated wave, and none for eight waves, which would need more than the three
    per wave the search allows."""
    got, place = sys_placement(np.random.default_rng(7).uniform(1.0, 1e6, nw), cap, iso)
    assert got == pad and (place == -1).sum() == 8 * pad


def test_sys_placement_rejects_bad_arguments():
    lib = L.lib()
    load = np.ones(8)
    out = np.zeros(8 + 24 * 8, dtype=np.int32)
    pad = C.c_int32(0)
    for nw, cap, iso in [(0, 1024, 0), (8, 7, 0), (8, 1024, -1), (8, 1024, 9)]:
        assert lib.mf_debug_sys_placement(L.ptr(load, C.c_double), nw, cap, iso, C.byref(pad),
                                          L.ptr(out, C.c_int32)) == L.MF_ERR_INVALID
    assert lib.mf_debug_sys_placement(None, 8, 1024, 0, C.byref(pad), L.ptr(out, C.c_int32)) == L.MF_ERR_INVALID


# ---------------------------------------------------------------------------------------------
# the split deterministic sweep's slot table

def det_slot_table(begin, count, flags, max_blocks, alone, period):
    nw = len(count)
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    room = 4 * nw + 4
    bo, co, fo = np.zeros(room, np.int64), np.zeros(room, np.int32), np.zeros(room, np.int32)
    n = C.c_int64(-1)
    st = L.lib().mf_debug_det_slot_table(L.ptr(begin, C.c_int64), L.ptr(count, C.c_int32), L.ptr(flags, C.c_int32), nw,
                                         max_blocks, alone, period, L.ptr(bo, C.c_int64), L.ptr(co, C.c_int32),
                                         L.ptr(fo, C.c_int32), C.byref(n))
    return st, list(zip(bo[:max(n.value, 0)].tolist(), co[:max(n.value, 0)].tolist(), fo[:max(n.value, 0)].tolist()))


def random_waves(rng, nw, hot):
    """nw waves: `hot` single-item ones of 5000..8000 entries, the others 0..200 entries (about one
    in seven empty, one in five single-item); begin = the entries before the wave."""
    count = rng.integers(1, 201, nw)
    count[rng.random(nw) < 1 / 7] = 0
    flags = (rng.random(nw) < 1 / 5).astype(np.int32) * SINGLE
    hot_at = rng.choice(nw, size=min(hot, nw), replace=False)
    count[hot_at] = rng.integers(5000, 8001, len(hot_at))
    flags[hot_at] = SINGLE
    begin = np.concatenate([[0], np.cumsum(count)[:-1]]) if nw else np.zeros(0, np.int64)
    return begin, count, flags


SLOT_NW = [0, 1, 2, 5, 64, 300, 700, 1000]


@pytest.mark.parametrize("nw", SLOT_NW)
def test_det_slot_table_invariants(nw):
    rng = np.random.default_rng(2000 + nw)
    for alone in (0, 1):
        for period in (8, 16, 256):
            for max_blocks in (1024, 4096):
                for hot in (0, 1, 3, 100):
                    begin, count, flags = random_waves(rng, nw, hot)
                    st, slots = det_slot_table(begin, count, flags, max_blocks, alone, period)
                    case = f"nw={nw} alone={alone} period={period} max_blocks={max_blocks} hot={hot}"
                    assert st == L.MF_OK, (case, L.lib().mf_last_error())
                    check_slot_table(case, begin, count, flags, slots, max_blocks, alone, period)


def check_slot_table(case, begin, count, flags, slots, max_blocks, alone, period):
    nw = len(count)
    assert len(slots) % 2 == 0 and len(slots) <= 4 * nw + 4 and len(slots) // 2 <= max_blocks, case
    # every wave with entries exactly once; a slot without entries is a helper or empty, never work
    work = sorted(s for s in slots if s[1] > 0)
    assert work == sorted((int(b), int(c), int(f)) for b, c, f in zip(begin, count, flags) if c > 0), case
    assert all(s == (0, 0, 0) or s[2] == HELPER for s in slots if s[1] == 0), case
    for x, s in enumerate(slots):
        if s[1] > 0 and s[2] & SINGLE:  # a single-item wave leads its block, its helper beside it
            assert x % 2 == 0 and slots[x + 1] == (s[0], 0, HELPER), (case, x)
        if s[2] == HELPER:
            assert x % 2 == 1 and slots[x - 1][2] & SINGLE and slots[x - 1][0] == s[0], (case, x)
    blocks = [(slots[x], slots[x + 1]) for x in range(0, len(slots), 2)]
    empty = [b for b, blk in enumerate(blocks) if blk == ((0, 0, 0), (0, 0, 0))]
    busy = [blk for blk in blocks if blk != ((0, 0, 0), (0, 0, 0))]
    # the single-item blocks first, longest chain first
    lead_single = [bool(blk[0][2] & SINGLE) for blk in busy]
    assert lead_single == sorted(lead_single, reverse=True), case
    chains = [blk[0][1] for blk in busy if blk[0][2] & SINGLE]
    assert chains == sorted(chains, reverse=True), case
    if not busy:  # a table with no work at all: one empty block stands for it
        assert empty == [0], case
    elif not alone:
        assert not empty, case
    else:
        # the chains within half of the longest keep a CU each (at most 64 and period / 2 of them):
        # block b shares block (b mod period)'s CU, so those positions stay empty from `period` on
        H = min(sum(2 * c >= chains[0] for c in chains), 64, period // 2) if chains else 0
        assert all(b >= period and b % period < H for b in empty), case
        assert not empty or len(blocks) <= max_blocks, case


def test_det_slot_table_refuses_more_blocks_than_fit():
    """A block past the co-resident limit would never start: 64 multi-item waves are 32 blocks."""
    count = np.full(64, 10)
    begin = np.arange(64) * 10
    st, _ = det_slot_table(begin, count, np.zeros(64), 8, 1, 256)
    assert st == L.MF_ERR_INVALID
    assert b"det slot table: more blocks than can be resident at once" in L.lib().mf_last_error()


def test_det_slot_table_rejects_bad_arguments():
    lib = L.lib()
    one = np.zeros(8, np.int64)
    i32 = np.zeros(8, np.int32)
    n = C.c_int64(0)
    args = lambda nw, mb, period: (L.ptr(one, C.c_int64), L.ptr(i32, C.c_int32), L.ptr(i32, C.c_int32), nw, mb, 1, period,
                                   L.ptr(one, C.c_int64), L.ptr(i32, C.c_int32), L.ptr(i32, C.c_int32), C.byref(n))
    for nw, mb, period in [(-1, 8, 8), (1, 0, 8), (1, 8, 0)]:
        assert lib.mf_debug_det_slot_table(*args(nw, mb, period)) == L.MF_ERR_INVALID
    assert lib.mf_debug_det_slot_table(None, None, None, 1, 8, 1, 8, L.ptr(one, C.c_int64), L.ptr(i32, C.c_int32),
                                       L.ptr(i32, C.c_int32), C.byref(n)) == L.MF_ERR_INVALID

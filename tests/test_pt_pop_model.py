"""The deal of the persistent kernels' queues (csrc/device/rt_pt_queue.h pt_pop) as a plain-Python model of ONE call by one wave, and the
header's host+device bit helpers against it (through the test hooks, on the host — no GPU).  The model is the specification: what a call
hands to which lane, what it leaves in the bitmap, where the cursor stands and what the count is.  test_gpu_pt_pop.py holds the device
function to it."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_NONE = 0xFFFFFFFF


def set_bits(v):
    """positions of the set bits of a 32-bit word, lowest first"""
    return [b for b in range(32) if (v >> b) & 1]


def nth_bit(v, n):
    """position of the n-th set bit (n from 0)"""
    return set_bits(v)[n]


def low_bits(v, n):
    """the lowest n set bits of v"""
    return sum(1 << b for b in set_bits(v)[:n])


def pop_model(bitmap, nw, cursor, count, want, from_start=False):
    """One pt_pop call.  bitmap: list of nw words (changed in place); want: 64-bit mask of the lanes that want a path.
    Returns (per-lane results [64], cursor, count).

    The wave looks at up to 64 words at a time, word cursor + i (mod nw) for lane i < nw, and takes set bits in that order, lowest bit
    first, until every wanting lane has one or the ring has been swept once (ceil(nw / 64) looks).  The wanting lane of rank r (r-th set
    bit of `want`) gets the r-th path taken.  After a look that met the need the cursor is the last word touched if that kept bits, else
    the word after it; after a look that did not, it moves on by 64 words (mod nw)."""
    if from_start:
        cursor = 0
    need = bin(want).count("1")
    paths = []
    swept = 0
    while swept < nw and len(paths) < need:
        next_cursor = cursor + 64
        last = None
        for i in range(min(64, nw)):
            w = (cursor + i) % nw
            room = need - len(paths)
            if bitmap[w] == 0 or room <= 0:
                continue
            take = low_bits(bitmap[w], room)
            bitmap[w] &= ~take
            paths += [w * 32 + b for b in set_bits(take)]
            last = w
        if last is not None and len(paths) >= need:
            next_cursor = last if bitmap[last] else last + 1
        cursor = next_cursor % nw
        swept += 64
    got, r = [PT_NONE] * 64, 0
    for lane in range(64):
        if (want >> lane) & 1:
            if r < len(paths):
                got[lane] = paths[r]
            r += 1
    return got, cursor, count - len(paths)


# ---- the model's own behaviour on cases small enough to check by eye -------------------------------------------------------------------

def test_model_deals_by_rank_cuts_a_word_and_parks_the_cursor_on_it():
    bm = [0b1011_0000, 0, 0b0110]
    got, cur, cnt = pop_model(bm, 3, 2, 5, want=0b1010_0001)  # three lanes want; the sweep starts at word 2
    assert [got[0], got[5], got[7]] == [2 * 32 + 1, 2 * 32 + 2, 0 * 32 + 4] and got.count(PT_NONE) == 61
    assert bm == [0b1010_0000, 0, 0] and cur == 0 and cnt == 2
    got, cur, cnt = pop_model(bm, 3, cur, cnt, want=(1 << 64) - 1)  # more wanted than there is: one sweep, the rest get nothing
    assert got[:2] == [5, 7] and got[2:] == [PT_NONE] * 62 and bm == [0, 0, 0] and cnt == 0
    assert cur == (0 + 64) % 3


def test_model_moves_past_a_word_it_emptied_and_from_start_sweeps_from_word_zero():
    bm = [0, 0b11, 0b1]
    got, cur, cnt = pop_model(bm, 3, 1, 3, want=0b11)
    assert got[:2] == [32, 33] and cur == 2 and bm == [0, 0, 1]
    bm = [0b1, 0, 0b1]
    got, cur, cnt = pop_model(bm, 3, 2, 2, want=0b1, from_start=True)
    assert got[0] == 0 and cur == 1 and bm == [0, 0, 1]


def test_model_sweeps_a_long_ring_in_looks_of_64_words():
    bm = [0] * 160
    bm[150] = 0b100
    got, cur, cnt = pop_model(bm, 160, 10, 1, want=0b1)  # looks at 10..73, 74..137, 138..159 + 0..41
    assert got[0] == 150 * 32 + 2 and cur == 151 and cnt == 0


# ---- the header's bit helpers against the model's ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_pt_nth_bit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtt_pt_nth_bit.restype = None
    L.rtt_pt_low_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtt_pt_low_bits.restype = None
    return L


def helper_words():
    rng = np.random.default_rng(11)
    dense = rng.integers(0, 1 << 32, 5000, dtype=np.uint64)
    sparse = dense[:2500] & rng.integers(0, 1 << 32, 2500, dtype=np.uint64) & rng.integers(0, 1 << 32, 2500, dtype=np.uint64)
    full = dense[2500:] | rng.integers(0, 1 << 32, 2500, dtype=np.uint64) | rng.integers(0, 1 << 32, 2500, dtype=np.uint64)
    special = [0, 1, 0x80000000, 0xFFFFFFFF] + [1 << b for b in range(32)]
    return [int(x) for x in np.concatenate([dense, sparse, full])] + special


def test_bit_helpers_equal_the_model_on_every_n(hooks):
    """pt_nth_bit(v, n) for every n < popcount(v) and pt_low_bits(v, n) for every 1 <= n <= popcount(v): 10^4 random words (a third of
    them sparse, a third nearly full) and 0, 1, 0x80000000, 0xFFFFFFFF and the single-bit words."""
    words = helper_words()
    assert len(words) >= 10_000 + 4 + 32
    v_nth, n_nth, want_nth, v_low, n_low, want_low = [], [], [], [], [], []
    for v in words:
        bits = set_bits(v)
        for n in range(len(bits)):
            v_nth.append(v); n_nth.append(n); want_nth.append(nth_bit(v, n))
            v_low.append(v); n_low.append(n + 1); want_low.append(low_bits(v, n + 1))
    v_nth, n_nth = np.array(v_nth, np.uint32), np.array(n_nth, np.int32)
    out = np.full(len(v_nth), -1, np.int32)
    hooks.rtt_pt_nth_bit(v_nth.ctypes.data, n_nth.ctypes.data, out.ctypes.data, len(out))
    bad = out != np.array(want_nth, np.int32)
    assert not bad.any(), (v_nth[bad][:5], n_nth[bad][:5], out[bad][:5])
    v_low, n_low = np.array(v_low, np.uint32), np.array(n_low, np.int32)
    out = np.zeros(len(v_low), np.uint32)
    hooks.rtt_pt_low_bits(v_low.ctypes.data, n_low.ctypes.data, out.ctypes.data, len(out))
    bad = out != np.array(want_low, np.uint32)
    assert not bad.any(), (v_low[bad][:5], n_low[bad][:5], out[bad][:5])

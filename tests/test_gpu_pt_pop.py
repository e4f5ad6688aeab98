"""rt_pt_queue.h pt_pop on the device (the rtt_pt_pop hook: one workgroup, a bitmap in LDS, a fixed number of calls per wave) against the
model of test_pt_pop_model.py.  One wave: every call's 64 results, the cursor and the count after it, and the bitmap left behind equal the
model's exactly.  Four waves on one bitmap at once (claims come back short): every path is handed out exactly once."""
import ctypes as C
import os

import numpy as np
import pytest

from test_pt_pop_model import PT_NONE, pop_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ALL = (1 << 64) - 1
LOW16 = (1 << 16) - 1                 # the exact role's request: lanes < 16
HOLES = 0xF0F0_00FF_8000_0001 | (1 << 37)
FULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_pt_pop.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtt_pt_pop.restype = C.c_int
    return L


def device_pops(hooks, bitmap, cursor, wants, from_start, waves=1):
    """-> (got [waves, calls, 64], cursors [waves, calls], counts [waves, calls], bitmap after, count after)"""
    bm = np.array(bitmap, np.uint32)
    count = np.array([sum(bin(int(w)).count("1") for w in bitmap)], np.int32)
    want = np.array(wants, np.uint64)
    got = np.zeros((waves, len(wants), 64), np.uint32)
    cursors, counts = np.zeros((waves, len(wants)), np.uint32), np.zeros((waves, len(wants)), np.int32)
    rc = hooks.rtt_pt_pop(bm.ctypes.data, len(bm), count.ctypes.data, cursor, want.ctypes.data, len(wants), int(from_start), waves,
                          got.ctypes.data, cursors.ctypes.data, counts.ctypes.data)
    assert rc == 0
    return got, cursors, counts, bm, int(count[0])


def random_bitmap(rng, nw, density):
    return [int(sum(1 << b for b in range(32) if rng.random() < density)) for _ in range(nw)]


def one_wave_cases():
    rng = np.random.default_rng(5)
    cases = {}
    calls = [ALL, HOLES, LOW16, ALL, 1 << 63, ALL, HOLES, ALL]
    for nw in (1, 3, 40, 64, 65, 160):
        for cursor in sorted({0, nw - 1, nw // 2}):            # nw - 1: the first look wraps
            cases[f"nw{nw}-cursor{cursor}-mixed"] = (random_bitmap(rng, nw, 0.35), cursor, calls)
        cases[f"nw{nw}-sparse"] = (random_bitmap(rng, nw, 0.02), nw - 1, calls)
    # full words: a lane's rank in its word reaches 31, the words' counts need the sixth bit; 64 wanted = exactly two words
    cases["full-words"] = ([FULL] * 40, 39, [ALL, ALL, LOW16, HOLES, ALL, LOW16, LOW16, ALL])
    cases["full-words-ring-of-3"] = ([FULL] * 3, 1, [ALL, LOW16, ALL])
    twelve = [0] * 40
    for k in range(12):
        twelve[(3 * k + 2) % 40] = 1 << ((7 * k) % 32)
    cases["one-bit-in-each-of-12-words-all-want"] = (twelve, 30, [ALL, ALL])             # 12 paths, 52 lanes get none, the ring swept once
    cases["one-bit-in-each-of-12-words-16-want"] = (twelve, 0, [LOW16, LOW16])
    cases["one-bit-in-each-of-12-words-holes"] = (twelve, 17, [0x8000_0000_0000_0101, ALL])
    cases["cut-mid-word"] = ([0xFFFF00FF, 0x0000F000, 0x80000001], 0, [0x1F, 0x700, ALL, ALL])   # 5 of 24 bits, then 3 more of the same word
    cases["cut-at-bit-31"] = ([0x80000001, FULL], 0, [0b1, 0b1, LOW16, LOW16, ALL])
    cases["empty"] = ([0] * 65, 7, [ALL, LOW16])
    cases["nobody-wants"] = ([FULL] * 3, 2, [0, ALL])
    cases["long-ring-last-look-finds-it"] = ([0] * 150 + [0b100] + [0] * 9, 10, [0b1, ALL])
    return cases


CASES = one_wave_cases()


@pytest.mark.parametrize("from_start", [False, True], ids=["rotating", "from-start"])
@pytest.mark.parametrize("name", list(CASES))
def test_one_wave_equals_the_model(hooks, name, from_start):
    bitmap, cursor, wants = CASES[name]
    got, cursors, counts, bm_after, count_after = device_pops(hooks, bitmap, cursor, wants, from_start)
    model_bm, cur, cnt = list(bitmap), cursor, sum(bin(w).count("1") for w in bitmap)
    for c, want in enumerate(wants):
        want_got, cur, cnt = pop_model(model_bm, len(bitmap), cur, cnt, want, from_start)
        assert got[0, c].tolist() == want_got, (name, c, hex(want))
        assert int(cursors[0, c]) == cur and int(counts[0, c]) == cnt, (name, c, int(cursors[0, c]), cur, int(counts[0, c]), cnt)
    assert bm_after.tolist() == model_bm and count_after == cnt


@pytest.mark.parametrize("from_start", [False, True], ids=["rotating", "from-start"])
@pytest.mark.parametrize("density", [0.3, 0.9], ids=["sparse", "dense"])
def test_four_waves_hand_out_every_path_exactly_once(hooks, density, from_start):
    """Four waves pop the same 160-word bitmap at once, each asking for 64 paths per call, often enough for any one of them to empty it
    alone (a call that comes back short has swept the whole ring, and nothing is pushed): the union of what they got is the initial bit
    set, no path twice, the bitmap empty and the count 0."""
    rng = np.random.default_rng(23)
    bitmap = random_bitmap(rng, 160, density)
    bitmap[5] = bitmap[6] = bitmap[100] = FULL
    paths = sorted(w * 32 + b for w, v in enumerate(bitmap) for b in range(32) if (v >> b) & 1)
    n_calls = len(paths) // 64 + 2
    got, _, _, bm_after, count_after = device_pops(hooks, bitmap, 3, [ALL] * n_calls, from_start, waves=4)
    handed = got[got != PT_NONE]
    print(f"{len(paths)} paths, {n_calls} calls per wave; paths per wave: {[(got[w] != PT_NONE).sum() for w in range(4)]}")
    assert sorted(handed.tolist()) == paths
    assert not bm_after.any() and count_after == 0

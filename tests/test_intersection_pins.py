"""Pins the CPU oracle's box test and triangle test (oracle_bvh.h aabb_ray, oracle_hw8.cpp tri_ray) and the numpy restatement of the
box test (intersection_model.ref_box) to the compiled reference at the branch points of that code.  The cases are
tests/intersection_cases.py; the reference's answers are tests/golden/pins_intersection_edges.npz (golden/make_goldens.py).  The bar
is equal bits, or NaN on both sides.  The same cases then hold the device functions to the same file (test_gpu_intersection.py), and
the restatement carries the soundness tests of the exactness gate there.  Here also: that a gate with margins 64 times smaller would
fail those soundness tests on their own cases (the tests are not vacuous)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import intersection_cases as ic
import intersection_model as im
import oracle_lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_intersection_edges.npz")
F = np.float32
GATE_ROWS = 400000


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def differing(got, want):
    """Indices of the rows on which two answers (flags, then float bits) differ: other than equal words, or NaN in the same float on
    both sides."""
    got, want = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(want, np.uint32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = got == want
    same[:, 1:] |= np.isnan(got[:, 1:].view(F)) & np.isnan(want[:, 1:].view(F))
    return np.flatnonzero(~same.all(axis=1))


def model_box_answers():
    r = ic.rows("box")
    ok, inside, t = im.ref_box(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12])
    return np.stack([ok.astype(np.uint32) | (inside.astype(np.uint32) << 1), ic.bits(t)], axis=1)


@functools.lru_cache(maxsize=None)
def gate_cases(scale_index):
    """One scale's soundness cases, shared by the host test below and the GPU tests: the rows, and the reference's answers (through the
    model) on each row's own box and three boxes above it."""
    M = ic.SCALES[scale_index]
    rows = ic.gate_rows(M, GATE_ROWS, 8400 + scale_index)
    rows.setflags(write=False)
    return rows, im.BoxesAbove(rows, *ic.grown_boxes(rows, M, 8410 + scale_index))


def hit_bound(rows):
    """float32(t + gap): where the reference's best hit would stand if the runner-up at the gap came first."""
    with np.errstate(over="ignore"):
        return (rows[:, 12] + rows[:, 13]).astype(F)


@pytest.mark.parametrize("family", ic.FAMILIES)
def test_oracle_equals_reference_at_the_edges(gold, family):
    got, want = ic.oracle_answers()[family], gold[family]
    bad = differing(got, want)
    print(f"{family}: {len(want)} cases, {bad.size} differ from the reference")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_numpy_box_model_equals_reference(gold):
    got = model_box_answers()
    bad = differing(got, gold["box"])
    print(f"box model: {len(got)} cases, {bad.size} differ from the reference")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), gold["box"][bad[:5]].tolist())


def test_cases_reach_the_branches_they_claim(gold):
    """Counted over the reference's answers, so that a change of the table that loses an edge fails here and not silently."""
    r = ic.reach(gold)
    print(r)
    assert r["box_rows"] + r["tri_rows"] <= 20000
    assert r["box_nan_share"] <= 0.10 and r["tri_nan_share"] <= 0.10                      # numbers carry the comparison
    # box: each exit of `if (t1 > t2 || t2 < 0)` and of `if (t1 < 0)`, every kind of case, every scale
    assert r["box_accepted"] >= 2000 and r["box_rejected"] >= 2000 and r["box_inside"] >= 300 and r["box_outside"] >= 2000
    assert r["box_behind_rejected"] >= 300                                                 # t2 < 0
    assert r["box_graze_accepted"] >= 300                                                  # t1 == t2 is no rejection
    assert min(r["box_zero_t_entry"]) >= 50 and min(r["box_zero_t_exit"]) >= 50            # t1 == 0 and t2 == 0, +0 and -0 each
    assert min(r["box_nan_accepted_per_axis"]) >= 20                                       # 0/0 on each axis with the box accepted ...
    assert min(r["box_nan_rejected_per_axis"]) >= 20                                       # ... and rejected
    for name, (accepted, rejected) in r["box_kinds"].items():
        assert accepted + rejected >= 100, name
    assert all(n >= 3000 for n in r["box_scales"].values())
    # tri: every exit and both branches of the solve
    assert r["tri_hit"] >= 3000 and r["tri_miss"] >= 2000 and min(r["tri_facing"]) >= 1000
    assert r["tri_u_zero"] >= 100 and r["tri_v_zero"] >= 100                               # through a vertex, along an edge: no rejection at 0
    assert min(r["tri_uv_one"]) >= 20                                                      # u + v one ulp below 1, equal to 1, and beyond it
    assert min(r["tri_a2_zero"]) >= 50 and r["tri_a2_nonzero_hits"] >= 3000
    assert r["tri_den_zero_proper"] >= 50 and r["tri_normal_zero"] >= 100
    assert min(r["tri_dn"]) >= 300                                                         # dn > 0, dn < 0, dn == 0
    e = r["tri_t_exits"]
    assert e["nonpositive"] >= 100 and e["beyond"] >= 100 and e["nan"] >= 100 and min(e["near_zero"]) >= 100 and min(e["near_tmax"]) >= 100
    assert min(r["tri_near_singular"]) >= 200
    assert r["tri_nan_hits"] >= 10                                                         # a NaN in u or v passes all three comparisons: a hit
    for name, (hit, miss) in r["tri_kinds"].items():
        assert hit + miss >= 100, name
    assert all(n >= 3000 for n in r["tri_scales"].values())


def test_nan_acceptance_is_the_x_axis_alone(gold):
    """d_k == 0 with the origin exactly on the low face of axis k makes (-s - o) / d a 0/0.  std::min hands a NaN in its FIRST operand
    on, and so does std::max: on the x axis the NaN reaches t1 and t2, every comparison with it is false, and the reference accepts the
    box wherever the ray goes, with t = NaN.  On y and z the NaN is std::max's / std::min's SECOND operand and is dropped: the axis
    takes no part.  On the high face the NaN is the second operand of the per-axis min and max, and the axis's interval is the other
    quotient twice, an infinity: rejected."""
    b, g = ic.families()["box"], gold["box"]
    ok, t = (g[:, 0] & 1) != 0, g[:, 1].view(F)
    kb = ic.K["box"]
    low, high = b["kind"] == kb["zero_on_low_face"], b["kind"] == kb["zero_on_high_face"]
    assert ok[low & (b["axis"] == 0)].all() and np.isnan(t[low & (b["axis"] == 0)]).all()
    for k in (1, 2):
        rows = low & (b["axis"] == k)
        assert ok[rows].any() and (~ok[rows]).any() and not np.isnan(t[rows & ok]).any()
    assert not ok[high].any()


def test_golden_is_current_with_live_reference(gold):
    """Where the reference harnesses are built (and have the entry points), the file is what they answer today."""
    p8 = oracle_lib.ref_path("libref_hw8.so")
    if p8 is None or not hasattr(C.CDLL(p8), "ref8_box_test") or not hasattr(C.CDLL(p8), "ref8_tri_test"):
        print("oracle/_ref is not built from this tree's harnesses: pins_intersection_edges.npz not re-evaluated live")
        return
    live = ic.evaluate("reference")
    for family in ic.FAMILIES:
        assert np.array_equal(live[family], gold[family]), family


@pytest.mark.parametrize("scale_index", range(len(ic.SCALES)))
def test_a_gate_with_margins_64_times_smaller_fails_the_soundness_cases(scale_index):
    """The vacuity guard of test_gpu_intersection.py's soundness tests: on the same rows and boxes, the numpy model of the gate with c1
    and c2 scaled by 1/64 lets hits stand whose boxes the reference rejects (a) or would prune behind the runner-up (b).  With today's
    constants the model finds none; the device's own decisions are what the GPU test asserts on."""
    rows, above = gate_cases(scale_index)
    found = {1.0: [0, 0, 0], 1.0 / 64: [0, 0, 0]}
    for scale, f in found.items():
        for gap in ic.GAPS:
            r = ic.with_gap(rows, gap)
            stands = im.hit_stands(r, scale)
            f[0] += int(stands.sum()); f[1] += above.rejected(stands).size; f[2] += above.pruned(stands, hit_bound(r)).size
    print(f"M = {ic.SCALES[scale_index]}: standing, (a), (b) at today's constants {found[1.0]}, at 1/64 {found[1.0 / 64]}")
    assert found[1.0][1:] == [0, 0]
    assert found[1.0 / 64][1] >= 100 and found[1.0 / 64][2] >= 20

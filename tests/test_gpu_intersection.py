"""The device's intersection layer, one lane per case (csrc/test_hooks.hip rtt_ref_box_test .. rtt_slab_padded call the product's functions).

A. ref_box_test (rt_ref_walk.h) and tri_test / tri_test_closer (rt_device.h, on the host's own make_isect record) against the compiled
   reference's answers (tests/golden/pins_intersection_edges.npz) on the cases of intersection_cases.py, bit for bit or NaN on both sides.
B. Soundness.  The model is intersection_model.ref_box, which test_intersection_pins.py pins to the same file.
   B1  the exactness gate (rt_exact.h pt_hit_stands, pt_box_robust, rq_any_hit_stands): whenever it lets a hit stand, the reference's
       box test accepts the triangle's box and every box above it (a), and enters none of them from outside behind the runner-up (b).
   B2  the walkers' slab_test on boxes padded by the host's pad_box: it enters every box the reference's test enters, no later.
   With test_gpu_device_bvh's "grid box contains float box" test this closes the chain from the reference's test to the persistent
   walkers' 16-bit boxes."""
import ctypes as C
import os

import numpy as np
import pytest

import intersection_cases as ic
import intersection_model as im
from test_intersection_pins import GOLD, differing, gate_cases, hit_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SLAB_ROWS = 1000000


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    P = C.c_void_p
    for name in ("rtt_ref_box_test", "rtt_hit_stands", "rtt_box_robust", "rtt_any_hit_stands"):
        getattr(L, name).argtypes = [P, P, C.c_size_t]
    L.rtt_tri_test.argtypes = [P, P, P, C.c_size_t]
    L.rtt_slab_padded.argtypes = [P, C.c_float, C.c_float, P, P, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def decide(fn, rows16):
    rows16 = np.ascontiguousarray(rows16, F)
    out = np.zeros(len(rows16), np.uint32)
    assert fn(rows16.ctypes.data, out.ctypes.data, len(rows16)) == 0
    return out


def tri_test(hooks, keep_t):
    """tri_test and tri_test_closer (with keep_t per row) on the `tri` family: two n x 4 arrays of flags and the bits of t, u, v."""
    rows = ic.rows("tri")
    keep_t = np.ascontiguousarray(keep_t, F)
    out = np.zeros((len(rows), 8), np.uint32)
    assert hooks.rtt_tri_test(rows.ctypes.data, keep_t.ctypes.data, out.ctypes.data, len(rows)) == 0
    return out[:, :4], out[:, 4:]


def report(name, rows, bad, dev, want, against):
    print(f"{name}: {len(want)} cases, {bad.size} differ from {against}")
    for i in bad[:8]:
        print(f"  case {i}: in {[float(x).hex() for x in rows[i]]}\n    device {[hex(int(x)) for x in dev[i]]} {against} {[hex(int(x)) for x in want[i]]}")
    return bad.size


def test_ref_box_test_equals_reference(hooks, gold):
    """ref_box_test, the box test of every exact walk: both exits of each branch, t1 == 0 and t2 == 0 of either sign, t1 == t2, flat
    boxes, direction components of +-0, denormals and 1e30, and 0/0 on each axis (which axis's NaN swallows the others)."""
    rows = ic.rows("box")
    dev = np.zeros((len(rows), 2), np.uint32)
    assert hooks.rtt_ref_box_test(rows.ctypes.data, dev.ctypes.data, len(rows)) == 0
    assert report("box", rows, differing(dev, gold["box"]), dev, gold["box"], "the reference") == 0


def test_tri_test_equals_reference(hooks, gold):
    """tri_test on the record the host's make_isect forms.  u and v are compared as the reference shows them, through the texcoords of a
    figure with corners (1,0), (0,1), (0,0): ic.as_texcoords applies those two sums to the device's u and v (-0 becomes +0, a NaN in one
    reaches the other; every other value is unchanged)."""
    rows = ic.rows("tri")
    dev, _ = tri_test(hooks, np.full(len(rows), np.inf))
    tu, tv = ic.as_texcoords(dev[:, 2].view(F), dev[:, 3].view(F))
    hit = (dev[:, 0] & 1) != 0
    shown = np.stack([dev[:, 0], dev[:, 1], np.where(hit, ic.bits(tu), 0), np.where(hit, ic.bits(tv), 0)], axis=1)
    n_bad = report("tri", rows, differing(shown, gold["tri"]), shown, gold["tri"], "the reference")
    n_bad += report("tri", rows, differing(shown, ic.oracle_answers()["tri"]), shown, ic.oracle_answers()["tri"], "the oracle")
    ordinary = hit & ~np.isnan(tu) & ~np.isnan(tv) & (dev[:, 2] != 0x80000000) & (dev[:, 3] != 0x80000000)
    print(f"tri: on {int(ordinary.sum())} ordinary hits the texcoords are u and v themselves")
    assert np.array_equal(shown[ordinary, 2:], dev[ordinary, 2:]) and ordinary.sum() >= 3000
    assert n_bad == 0


def test_tri_test_closer_is_tri_test_up_to_keep_t(hooks):
    """tri_test_closer answers as tri_test for keep_t of t, t + 1 ulp and +inf (and, on rows that miss, for any keep_t), and rejects for
    keep_t of t - 1 ulp on rows that hit."""
    rows = ic.rows("tri")
    plain, closer = tri_test(hooks, np.full(len(rows), np.inf))
    hit = (plain[:, 0] & 1) != 0
    t = plain[:, 1].view(F)
    assert np.array_equal(closer, plain)
    print(f"tri_test_closer: {int(hit.sum())} hits, {int((~hit).sum())} misses")
    for name, keep in (("t", t), ("t + 1 ulp", np.where(hit, ic.ulp_step(np.where(hit, t, F(1)), 1), t))):
        keep = np.where(hit, keep, F([1e-3, 1.0, 1e30])[np.arange(len(rows)) % 3])       # a miss stays one
        again, closer = tri_test(hooks, keep)
        bad = np.flatnonzero((closer != plain).any(axis=1))
        print(f"  keep_t = {name}: {bad.size} differ from tri_test")
        assert np.array_equal(again, plain) and bad.size == 0, (name, bad[:5].tolist())
    below = np.where(hit, ic.ulp_step(np.where(hit, t, F(1)), -1), F(0))
    _, closer = tri_test(hooks, below)
    still = np.flatnonzero(hit & ((closer[:, 0] & 1) != 0))
    print(f"  keep_t = t - 1 ulp: {still.size} of {int(hit.sum())} hits are still reported")
    assert still.size == 0 and not closer[~hit].any()


@pytest.mark.parametrize("scale_index", range(len(ic.SCALES)))
def test_gate_is_sound_against_the_reference_box_test(hooks, scale_index):
    """B1.  Per scale 400,000 rows (a box, a ray, a hit at t on or near a face or inside) and, for each, the runner-up nowhere and at
    t 2^-4, 2^-10, 2^-16, 2^-20 behind the hit.  For every standing decision of pt_hit_stands, on the triangle's own box and three
    grown copies: (a) the model accepts the box; (b) the model reports `inside`, or not float32(t + gap) < t_box, the reference's
    pruning condition curBest < t_box for a runner-up at the gap.  pt_box_robust (with and without its pretest): (a).
    rq_any_hit_stands with tmax = t + gap: (a), and the model reports `inside` or t_box < tmax.  Zero violations is the bar.
    Vacuity: the device lets at least half as many hits stand as the numpy model of the gate (the same formulas with an IEEE
    reciprocal); that a gate with smaller margins fails on these rows is test_intersection_pins's."""
    M = ic.SCALES[scale_index]
    rows, above = gate_cases(scale_index)
    n_dev = n_model = n_any = 0
    bad = {"hit_stands (a)": 0, "hit_stands (b)": 0, "any_hit_stands (a)": 0, "any_hit_stands (b)": 0}
    for gap in ic.GAPS:
        r = ic.with_gap(rows, gap)
        bound = hit_bound(r)
        stands = decide(hooks.rtt_hit_stands, r) != 0
        model = im.hit_stands(r)
        n_dev += int(stands.sum()); n_model += int(model.sum())
        a, b = above.rejected(stands), above.pruned(stands, bound)
        bad["hit_stands (a)"] += a.size; bad["hit_stands (b)"] += b.size
        r_any = r.copy()
        r_any[:, 13] = bound                                             # tmax in the gap's place
        any_stands = decide(hooks.rtt_any_hit_stands, r_any) != 0
        n_any += int(any_stands.sum())
        aa, ab = above.rejected(any_stands), above.pruned(any_stands, bound, strict=False)
        bad["any_hit_stands (a)"] += aa.size; bad["any_hit_stands (b)"] += ab.size
        print(f"M = {M}, gap {gap}: standing device {int(stands.sum())} model {int(model.sum())} (they differ on {int((stands != model).sum())}), "
              f"any-hit {int(any_stands.sum())}; violations (a) {a.size} (b) {b.size}, any-hit (a) {aa.size} (b) {ab.size}")
        for name, idx in (("(a)", a), ("(b)", b), ("any (a)", aa), ("any (b)", ab)):
            for i in idx[:4]:
                print(f"  {name} row {i}: {[float(x).hex() for x in r[i]]} t_box {above.t_box[:, i].tolist()} ok {above.ok[:, i].tolist()} inside {above.inside[:, i].tolist()}")
    robust = decide(hooks.rtt_box_robust, rows)
    for bit, name in ((1, "box_robust<true> (a)"), (2, "box_robust<false> (a)")):
        idx = above.rejected((robust & bit) != 0)
        bad[name] = idx.size
        print(f"M = {M}: {name[:-4]} holds on {int(((robust & bit) != 0).sum())} of {len(rows)} rows, violations {idx.size}")
        for i in idx[:4]:
            print(f"  row {i}: {[float(x).hex() for x in rows[i]]}")
    print(f"M = {M}: standing decisions device {n_dev}, model {n_model}, any-hit {n_any}; violations {bad}")
    assert n_model >= 100000 and 2 * n_dev >= n_model and 2 * n_any >= n_model
    assert ((robust & 1) != 0).sum() >= ((robust & 2) != 0).sum() >= 50000    # the pretest only adds
    assert all(v == 0 for v in bad.values()), bad


@pytest.mark.parametrize("scale_index", range(len(ic.SCALES)))
def test_padded_slab_test_enters_what_the_reference_enters(hooks, scale_index):
    """B2.  slab_test at tbest = RT_T_MAX on the box as the host pads it (pad_box with scene_abs_pad(M)), 1,000,000 rows of the `box`
    family's generator per scale: where the model accepts, slab_test accepts; where the model accepts from outside, tnear <= t_box;
    where it reports `inside`, tnear <= 0.
    Every direction component is at least 1e-30 in magnitude.  Rows with a zero component are left out because of what the pins show
    (test_nan_acceptance_is_the_x_axis_alone): with d_x == 0 and the origin exactly on the box's low x face the reference forms 0/0,
    the NaN swallows the other axes and the reference accepts a box the ray plainly misses; no conservative test can follow it there.
    Such rays take the exact walk in queries (rq_classify: dmin >= 1e-30f); what the render pipelines do with them is in DESIGN.md 3."""
    M = ic.SCALES[scale_index]
    rows, _ = ic.box_rows(M, SLAB_ROWS, 8500 + scale_index)
    assert (np.abs(rows[:, 9:12]) >= F(1e-30)).all()
    ok, inside, t_box = im.ref_box(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])
    flag, tnear, unbounded, tnear_u = (np.zeros(len(rows), dt) for dt in (np.uint32, F, np.uint32, F))
    assert hooks.rtt_slab_padded(rows.ctypes.data, F(M), -1.0, flag.ctypes.data, tnear.ctypes.data, len(rows)) == 0
    assert hooks.rtt_slab_padded(rows.ctypes.data, F(M), np.inf, unbounded.ctypes.data, tnear_u.ctypes.data, len(rows)) == 0
    assert np.array_equal(tnear, tnear_u)
    # The walkers call slab_test with tbest <= RT_T_MAX, and tbest is a clause of the test: a box that the ray enters beyond RT_T_MAX is
    # declined on purpose (no triangle test accepts a t >= RT_T_MAX).  Rays of length 0.07 meet such boxes at M = 1000.  So the first
    # assertion is made twice: with no bound on every row, and at tbest = RT_T_MAX on the rows the reference enters within RT_T_MAX.
    beyond = ok & ~inside & ~(t_box <= ic.T_MAX)
    entered, entered_u = flag != 0, unbounded != 0
    missed = np.flatnonzero((ok & ~entered_u) | (ok & ~beyond & ~entered))
    late = np.flatnonzero(ok & entered_u & ~inside & ~(tnear <= t_box))
    late_inside = np.flatnonzero(ok & entered_u & inside & ~(tnear <= 0))
    print(f"M = {M}: {len(rows)} rows, the reference accepts {int(ok.sum())} ({int(inside.sum())} from inside, {int(beyond.sum())} entered beyond RT_T_MAX), "
          f"slab_test {int(entered.sum())}, without a bound {int(entered_u.sum())}; accepted by the reference only {missed.size}, "
          f"entered later than the reference {late.size}, inside with tnear > 0 {late_inside.size}")
    for i in np.concatenate([missed[:4], late[:4], late_inside[:4]]):
        print(f"  row {i}: {[float(x).hex() for x in rows[i]]} t_box {float(t_box[i]).hex()} inside {bool(inside[i])} slab_test {bool(entered[i])} tnear {float(tnear[i]).hex()}")
    assert ok.sum() >= 0.2 * len(rows) and inside.sum() >= 0.02 * len(rows) and (~ok).sum() >= 0.2 * len(rows)
    assert missed.size == 0 and late.size == 0 and late_inside.size == 0

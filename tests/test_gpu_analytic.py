"""The device's analytic figures, light pdf and samplers of the .txt snapshots, one lane per case (csrc/test_hooks.hip rtt_quad .. rtt_cosine_txt
call the product's functions on records the host's own pack_prim / pack_fig5 form): smallest_root in both root forms, box_slabs, prim_hit1,
prim_hit in its three instantiations, fig_hit5, light_pdf4, light_pdf_one5, pdf_one4 and pdf_one5 on points of their own, light_sample4 and
light_sample5 (box_face_point, rng_n01_slot, the triangle's fold and the rejection loop beneath them) and cosine_sample_txt, against the
compiled reference's answers (tests/golden/pins_analytic_edges.npz) and the oracle's on the cases of analytic_cases.py: bit for bit, or NaN
on both sides; engine states and normal caches equal.  box_face_point on its own is held to the oracle: the reference keeps that point
in a local of its loop (analytic_cases.face_point_cases)."""
import ctypes as C
import os

import numpy as np
import pytest

import analytic_cases as ac
from test_analytic_pins import GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
HW5_LONG_DOUBLE_ROWS = ()      # lpdf rows on which hw5's 80-bit t + eps and the device's double sum narrow to different floats: none on this table


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    P = C.c_void_p
    for name in ("rtt_quad", "rtt_slabs", "rtt_fig", "rtt_lpdf", "rtt_pdf_one"):
        getattr(L, name).argtypes = [P, P, C.c_size_t]
    for name in ("rtt_lsample", "rtt_cosine_txt", "rtt_face_point"):
        getattr(L, name).argtypes = [P, P, P, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def run(fn, rows, width, aux=None):
    rows = np.ascontiguousarray(rows, F)
    out = np.zeros((len(rows), width), U)
    rc = fn(rows.ctypes.data, out.ctypes.data, len(rows)) if aux is None else fn(rows.ctypes.data, np.ascontiguousarray(aux, U).ctypes.data, out.ctypes.data, len(rows))
    assert rc == 0, rc
    return out


def report(name, rows, dev, want, against, only=None):
    idx = np.arange(len(rows)) if only is None else only
    bad = idx[ac.differing(dev[idx], want[idx])]
    print(f"{name}: {len(idx)} cases, {bad.size} differ from {against}")
    for i in bad[:8]:
        print(f"  case {i}: in {[float(x).hex() for x in rows[i]]}\n    device {[hex(int(x)) for x in dev[i]]} {against} {[hex(int(x)) for x in want[i]]}")
    return bad.size


def both(name, rows, dev, gold_cols, oracle_cols, only=None):
    return report(name, rows, dev, gold_cols, "the reference", only) + report(name, rows, dev, oracle_cols, "the oracle", only)


def test_smallest_root_equals_reference_in_both_forms(hooks, gold):
    rows = ac.rows("quad")
    dev = run(hooks.rtt_quad, rows, 4)
    assert both("quad", rows, dev, gold["quad"], ac.oracle_answers()["quad"]) == 0


def test_box_slabs_equals_reference(hooks, gold):
    rows = ac.rows("slabs")
    dev = run(hooks.rtt_slabs, rows, 2)
    assert both("slabs", rows, dev, gold["slabs"], ac.oracle_answers()["slabs"]) == 0


def test_figure_tests_equal_reference(hooks, gold):
    """prim_hit1, prim_hit<true>, prim_hit<false>, prim_hit<false, true> and fig_hit5 on the ellipsoids, planes and boxes; fig_hit5 on the triangles."""
    rows = ac.rows("fig")
    dev = run(hooks.rtt_fig, rows, 25)
    n_bad = 0
    for k, name in enumerate(("hw1 prim_hit1", "hw2 prim_hit<true>", "hw3 prim_hit<false>", "hw4 prim_hit<false, true>", "hw5 fig_hit5")):
        c = slice(5 * k, 5 * k + 5)
        n_bad += both(name, rows, dev[:, c], gold["fig"][:, c], ac.oracle_answers()["fig"][:, c])
    rows = ac.rows("tri5")
    dev = run(hooks.rtt_fig, rows, 25)[:, 20:25]
    n_bad += both("hw5 fig_hit5 on triangles", rows, dev, gold["tri5"], ac.oracle_answers()["tri5"])
    assert n_bad == 0


def test_light_pdfs_equal_reference(hooks, gold):
    """light_pdf4 and light_pdf_one5.  hw5 forms t + eps in 80 bits, the device in double: rows on which the two narrow differently would be
    listed in HW5_LONG_DOUBLE_ROWS (at most 1 in 10,000 rows) and left out of the hw5 comparison; the list is empty."""
    rows = ac.rows("lpdf")
    dev = run(hooks.rtt_lpdf, rows, 2)
    g, o = gold["lpdf"], ac.oracle_answers()["lpdf"]
    print("rows excluded for hw5's 80-bit sum:", list(HW5_LONG_DOUBLE_ROWS))
    assert len(HW5_LONG_DOUBLE_ROWS) * 10000 <= len(rows)
    keep = np.setdiff1d(np.arange(len(rows)), np.asarray(HW5_LONG_DOUBLE_ROWS, int))
    n_bad = both("hw4 light_pdf4", rows, dev[:, 0:1], g[:, 0:1], o[:, 0:1], np.flatnonzero(rows[:, 0] != ac.TRIANGLE))
    n_bad += both("hw5 light_pdf_one5", rows, dev[:, 1:2], g[:, 1:2], o[:, 1:2], keep)
    assert n_bad == 0


def test_pdf_one_equals_reference(hooks, gold):
    """pdf_one4 and pdf_one5 on a y and yn that no hit produced: y == x, y at the ellipsoid's centre, d . yn == +-0, figures without an area,
    NaN and inf in every argument."""
    rows = ac.rows("pone")
    dev = run(hooks.rtt_pdf_one, rows, 2)
    g, o = gold["pone"], ac.oracle_answers()["pone"]
    n_bad = both("hw4 pdf_one4", rows, dev[:, 0:1], g[:, 0:1], o[:, 0:1], np.flatnonzero(rows[:, 0] != ac.TRIANGLE))
    n_bad += both("hw5 pdf_one5", rows, dev[:, 1:2], g[:, 1:2], o[:, 1:2])
    assert n_bad == 0


def test_box_face_point_equals_oracle(hooks):
    """box_face_point against the oracle's lines for it (the reference keeps the point in a local of its loop; test_analytic_pins.py holds
    the oracle's to the reference's draw order): the point in the box's frame and the engine state."""
    s, seeds, _ = ac.face_point_cases()
    dev = run(hooks.rtt_face_point, s, 4, seeds)
    assert report("box_face_point", s, dev, ac.face_point_oracle(), "the oracle") == 0


def device_aux(aux, before):
    """seed, whether the normal cache holds a value, its bits: the cache as the reference reports it before the call."""
    return np.ascontiguousarray(np.stack([aux[:, 0], before[:, 0], before[:, 1]], axis=1), U)


def test_light_samplers_equal_reference(hooks, gold):
    """light_sample4 as light i % 32 of a pixel (its own cache of normals, every other cache holding a sentinel that must survive) and
    light_sample5 with the pixel's one cache: direction, engine state and the cache afterwards."""
    rows, aux = ac.rows("lsample"), ac.aux("lsample")
    g, o = gold["lsample"], ac.oracle_answers()["lsample"]
    assert np.array_equal(g[:, 14:16], o[:, 14:16])                      # the cache the rows start from, as the oracle primes it
    dev = run(hooks.rtt_lsample, rows, 13, device_aux(aux, g[:, 14:16]))
    not_tri = np.flatnonzero(rows[:, 0] != ac.TRIANGLE)
    n_bad = both("hw4 light_sample4", rows, dev[:, 0:6], g[:, 0:6], o[:, 0:6], not_tri)
    n_bad += both("hw5 light_sample5", rows, dev[:, 7:13], g[:, 8:14], o[:, 8:14])
    disturbed = not_tri[dev[not_tri, 6] != 1]
    print(f"hw4: {disturbed.size} rows disturbed another object's normal cache")
    assert n_bad == 0 and disturbed.size == 0


def test_cosine_sample_equals_reference(hooks, gold):
    rows, aux = ac.rows("cosine"), ac.aux("cosine")
    g, o = gold["cosine"], ac.oracle_answers()["cosine"]
    dev = run(hooks.rtt_cosine_txt, rows, 6, device_aux(aux, g[:, 14:16]))
    n_bad = both("hw4 Cosine", rows, dev, g[:, 0:6], o[:, 0:6]) + both("hw5 Cosine", rows, dev, g[:, 8:14], o[:, 8:14])
    assert n_bad == 0

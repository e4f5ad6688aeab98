"""The persistent kernel's walkers read nodes, triangles and lights at 32-bit offsets from a scalar base, and the light walker reads its
lights as a pair of arrays, the 48-byte test records packed and the 96-byte remainders (rt_types.h LightRest).  Nothing a walk decides
may move: on a scene whose light tree is built on the device (64 lights or more) and on one below that (the reference's topology), the
persistent pipeline's pixels equal the oracle's and the round pipeline's with its exact kernels, bit for bit, floats and bytes, with the
same query counts; and record k of the pair of arrays is the light record that the walker's leaf order puts at k, field for field."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 32, 24, 4
# n triangles, emissive materials of six: about 200 lights (device-built light tree) and about 33 (the host's)
CASES = {"device_light_tree": dict(n=600, seed=3, n_emissive_mats=2), "host_light_tree": dict(n=200, seed=3, n_emissive_mats=1)}
LIGHT_REC = np.dtype([("isect", np.uint32, 12), ("rest", np.uint32, 24)])  # compared as bits: a NaN stays equal to itself


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_light_walk_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.rtt_light_walk_arrays.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def scene_data():
    return {name: pin_cases.random_triangle_scene(**kw) for name, kw in CASES.items()}


@pytest.fixture(scope="module")
def oracle_frames(scene_data):
    return {name: oracle_lib.Hw8Oracle(sd).render(W, H, SPP)[:2] for name, sd in scene_data.items()}


def _n_lights(rt, sd):
    scene = rt.Scene(sd)
    try:
        return scene.info().n_lights
    finally:
        scene.close()


def test_the_cases_lie_on_both_sides_of_the_threshold(rt, scene_data):
    assert _n_lights(rt, scene_data["device_light_tree"]) >= 64
    assert 0 < _n_lights(rt, scene_data["host_light_tree"]) < 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_pixels_and_counts_equal_the_round_pipeline_and_the_oracle(rt, monkeypatch, scene_data, oracle_frames, name):
    sd = scene_data[name]
    scene = rt.Scene(sd)
    try:
        rgb, rgb8, st = scene.render(W, H, SPP)
    finally:
        scene.close()
    monkeypatch.setenv("RTAMD_KERNEL", "wavefront")
    monkeypatch.setenv("RTAMD_ROUNDS_EXACT", "1")
    scene = rt.Scene(sd)
    try:
        rgb_r, rgb8_r, st_r = scene.render(W, H, SPP, counters=True)  # the round pipeline counts its queries only when asked to
    finally:
        scene.close()
    ref, ref8 = oracle_frames[name]
    print(f"{name}: persistent {st.closest_hit_queries}+{st.light_pdf_queries} queries, exact {st.exact_closest_hits}+{st.exact_light_sums}; "
          f"rounds {st_r.closest_hit_queries}+{st_r.light_pdf_queries}, exact {st_r.exact_closest_hits}+{st_r.exact_light_sums}; "
          f"floats equal: rounds {np.array_equal(rgb, rgb_r)}, oracle {np.array_equal(rgb, ref)}; byte mismatches {int((rgb8 != rgb8_r).sum())}, {int((rgb8 != ref8).sum())}")
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st_r.pipeline == rt.RT_PIPELINE_ROUNDS
    assert st.reference_exact == 1 and st_r.reference_exact == 1
    assert np.array_equal(rgb, rgb_r) and np.array_equal(rgb8, rgb8_r)
    assert np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    assert st.light_pdf_queries == st_r.light_pdf_queries and st.light_pdf_queries > 0
    assert st.exact_light_sums == st_r.exact_light_sums


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_pair_of_arrays_holds_the_leaf_ordered_records(rt, hooks, scene_data, name):
    """Record k of the walker's leaf order is the light `pad >> 1` of the reference's order with its pad word rewritten (index << 1 |
    last of its leaf): the test array must hold its first 48 bytes but for that word, the remainder array its other 96, and every light
    must appear once."""
    scene = rt.Scene(scene_data[name])
    try:
        n = scene.info().n_lights
        test = np.zeros((n, 12), np.uint32)
        rest = np.zeros((n, 24), np.uint32)
        lights = np.zeros(n, LIGHT_REC)
        got = hooks.rtt_light_walk_arrays(scene._h, test.ctypes.data, rest.ctypes.data, lights.ctypes.data, n)
    finally:
        scene.close()
    assert got == n
    index = test[:, 11] >> 1
    assert np.array_equal(np.sort(index), np.arange(n, dtype=np.uint32))
    assert np.array_equal(test[:, :11], lights["isect"][index][:, :11])
    assert np.array_equal(rest, lights["rest"][index])
    assert test[-1, 11] & 1 == 1  # the last record ends its leaf
    if name == "host_light_tree":  # the reference's topology: the leaf order is the light order, the leaf marks are the reference's
        assert np.array_equal(index, np.arange(n, dtype=np.uint32))
        assert np.array_equal(test[:, 11] & 1, (lights["isect"][:, 11] != 0).astype(np.uint32))

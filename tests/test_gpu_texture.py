"""The device's texture layer (rt_device.h: sample_texture in both its forms, load_texel, apply_normal_map) and the hw8 render pipelines
against the compiled reference's own hw8 scene.cpp, through the golden files of test_texture_pins.py; nothing here reads the reference.

  taps          csrc/test_hooks.hip rtt_sample_texture, one lane per case of tests/texture_cases.py, over a scene made through the public API
                from the table's images: scene preparation's texel packing, offsets, spare bytes and sRGB table are under test with the taps
  normal maps   rtt_apply_normal_map on the table's rows
  first hits    rt_query_surface on the scene texture_edges against surface_model.py bound to the reference's taps
  renders       every frame of pins_hw8_paths.npz on the persistent, round and mega pipelines

The bar for taps, normal maps and surfaces is equal bits, or NaN on both sides."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import surface_cases
import surface_model as sm
import test_gpu_query as tq
import texture_cases as tc
from test_gpu_scenes import _parity, _report
from test_shading_pins import differing
from test_texture_pins import FRAME, GOLD, GOLD_PATHS, PATH_CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TAP_FAMILIES = ("texel", "tap", "past_end")


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    P = C.c_void_p
    L.rtt_sample_texture.argtypes = [P, C.c_int, P, P, P, P, C.c_size_t]
    L.rtt_apply_normal_map.argtypes = [P, P, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gold_paths():
    return dict(np.load(GOLD_PATHS))


@pytest.fixture(scope="module")
def tap_scene(rt):
    scene = rt.Scene(tc.scene_data())
    yield scene
    scene.close()


def device_taps(hooks, scene, names, form):
    """One launch over the rows of the named families, one after the other: {name: n x 3}."""
    fams = [tc.families()[n] for n in names]
    slot, uv, srgb = (np.ascontiguousarray(np.concatenate([f[k] for f in fams])) for k in ("slot", "uv", "srgb"))
    out = np.zeros((len(slot), 3), F)
    t0 = time.perf_counter()
    rc = hooks.rtt_sample_texture(scene._h, form, slot.ctypes.data, uv.ctypes.data, srgb.ctypes.data, out.ctypes.data, len(slot))
    print(f"rtt_sample_texture form {form}: {len(slot)} lanes, {1e3 * (time.perf_counter() - t0):.2f} ms")
    assert rc == 0, rc
    return dict(zip(names, np.split(out, np.cumsum([len(f["slot"]) for f in fams])[:-1])))


def check(name, dev, want, against):
    bad = differing(dev, want)
    print(f"{name}: {len(want)} cases, {bad.size} differ from {against}")
    fam = tc.families()[name]
    for i in bad[:8]:
        row = {k: v[i].tolist() for k, v in fam.items()}
        print(f"  case {i}: {row}\n    device {[float(x).hex() for x in dev[i]]} {against} {[float(x).hex() for x in want[i]]}")
    return bad.size


@pytest.mark.parametrize("form", [0, 1])
def test_taps_equal_reference_and_oracle(hooks, gold, tap_scene, form):
    """Every byte value under both curves; every image from 1x1 to 1000x3 and the environment map with uv on and one float beside every
    texel boundary, shifted by whole numbers, at +-0, +-denormal, +-1e-8, +-1, +-(1e6 + 0.5), 8388607.5, 2^24 and 1e30; and the taps whose
    product rounds up to the size, where load_texel answers 0 for the texel past the end, as the reference reads it from zeroed bytes."""
    dev = device_taps(hooks, tap_scene, TAP_FAMILIES, form)
    o = tc.oracle_answers()
    n_bad = sum(check(name, dev[name], gold[name], "the reference") + check(name, dev[name], o[name], "the oracle") for name in TAP_FAMILIES)
    assert n_bad == 0


@pytest.mark.parametrize("form", [0, 1])
def test_nonfinite_coordinates_give_nan_and_no_error(hooks, tap_scene, form):
    """NaN and infinite texcoords (a hit with den == 0 has NaN u and v): (int)NaN is 0 on the device, so the tap reads texel (0, 0) with NaN
    weights.  The device and the oracle both answer NaN in every channel, and the call returns with no HIP error."""
    dev = device_taps(hooks, tap_scene, ("nonfinite",), form)["nonfinite"]
    assert np.isnan(dev).all() and np.isnan(tc.oracle_answers()["nonfinite"]).all()
    again = device_taps(hooks, tap_scene, ("texel",), form)["texel"]          # and the device goes on answering
    assert differing(again, tc.oracle_answers()["texel"]).size == 0


def test_hook_refuses_slots_outside_the_scene(hooks, tap_scene):
    slot, uv, srgb, out = np.array([len(tc.images())], np.int32), np.zeros((1, 2), F), np.zeros(1, np.int32), np.zeros((1, 3), F)
    for s in (len(tc.images()), -2, 1 << 20):
        slot[0] = s
        assert hooks.rtt_sample_texture(tap_scene._h, 0, slot.ctypes.data, uv.ctypes.data, srgb.ctypes.data, out.ctypes.data, 1) == -1


def test_normal_maps_equal_reference_and_oracle(hooks, gold):
    """apply_normal_map with sn and the tangent unit, non-unit, zero, parallel and antiparallel, tanw +-1, +-0 and 2, samples on the k / 255
    lattice and between, and (0.5, 0.5, 0.5), whose local normal is 0: NaN on every side."""
    rows = tc.families()["normal_map"]["rows"]
    dev = np.zeros((len(rows), 3), F)
    assert hooks.rtt_apply_normal_map(rows.ctypes.data, dev.ctypes.data, len(rows)) == 0
    n_bad = 0
    for want, against in ((gold["normal_map"], "the reference"), (tc.oracle_answers()["normal_map"], "the oracle")):
        bad = differing(dev, want)
        print(f"normal_map: {len(rows)} cases, {bad.size} differ from {against}")
        for i in bad[:8]:
            print(f"  case {i}: in {[float(x).hex() for x in rows[i]]}\n    device {dev[i].tolist()} {against} {want[i].tolist()}")
        n_bad += bad.size
    assert n_bad == 0


def test_surfaces_of_texture_edges_are_made_of_the_references_taps(rt, gold):
    """rt_query_surface on the camera set's hits of texture_edges: every word of every rt_surface equals the record that surface_model.py
    makes of the taps the REFERENCE gave at those texcoords (pins_texture_edges.npz edge_hit_taps), not of the oracle's."""
    sd = surface_cases.scene_data("texture_edges")
    scene = rt.Scene(sd)
    try:
        o, d = tq._camera_rays(sd)
        hits, _ = scene.query_closest(o, d)
        got, st = scene.query_surface(hits)
    finally:
        scene.close()
    hit = hits["triangle"] != surface_cases.MISS
    uv = np.ascontiguousarray(hits["texcoord"]).view(np.uint32)
    assert np.array_equal(uv[hit], gold["edge_hit_uv"][hit]) and hit.sum() > 1000, "the device's hits are not the ones the golden taps answer"
    table = {}
    for i in np.flatnonzero(hit):
        m = sd.materials[int(sd.material_index[hits["triangle"][i]])]
        for k, kind in enumerate(surface_cases.KINDS):
            if getattr(m, kind) >= 0:
                table[(int(sd.texture_source[getattr(m, kind)]), int(uv[i, 0]), int(uv[i, 1]), int(k < 2))] = gold["edge_hit_taps"][i, k]

    def tap(image, tu, tv, srgb):
        return table[(image, int(F(tu).view(np.uint32)), int(F(tv).view(np.uint32)), srgb)]
    want = sm.expected_surfaces(rt, sd, hits, tap)
    assert st.rays == len(hits) and st.invalid_rays == 0
    assert np.array_equal(surface_cases.words(got), surface_cases.words(want)), surface_cases.first_difference(surface_cases.words(got), surface_cases.words(want))
    assert len(np.unique(got["material"][hit])) == len(surface_cases.EDGE_ROWS)


@pytest.fixture(params=["persistent", "wavefront", "mega"])
def kernel(request, monkeypatch):
    monkeypatch.setenv("RTAMD_KERNEL", request.param)
    return request.param


@pytest.mark.parametrize("key", PATH_CASES)
def test_renders_equal_reference_paths(rt, gold_paths, kernel, key):
    """The reference's own Scene::getPixel, float radiance per pixel, by the bar test_gpu_scenes.py::test_textured_room_matches_oracle holds
    each pipeline to: the persistent pipeline bit for bit; the round and mega pipelines, which keep the walkers' padded boxes, RMSE < 1e-3
    with at most 2 pixels off."""
    name, depth = PATH_CASES[key]
    scene = rt.Scene(surface_cases.scene_data(name))
    try:
        rgb, _, st = scene.render(*FRAME, ray_depth=depth)
    finally:
        scene.close()
    ref = gold_paths[key]
    rmse, bad = _report(f"{key}[{kernel}] {FRAME[0]}x{FRAME[1]}x{FRAME[2]} depth {depth}", rgb, ref)
    assert _parity(kernel, rmse, bad, rgb, ref, None, None, max_bad=2)
    assert st.reference_exact == (1 if kernel == "persistent" else 0)

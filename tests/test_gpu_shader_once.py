"""The persistent kernel's shader takes a hit at the deepest level through the same sections as every other hit (rt_persistent.h,
pt_shade_lean): the pixels stay the reference's bit for bit at the depths where such hits are all, half or a sixth of the shaded hits,
and the deepest level still traces nothing and sums no light pdf."""
import os
import sys

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def small_room(rt, tmp_path_factory):
    import gen_synth_room
    path, _ = gen_synth_room.generate(str(tmp_path_factory.mktemp("room")), 8, 12, 9, tex_size=64)
    return rt.load_gltf(path)


def _render_and_compare(rt, sd, width, height, spp, depth):
    scene = rt.Scene(sd)
    rgb, rgb8, st = scene.render(width, height, spp, ray_depth=depth)
    scene.close()
    ref, ref8, _ = oracle_lib.Hw8Oracle(sd).render(width, height, spp, ray_depth=depth)
    print(f"{width}x{height}x{spp} depth {depth}: floats equal {np.array_equal(rgb, ref)}, byte mismatches {int((rgb8 != ref8).sum())}, "
          f"light-pdf queries {st.light_pdf_queries} of {st.samples} samples, closest-hit queries {st.closest_hit_queries}")
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT
    assert np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    return st


def _no_trace_at_the_last_level(st, depth):
    if depth == 1:
        assert st.light_pdf_queries == 0
    assert st.light_pdf_queries <= st.samples * (depth - 1)


@pytest.mark.parametrize("depth", [1, 2, 6])
def test_textured_room_by_depth(rt, small_room, depth):
    st = _render_and_compare(rt, small_room, 96, 54, 9, depth)
    assert st.samples == 96 * 54 * 9
    _no_trace_at_the_last_level(st, depth)


@pytest.mark.parametrize("depth", [1, 2])
def test_emission_texture_by_depth(rt, sphere_scene, depth):
    """sphere_emissive.gltf: the emission of a hit at the deepest level is a texture lookup, made by the common attribute code"""
    st = _render_and_compare(rt, sphere_scene, 64, 64, 4, depth)
    _no_trace_at_the_last_level(st, depth)


def test_the_query_bound_can_fail(rt, small_room, monkeypatch):
    """Without the shortcut (RTAMD_NO_LAST_LEVEL_SHORTCUT=1) a depth-1 render does sum light pdfs: the bound above is a condition."""
    monkeypatch.setenv("RTAMD_NO_LAST_LEVEL_SHORTCUT", "1")
    scene = rt.Scene(small_room)
    _, _, st = scene.render(96, 54, 9, ray_depth=1)
    scene.close()
    print(f"shortcut off, depth 1: light-pdf queries {st.light_pdf_queries}")
    assert st.light_pdf_queries > 0

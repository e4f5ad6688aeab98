"""Light-pdf sums settled where the ray is made (rt_persistent.h PT_LIGHT_SETTLE): a bounce whose light-tree walk would enter no
record of the tree's root gets the walker's sum of no hits from the shader and never reaches the light walker.  The pixels must stay
the reference's, bit for bit, floats and bytes: on the headline frame where the lamp sphere and the ceiling quads are in view, in a
scene without lights, with a single-triangle light (a root with one used record) and on an emitter-less sphere lit by an
environment map."""
import os
import sys

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _check_exact(rt, scene, sd, w, h, spp):
    rgb, rgb8, st = scene.render(w, h, spp)
    ref, ref8, cnt = oracle_lib.Hw8Oracle(sd).render(w, h, spp)
    print(f"{w}x{h}x{spp}: {st.closest_hit_queries}+{st.light_pdf_queries} queries (oracle light sums {cnt.lightq}), "
          f"bit_exact {np.array_equal(rgb, ref)} byte_mismatch {(rgb8 != ref8).sum()}")
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.reference_exact == 1
    assert np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    return rgb, rgb8, st


def _check_counting_render(scene, rgb, rgb8, st, w, h, spp):
    """The counting variant of the kernel classifies every light sum (and settles the same ones): same pixels, same query counts."""
    rgb_c, rgb8_c, st_c = scene.render(w, h, spp, counters=True)
    assert np.array_equal(rgb_c, rgb) and np.array_equal(rgb8_c, rgb8)
    assert (st_c.closest_hit_queries, st_c.light_pdf_queries) == (st.closest_hit_queries, st.light_pdf_queries)


def test_headline_frame_crops_with_the_lights_in_view(rt, tmp_path):
    """The bench frame (1920x1080x256) in full; the oracle replays full-size 32x32 crops: the brightest tile of the frame and of its
    upper third (the lamp sphere and the ceiling quads: rays that start on a light, and the bounces beside it whose sums are settled at
    the root or walked), and two fixed tiles of the lit room."""
    import gen_synth_room
    path, _ = gen_synth_room.generate(str(tmp_path), 64, 50, 43)
    sd = rt.load_gltf(path)
    scene = rt.Scene(sd)
    rgb, rgb8, st = scene.render(1920, 1080, 256)
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.reference_exact == 1
    tiles = rgb[:1056].astype(np.float64).reshape(33, 32, 60, 32, 3).mean(axis=(1, 3, 4))
    ty, tx = np.unravel_index(int(np.argmax(tiles)), tiles.shape)
    uy, ux = np.unravel_index(int(np.argmax(tiles[:11])), tiles[:11].shape)
    crops = [(int(tx) * 32, int(ty) * 32), (int(ux) * 32, int(uy) * 32), (944, 524), (1700, 96)]
    orc = oracle_lib.Hw8Oracle(sd)
    for (x0, y0) in dict.fromkeys(crops):
        ref, ref8, _ = orc.render(1920, 1080, 256, rect=(x0, y0, 32, 32))
        crop, crop8 = rgb[y0:y0 + 32, x0:x0 + 32], rgb8[y0:y0 + 32, x0:x0 + 32]
        print(f"1080p crop ({x0},{y0}): mean {crop.mean():.4f} bit_exact {np.array_equal(crop, ref)} byte_mismatch {(crop8 != ref8).sum()}")
        assert np.array_equal(crop, ref) and np.array_equal(crop8, ref8)
    scene.close()


def test_scene_without_lights(rt):
    """No emissive triangle: no bounce asks for a light sum, so nothing is settled or walked (the mixture has no light component)."""
    sd = pin_cases.random_triangle_scene(n=300, seed=21, n_emissive_mats=0)
    scene = rt.Scene(sd)
    rgb, rgb8, st = _check_exact(rt, scene, sd, 64, 48, 6)
    assert st.light_pdf_queries == 0
    _check_counting_render(scene, rgb, rgb8, st, 64, 48, 6)
    scene.close()


def test_single_triangle_light(rt):
    """One emissive triangle, a large one above the soup: the light tree's root holds one used record (a leaf) and three unused ones
    that are never entered."""
    sd = pin_cases.random_triangle_scene(n=300, seed=22, n_emissive_mats=1)
    mat = sd.material_index.copy()
    mat[mat == 0] = 1
    mat[7] = 0
    pos = sd.positions.copy()
    pos[7] = [-3, 3.2, -3, 0, 3.2, 3, 3, 3.2, -3]
    sd = rt.SceneData(pos, sd.texcoords, sd.normals, sd.tangents, mat, list(sd.materials)[:sd.n_materials], camera=sd.camera)
    scene = rt.Scene(sd)
    rgb, rgb8, st = _check_exact(rt, scene, sd, 80, 60, 8)
    assert st.light_pdf_queries > 0 and rgb.mean() > 0.001
    _check_counting_render(scene, rgb, rgb8, st, 80, 60, 8)
    scene.close()


def test_emitterless_sphere_with_environment_map(rt, tmp_path):
    """sphere_roughness.gltf (no emitters) under an environment map: every bounce that leaves the sphere misses into the map."""
    import gen_synth_room
    yy, xx = np.mgrid[0:32, 0:64]
    env = np.stack([90 + 80 * np.sin(xx / 64 * 2 * np.pi), 130 + 60 * np.cos(yy / 32 * np.pi), 180 - yy * 3], axis=2).clip(0, 255).astype(np.uint8)
    env_path = str(tmp_path / "env.png")
    gen_synth_room.write_png(env_path, env)
    sd = rt.load_gltf(os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_roughness.gltf"), environment=env_path)
    scene = rt.Scene(sd)
    rgb, rgb8, st = _check_exact(rt, scene, sd, 72, 72, 8)
    assert rgb.mean() > 0.02
    _check_counting_render(scene, rgb, rgb8, st, 72, 72, 8)
    scene.close()


def test_emissive_sphere_counting_render(rt, sphere_scene):
    """The emissive sphere (a light tree of many triangles around the camera's view): every sum is classified by the counting
    variant and the settled ones give the oracle's pixels."""
    scene = rt.Scene(sphere_scene)
    rgb, rgb8, st = _check_exact(rt, scene, sphere_scene, 64, 64, 8)
    assert st.light_pdf_queries > 0
    _check_counting_render(scene, rgb, rgb8, st, 64, 64, 8)
    scene.close()

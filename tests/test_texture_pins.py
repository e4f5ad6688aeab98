"""Pins the texture layer and the whole hw8 integrator to the compiled reference's own hw8 scene.cpp (oracle/ref/ref_hw8_scene.cpp: the
file is built unmodified behind a one-line stand-in for its third-party header).

  texture taps and normal maps   tests/texture_cases.py -> tests/golden/pins_texture_edges.npz: the oracle's sample_texture and
                                 apply_normal_map, and surface_model.py's numpy apply_normal_map, equal the reference's static
                                 sampleTexture / applyNormalMaps; equal bits, or NaN on both sides
  paths                          tests/golden/pins_hw8_paths.npz: Hw8Oracle.render equals the reference's Scene::getPixel on every pixel of
                                 PATH_CASES, textures, normal maps and environment map included

Neither needs oracle/_ref at test time.  The same files then hold the device (test_gpu_texture.py)."""
import os

import numpy as np
import pytest

import oracle_lib
import surface_cases
import surface_model as sm
import texture_cases as tc
from test_shading_pins import differing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD, GOLD_PATHS = os.path.join(GOLDEN, "pins_texture_edges.npz"), os.path.join(GOLDEN, "pins_hw8_paths.npz")
F = np.float32
FRAME = (48, 32, 16)
SURFACE_SCENES = ("sphere", "sphere_emissive", "sphere_roughness", "soup_a", "soup_b")
# key of pins_hw8_paths.npz: (scene of surface_cases.py, ray depth)
PATH_CASES = {**{name: (name, 6) for name in SURFACE_SCENES}, **{name + "_env": (name + "_env", 6) for name in SURFACE_SCENES},
              "texture_edges": ("texture_edges", 6),
              **{f"{name}_depth{d}": (name, d) for name in ("soup_a", "soup_b") for d in (1, 2)}}
DARK = ("sphere", "sphere_roughness")       # no emitter and a black background: the reference's frame is black (their _env twins are not)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gold_paths():
    return dict(np.load(GOLD_PATHS))


@pytest.mark.parametrize("family", tc.REFERENCE_FAMILIES)
def test_oracle_equals_reference_at_the_edges(gold, family):
    got, want = tc.oracle_answers()[family], gold[family]
    bad = differing(got, want)
    print(f"{family}: {len(want)} cases, {bad.size} differ from the reference")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_numpy_normal_map_equals_reference(gold):
    """surface_model.apply_normal_map, which the first-hit layer's tests are held to, on the same rows."""
    rows = tc.families()["normal_map"]["rows"]
    got = sm.apply_normal_map(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7:10])
    bad = differing(got, gold["normal_map"])
    assert bad.size == 0, (bad[:5].tolist(), rows[bad[:5]].tolist(), got[bad[:5]].tolist(), gold["normal_map"][bad[:5]].tolist())


def test_nonfinite_coordinates_give_nan_in_every_channel():
    """NaN and infinite texcoords (a hit with den == 0 has NaN u and v).  The reference converts a NaN to int, which is undefined, so there is no
    golden answer: the oracle's is NaN in all three channels, and the device is held to that (test_gpu_texture.py)."""
    got = tc.oracle_answers()["nonfinite"]
    assert len(got) == 60 and np.isnan(got).all()
    uv = tc.families()["nonfinite"]["uv"]
    assert np.isnan(uv).any(axis=1).sum() >= 20 and np.isinf(uv).any(axis=1).sum() >= 20 and (~np.isfinite(uv[:, 0])).any() and (~np.isfinite(uv[:, 1])).any()


@pytest.mark.parametrize("key", PATH_CASES)
def test_oracle_render_equals_reference_path(gold_paths, key):
    name, depth = PATH_CASES[key]
    rgb, _, _ = surface_cases.oracle(name).render(*FRAME, ray_depth=depth)
    want = gold_paths[key]
    bad = differing(rgb.reshape(-1, 3), want.reshape(-1, 3))
    print(f"{key}: {rgb.shape[0] * rgb.shape[1]} pixels, {bad.size} differ from the reference, mean {float(np.nanmean(want)):.4f}")
    assert bad.size == 0, bad[:8].tolist()
    if key not in DARK:
        assert np.nanmean(want) > 0.005 and len(np.unique(want.reshape(-1, 3), axis=0)) > 100       # a picture, not a constant


def test_cases_reach_the_edges_they_claim(gold):
    """Counted over the reference's answers, so that a change of the table that loses an edge fails here and not silently."""
    fams = tc.families()
    # texel: every byte value in every channel under both curves, and the tap is the texel: channel c of case b is the value of byte ramp[b, c]
    ramp = tc.images()[0].reshape(256, 3)
    assert all(set(ramp[:, c].tolist()) == set(range(256)) for c in range(3))
    lut = np.stack([gold["texel"][:256, 0], gold["texel"][256:, 0]])                      # channel 0 of the ramp is b itself
    assert np.array_equal(lut[0].view(np.uint32), (F(1. / 255) * (F(1) * np.arange(256, dtype=F))).view(np.uint32))
    assert (np.diff(lut[1]) > 0).all() and lut[1, 0] == 0 and lut[1, 255] > 0.99
    for k in (0, 1):
        assert np.array_equal(gold["texel"][256 * k:256 * (k + 1)].view(np.uint32), lut[k][ramp].view(np.uint32))
    # past_end: enough of them, each exactly the blend that reads 0 for the texels past the end of the image, and 0 itself where every
    # texel with a weight lies there (row `height`)
    pe = fams["past_end"]
    assert len(pe["slot"]) >= 100 and len(pe["slot"]) == int(tc.past_end_mask(fams["tap"]).sum())
    model = tc.model_tap(pe, lut)
    bad = differing(model, gold["past_end"])
    assert bad.size == 0, (bad[:5].tolist(), model[bad[:5]].tolist(), gold["past_end"][bad[:5]].tolist())
    wh = tc.sizes_of(pe["slot"])
    row_h = tc.wrapped_index(pe["uv"][:, 1], wh[:, 1])[0] == wh[:, 1]
    col_w = tc.wrapped_index(pe["uv"][:, 0], wh[:, 0])[0] == wh[:, 0]
    last_row = tc.wrapped_index(pe["uv"][:, 1], wh[:, 1])[0] == wh[:, 1] - 1
    assert row_h.sum() >= 50 and (col_w & ~row_h).sum() >= 50 and (col_w & last_row).sum() >= 20
    assert np.all(gold["past_end"][row_h].view(np.uint32) == 0)
    share = len(pe["slot"]) / len(fams["tap"]["slot"])
    print(f"past_end: {len(pe['slot'])} of {len(fams['tap']['slot'])} taps ({100 * share:.1f} %), {int(row_h.sum())} in row `height`")
    # every image size is met, the environment map included, under both curves; results are numbers
    for s in list(range(1, len(tc.images()))) + [tc.ENV]:
        for name in ("tap", "past_end"):
            on = fams[name]["slot"] == s
            assert on.sum() >= 10 and set(fams[name]["srgb"][on].tolist()) == {0, 1}, (name, s)
    assert len(tc.images()) == 1 + len(tc.IMAGE_SIZES) and [im.shape[1::-1] for im in tc.images()[1:]] == list(tc.IMAGE_SIZES)
    assert tc.IMAGE_SIZES[-1] == (7, 3) and tc.env_image().shape == (3, 7, 3)
    assert not np.isnan(gold["tap"]).any() and len(np.unique(gold["tap"], axis=0)) > 3000
    assert 10000 <= len(fams["tap"]["slot"]) <= 14000 and len(fams["texel"]["slot"]) == 512 and len(fams["normal_map"]["rows"]) == 4000
    # normal_map: numbers carry the comparison, and the NaN of a zero local normal is there
    nan = np.isnan(gold["normal_map"]).any(axis=1)
    print(f"normal_map: {int(nan.sum())} of {len(nan)} answers are NaN")
    assert nan.mean() <= 0.10 and nan.sum() >= 10
    rows = fams["normal_map"]["rows"]
    flat = (rows[:, 7:10] == F(0.5)).all(axis=1)
    assert flat.sum() >= 10 and nan[flat].all()
    assert {1.0, -1.0, 2.0} <= set(rows[:, 6].tolist()) and (np.signbit(rows[:, 6]) & (rows[:, 6] == 0)).any() and (~np.signbit(rows[:, 6]) & (rows[:, 6] == 0)).any()


def test_texture_edges_scene_shows_every_row_of_its_table(gold):
    """First hits of the camera set: at least half on a textured material, every row of surface_cases.EDGE_ROWS under at least one pixel;
    and the golden taps answer the hits the oracle finds today, with the oracle's taps equal to them."""
    sd = surface_cases.scene_data("texture_edges")
    hits = tc.edge_hits()
    hit = hits["triangle"] != surface_cases.MISS
    mat = sd.material_index[hits["triangle"][hit]]
    textured = np.array([any(getattr(sd.materials[i], k) >= 0 for k in surface_cases.KINDS) for i in range(sd.n_materials)])
    print(f"texture_edges: {int(hit.sum())} of {len(hits)} rays hit, {int(textured[mat].sum())} on a textured material, per row {np.bincount(mat).tolist()}")
    assert textured[mat].sum() >= len(hits) / 2
    assert sd.n_materials == len(surface_cases.EDGE_ROWS) and np.all(np.bincount(mat, minlength=sd.n_materials) >= 1)
    assert np.array_equal(np.ascontiguousarray(hits["texcoord"]).view(np.uint32), gold["edge_hit_uv"])
    got = tc.edge_taps(oracle_lib.lib().rto_sample_texture, hits)
    assert differing(got, gold["edge_hit_taps"]).size == 0
    uv = hits["texcoord"][hit]
    assert (uv < -2).any() and (uv > 5000).any() and set(sd.texcoords[:2].reshape(-1).tolist()) == {0.0, 1.0}


def test_goldens_are_current_with_live_reference(gold, gold_paths):
    """Where the reference harness is built, the files are what it answers today."""
    if oracle_lib.ref_path("libref_hw8_scene.so") is None:
        print("oracle/_ref/libref_hw8_scene.so is not built: the golden files were not re-evaluated live")
        return
    live = tc.evaluate("reference")
    for family in tc.REFERENCE_FAMILIES:
        assert differing(live[family], gold[family]).size == 0, family
    for key in ("texture_edges", "soup_a_env", "soup_b_depth2"):
        name, depth = PATH_CASES[key]
        rgb, _, _ = oracle_lib.Ref8Scene(surface_cases.scene_data(name)).render(*FRAME, ray_depth=depth)
        assert differing(rgb.reshape(-1, 3), gold_paths[key].reshape(-1, 3)).size == 0, key

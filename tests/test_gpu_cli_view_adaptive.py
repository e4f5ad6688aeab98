"""The CLI's adaptive view sets on the sphere scene at 40x24: RTAMD_CAMERAS=file with RTAMD_ADAPTIVE=1 and RTAMD_TARGET_NOISE renders the
file's three cameras as one adaptive set and writes out_000.ppm .. out_002.ppm and, with RTAMD_SAMPLE_MAP=spp.pfm, spp_000.pfm ..
spp_002.pfm, equal to the binding's outputs for the same parameters, every sample count a multiple of the slice, one line per slice on
stderr; and without RTAMD_ADAPTIVE the RTAMD_CAMERAS run writes the bytes it always wrote.  (GPU needed: it renders.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_model as am
import view_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
W, H, SPP, SLICE = 40, 24, 24, 4
NAMES = ("own", "inside", "beside")
KNOBS = ("RTAMD_CAMERAS", "RTAMD_ADAPTIVE", "RTAMD_ADAPTIVE_DILATE", "RTAMD_SAMPLE_MAP", "RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_TARGET_NOISE",
         "RTAMD_NOISE_MIN_BATCHES", "RTAMD_NOISE_MAP", "RTAMD_DEVICE_LIST", "RTAMD_DEVICES", "RTAMD_SNAPSHOT", "RTAMD_DENOISE", "RTAMD_STREAMS")
LINE = re.compile(r"^slice (\d+): (\d+) views, (\d+) sub-tiles drew (\d+) samples, (\d+) converged, (\d+) capped, (\d+) \.\. (\d+) samples per pixel, \S+ ms on the GPU$", re.M)


def _run(out, **env):
    for k in KNOBS:
        assert k not in os.environ
    return subprocess.run([MAIN, SPHERE, str(W), str(H), str(SPP), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RTAMD_DEVICES="1", **env))


def _pixels(path):
    data = path.read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 3
    return np.frombuffer(data, np.uint8, W * H * 3, len(head)).reshape(H, W, 3)


def _counts(path):
    data = path.read_bytes()
    head = f"Pf\n{W} {H}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 4
    return np.frombuffer(data, "<f4", W * H, len(head)).reshape(H, W)[::-1]    # a PFM's rows run from the bottom up


@pytest.fixture(scope="module")
def scene(rt, sphere_scene):
    s = rt.Scene(sphere_scene)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cameras(sphere_scene):
    t = vc.table(sphere_scene)
    return [t[n] for n in NAMES]


@pytest.fixture(scope="module")
def cams_file(cameras, tmp_path_factory):
    path = tmp_path_factory.mktemp("cams") / "cams.txt"
    path.write_text("# position right up forward fov_y\n" + "\n".join(" ".join("%.9g" % x for x in vc.fields(c)) for c in cameras) + "\n")
    return path


@pytest.fixture(scope="module")
def target(scene, cameras):
    """The median over the three views' sub-tiles that have any noise of (noise / that view's mean luminance) after four uniform slices:
    the quiet sub-tiles and about half of the others meet it."""
    a = scene.adaptive_views(W, H, cameras, 1.0)
    ones = np.ones((3,) + a.grid, np.uint8)
    for _ in range(4):
        a.render_tiles(SLICE, ones)
    ratios = []
    for v in range(3):
        t = a.tiles(v)
        noise = np.nan_to_num(am.tile_noise(t))
        ratios.append(noise[noise > 0] / am.mean_luminance(t))
    a.close()
    value = float(np.median(np.concatenate(ratios)))
    assert value > 0
    return value


@pytest.mark.parametrize("dilate", [False, True])
def test_adaptive_cameras_write_the_bindings_outputs(rt, scene, cameras, cams_file, target, tmp_path, dilate):
    out, pfm = tmp_path / "o.ppm", tmp_path / "spp.pfm"
    env = dict(RTAMD_CAMERAS=str(cams_file), RTAMD_ADAPTIVE="1", RTAMD_TARGET_NOISE=repr(target), RTAMD_SLICE=str(SLICE), RTAMD_SAMPLE_MAP=str(pfm))
    if dilate:
        env["RTAMD_ADAPTIVE_DILATE"] = "1"
    r = _run(out, **env)
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    # the same run through the binding: the command line's parameters are the default min_batches and the samples asked for as the cap
    a = scene.adaptive_views(W, H, cameras, target, min_batches=4, max_samples=SPP, dilate=dilate)
    stats = []
    while True:
        st = a.render(SLICE)
        if st.samples == 0:
            break
        stats.append(st)
    total = 0
    for v in range(3):
        assert np.array_equal(_pixels(tmp_path / ("o_%03d.ppm" % v)), a.resolve(v, want_float=False)[1]), v
        spp = a.sample_map(v)
        got = _counts(tmp_path / ("spp_%03d.pfm" % v))
        assert np.array_equal(got, spp.astype(np.float32)), v
        assert (got % SLICE == 0).all() and got.min() >= 4 * SLICE and got.max() <= SPP       # every count a multiple of the slice
        total += int(spp.sum())
    a.close()
    assert not out.exists() and not pfm.exists() and not (tmp_path / "o_003.ppm").exists()
    lines = LINE.findall(r.stderr)
    assert [int(l[0]) for l in lines] == list(range(1, len(stats) + 1)) and r.stderr.count("slice ") == len(stats)
    for l, st in zip(lines, stats):
        assert tuple(int(x) for x in l[1:]) == (st.active_views, st.active_tiles, SLICE, st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples)
    assert int(lines[0][2]) == 3 * 5 * 3 and int(lines[-1][2]) < 3 * 5 * 3   # every sub-tile of every view at first, fewer at the end
    drawn = int(re.search(r"(\d+) camera samples of the (\d+) a uniform run draws", r.stderr).group(1))
    assert drawn == total < 3 * W * H * SPP


def test_without_the_knob_the_cameras_run_is_what_it_was(rt, scene, cameras, cams_file, tmp_path):
    views = scene.views(W, H, cameras)
    views.render(SPP)
    want = [views.resolve(v, want_float=False)[1] for v in range(3)]
    views.close()
    for env in ({}, {"RTAMD_ADAPTIVE": "0"}, {"RTAMD_SAMPLE_MAP": str(tmp_path / "no.pfm")}):
        out = tmp_path / "o.ppm"
        r = _run(out, RTAMD_CAMERAS=str(cams_file), **env)
        assert r.returncode == 0 and "FINISH" in r.stderr and "sub-tiles" not in r.stderr, r.stderr
        for v in range(3):
            assert np.array_equal(_pixels(tmp_path / ("o_%03d.ppm" % v)), want[v]), v
        assert not (tmp_path / "no_000.pfm").exists() and not (tmp_path / "no.pfm").exists()


@pytest.mark.parametrize("env,who,word", [({}, "RTAMD_ADAPTIVE", "RTAMD_TARGET_NOISE"),
                                          ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_SNAPSHOT": "hw7"}, "RTAMD_ADAPTIVE", "hw8 integrator only"),
                                          ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_DEVICE_LIST": "0,0"}, "RTAMD_ADAPTIVE", "one GPU"),
                                          ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_CHECKPOINT": "c.bin"}, "RTAMD_ADAPTIVE", "no checkpoint"),
                                          ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_NOISE_MAP": "n.pfm"}, "RTAMD_CAMERAS", "a view set has no checkpoint, noise monitor"),
                                          ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_STREAMS": "2"}, "RTAMD_CAMERAS", "replay mode")])
def test_the_other_refusals_of_the_two_modes_stay(cams_file, tmp_path, env, who, word):
    r = _run(tmp_path / "o.ppm", RTAMD_CAMERAS=str(cams_file), RTAMD_ADAPTIVE="1", **env)
    assert r.returncode == 1 and "error: %s: " % who in r.stderr and word in r.stderr and not (tmp_path / "o_000.ppm").exists(), r.stderr
    assert "no adaptive sampling" not in r.stderr

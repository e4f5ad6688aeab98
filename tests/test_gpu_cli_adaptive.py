"""The CLI's adaptive mode on a 43x21 frame: RTAMD_ADAPTIVE=1 with RTAMD_TARGET_NOISE writes rt_adaptive_resolve's bytes and, with
RTAMD_SAMPLE_MAP, the samples per pixel, all multiples of the slice; it prints one line per slice; what it cannot serve ends with an
error naming the reason; and without RTAMD_ADAPTIVE the command line writes the bytes it always wrote.  (GPU needed: it renders.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
W, H, SPP, SLICE = 43, 21, 24, 4
KNOBS = ("RTAMD_ADAPTIVE", "RTAMD_ADAPTIVE_DILATE", "RTAMD_SAMPLE_MAP", "RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_SLICE_LIMIT", "RTAMD_TARGET_NOISE",
         "RTAMD_NOISE_MIN_BATCHES", "RTAMD_NOISE_MAP", "RTAMD_DEVICE_LIST", "RTAMD_DEVICES", "RTAMD_SNAPSHOT", "RTAMD_DENOISE")
LINE = re.compile(r"^slice (\d+): (\d+) sub-tiles drew (\d+) samples, (\d+) converged, (\d+) capped, (\d+) \.\. (\d+) samples per pixel, \S+ ms on the GPU(?:, noise (\S+) worst tile (\S+))?$", re.M)


def _run(out, **env):
    for k in KNOBS:
        assert k not in os.environ
    return subprocess.run([MAIN, SPHERE, str(W), str(H), str(SPP), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def _pixels(path):
    data = path.read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 3
    return np.frombuffer(data, np.uint8, W * H * 3, len(head)).reshape(H, W, 3)


@pytest.fixture(scope="module")
def scene(rt, sphere_scene):
    s = rt.Scene(sphere_scene)
    yield s
    s.close()


@pytest.fixture(scope="module")
def target(scene):
    """The median noise of the sub-tiles that have any (the background's have none) after four uniform slices, over the frame's mean
    luminance: the quiet sub-tiles and about half of the others meet it."""
    a = scene.adaptive(W, H, 1.0)
    ones = np.ones(a.grid, np.uint8)
    for _ in range(4):
        a.render_tiles(SLICE, ones)
    t = a.tiles()
    _, s = a.noise(want_map=False)
    a.close()
    noise = np.sqrt(t["sum_se2"].astype(np.float64) / np.maximum(t["pixels"], 1))
    value = float(np.median(noise[noise > 0]) / s.mean_luminance)
    assert value > 0
    return value


def test_adaptive_run_writes_resolve_and_the_sample_map(rt, scene, target, tmp_path):
    out, pfm = tmp_path / "o.ppm", tmp_path / "spp.pfm"
    r = _run(out, RTAMD_ADAPTIVE="1", RTAMD_TARGET_NOISE=repr(target), RTAMD_SLICE=str(SLICE), RTAMD_SAMPLE_MAP=str(pfm))
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    # the same run through the binding: the command line's parameters are the default min_batches and the samples asked for as the cap
    a = scene.adaptive(W, H, target, min_batches=4, max_samples=SPP)
    stats = []
    while True:
        st = a.render(SLICE)
        if st.samples == 0:
            break
        stats.append(st)
    _, rgb8 = a.resolve(want_float=False)
    spp = a.sample_map()
    a.close()
    assert np.array_equal(_pixels(out), rgb8)
    data = pfm.read_bytes()
    head = f"Pf\n{W} {H}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 4
    got = np.frombuffer(data, "<f4", W * H, len(head)).reshape(H, W)[::-1]    # a PFM's rows run from the bottom up
    assert np.array_equal(got, spp.astype(np.float32))
    assert (got % SLICE == 0).all() and got.min() >= 4 * SLICE and got.max() <= SPP and len(np.unique(got)) >= 2
    lines = LINE.findall(r.stderr)
    assert [int(l[0]) for l in lines] == list(range(1, len(stats) + 1)) and r.stderr.count("slice ") == len(stats)
    for l, st in zip(lines, stats):
        assert (int(l[1]), int(l[2]), int(l[3]), int(l[4]), int(l[5]), int(l[6])) == (st.active_tiles, SLICE, st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples)
        assert (l[7] == "") == (int(l[0]) < 2)                      # the frame's noise from the second slice on
    assert int(lines[0][1]) == 6 * 3 and int(lines[-1][1]) < 6 * 3  # every sub-tile at first, fewer at the end
    drawn = int(re.search(r"(\d+) camera samples of the (\d+) a uniform run draws", r.stderr).group(1))
    assert drawn == int(spp.sum()) < W * H * SPP


def test_without_the_knob_nothing_changes(scene, target, tmp_path):
    out = tmp_path / "o.ppm"
    _, want8, _ = scene.render(W, H, SPP, want_float=False)
    for env in ({}, {"RTAMD_ADAPTIVE": "0"}, {"RTAMD_SAMPLE_MAP": str(tmp_path / "no.pfm")}):
        r = _run(out, **env)
        assert r.returncode == 0 and "FINISH" in r.stderr and "sub-tiles" not in r.stderr, r.stderr
        assert np.array_equal(_pixels(out), want8) and not (tmp_path / "no.pfm").exists()
    # the noise target alone is the frame-wide stop it was: a uniform run that ends at some slice, the plain picture at that count
    r = _run(out, RTAMD_TARGET_NOISE=repr(target), RTAMD_SLICE=str(SLICE))
    assert r.returncode == 0 and "sub-tiles" not in r.stderr, r.stderr
    m = re.search(r"CONVERGED after \d+ slices at (\d+) of", r.stderr)
    _, at8, _ = scene.render(W, H, int(m.group(1)) if m else SPP, want_float=False)
    assert np.array_equal(_pixels(out), at8)


@pytest.mark.parametrize("env,word", [({}, "RTAMD_TARGET_NOISE"), ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_SNAPSHOT": "hw7"}, "hw8 integrator only"),
                                      ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_DEVICE_LIST": "0,0"}, "one GPU"),
                                      ({"RTAMD_TARGET_NOISE": "0.1", "RTAMD_CHECKPOINT": "c.bin"}, "no checkpoint")])
def test_what_it_cannot_serve_is_named(tmp_path, env, word):
    r = _run(tmp_path / "o.ppm", RTAMD_ADAPTIVE="1", **env)
    assert r.returncode == 1 and "error: RTAMD_ADAPTIVE: " in r.stderr and word in r.stderr and not (tmp_path / "o.ppm").exists(), r.stderr

"""The CLI's preview: RTAMD_DENOISE=path.ppm writes the filtered picture next to out.ppm, after every slice of a sliced run; its bytes
are Accumulator.denoise's of the binding at that point, with the monitor's error map whenever a monitor runs and has two batches, and
out.ppm is byte for byte the file of a run without the knob.  (GPU needed: it renders.)"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SPHERE = os.path.join(SCENES, "hw8_sphere", "sphere_emissive.gltf")
W, H, SPP, SLICE = 64, 48, 12, 4
KNOBS = ("RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_SLICE_LIMIT", "RTAMD_TARGET_NOISE", "RTAMD_NOISE_MIN_BATCHES", "RTAMD_NOISE_MAP", "RTAMD_DEVICE_LIST",
         "RTAMD_DENOISE", "RTAMD_DENOISE_ALBEDO", "RTAMD_SNAPSHOT", "RTAMD_STREAMS")


def _run(args, **env):
    assert not any(k in os.environ for k in KNOBS)
    return subprocess.run([MAIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def _ppm(path):
    data = path.read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 3, data[:20]
    return np.frombuffer(data, np.uint8, W * H * 3, len(head)).reshape(H, W, 3)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("plain") / "o.ppm"
    r = _run([SPHERE, W, H, SPP, out])
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    return out.read_bytes()


@pytest.fixture(scope="module")
def previews(rt, sphere_scene):
    """Accumulator.denoise's bytes after the slices of the run: without a monitor, with one, with one and the albedo, and after one slice of all samples."""
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(W, H)
    mon = acc.noise_monitor()
    for _ in range(SPP // SLICE):
        acc.render(SLICE)
        mon.update()
    want = dict(blind=acc.denoise()[1], map=acc.denoise(monitor=mon)[1], map_albedo=acc.denoise(monitor=mon, albedo=True)[1])
    assert not np.array_equal(want["blind"], want["map"]) and not np.array_equal(want["map"], want["map_albedo"])
    scene.close()
    return want


def test_sliced_run_writes_the_bindings_preview_and_the_plain_picture(tmp_path, plain, previews):
    out, dn = tmp_path / "o.ppm", tmp_path / "dn.ppm"
    r = _run([SPHERE, W, H, SPP, out], RTAMD_SLICE=str(SLICE), RTAMD_DENOISE=str(dn))
    assert r.returncode == 0 and "FINISH" in r.stderr and r.stderr.count("slice ") == SPP // SLICE, r.stderr
    assert out.read_bytes() == plain and not (tmp_path / "dn.ppm.part").exists()
    assert np.array_equal(_ppm(dn), previews["blind"])
    assert not np.array_equal(_ppm(dn), _ppm(out))
    # without RTAMD_SLICE the frame is one slice: the same samples, the same preview
    out1, dn1 = tmp_path / "o1.ppm", tmp_path / "dn1.ppm"
    r = _run([SPHERE, W, H, SPP, out1], RTAMD_DENOISE=str(dn1))
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    assert out1.read_bytes() == plain and np.array_equal(_ppm(dn1), previews["blind"])


def test_a_running_monitor_steers_the_preview(tmp_path, plain, previews):
    out, dn = tmp_path / "o.ppm", tmp_path / "dn.ppm"
    r = _run([SPHERE, W, H, SPP, out], RTAMD_SLICE=str(SLICE), RTAMD_DENOISE=str(dn), RTAMD_TARGET_NOISE="1e-9")
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    assert out.read_bytes() == plain and np.array_equal(_ppm(dn), previews["map"])
    r = _run([SPHERE, W, H, SPP, out], RTAMD_SLICE=str(SLICE), RTAMD_DENOISE=str(dn), RTAMD_TARGET_NOISE="1e-9", RTAMD_DENOISE_ALBEDO="1")
    assert r.returncode == 0 and out.read_bytes() == plain and np.array_equal(_ppm(dn), previews["map_albedo"]), r.stderr


def test_two_device_entries_write_the_same_preview(tmp_path, plain, previews):
    out, dn = tmp_path / "o.ppm", tmp_path / "dn.ppm"
    r = _run([SPHERE, W, H, SPP, out], RTAMD_SLICE=str(SLICE), RTAMD_DENOISE=str(dn), RTAMD_TARGET_NOISE="1e-9", RTAMD_DEVICE_LIST="0,0")
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    assert out.read_bytes() == plain and np.array_equal(_ppm(dn), previews["map"])


def test_preview_is_written_after_every_slice(tmp_path, rt, sphere_scene):
    out, dn = tmp_path / "o.ppm", tmp_path / "dn.ppm"
    r = _run([SPHERE, W, H, SPP, out], RTAMD_SLICE=str(SLICE), RTAMD_SLICE_LIMIT="1", RTAMD_DENOISE=str(dn))
    assert r.returncode == 0 and "STOPPED after 1 slices" in r.stderr, r.stderr
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(W, H)
    acc.render(SLICE)
    assert np.array_equal(_ppm(dn), acc.denoise()[1]) and np.array_equal(_ppm(out), acc.resolve()[1])
    scene.close()


def test_hw6_and_txt_scenes_say_so_and_render_as_ever(tmp_path):
    cases = [([os.path.join(SCENES, "hw6", "practice6_1.gltf"), 32, 24, 2], dict(RTAMD_SNAPSHOT="hw6")),
             ([os.path.join(SCENES, "txt", "hw2_sample.txt")], dict(RTAMD_SNAPSHOT="hw2"))]
    for k, (args, env) in enumerate(cases):
        a, b, dn = tmp_path / f"a{k}.ppm", tmp_path / f"b{k}.ppm", tmp_path / f"dn{k}.ppm"
        r0 = _run(args + [a], **env)
        r1 = _run(args + [b], RTAMD_DENOISE=str(dn), **env)
        assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
        assert r1.stderr.count("RTAMD_DENOISE") == 1 and "no preview is written" in r1.stderr and "RTAMD_DENOISE" not in r0.stderr
        assert not dn.exists() and a.read_bytes() == b.read_bytes()

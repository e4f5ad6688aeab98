"""The CLI's noise target: RTAMD_TARGET_NOISE ends a sliced run at the first slice whose estimated noise is at or below it (once
RTAMD_NOISE_MIN_BATCHES slices, 4 by default, were observed); the file is then byte for byte the plain run's at that many samples.
RTAMD_NOISE_MAP writes the last per-pixel standard error as a grayscale PFM.  (GPU needed: it renders.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
W, H, SPP, SLICE = 64, 48, 32, 4
NOISE_LINE = re.compile(r"^slice (\d+): \d+ samples \((\d+) of \d+\), .* noise (\S+) worst tile (\S+)$", re.M)


def _run(out, samples=SPP, **env):
    for k in ("RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_SLICE_LIMIT", "RTAMD_TARGET_NOISE", "RTAMD_NOISE_MIN_BATCHES", "RTAMD_NOISE_MAP", "RTAMD_DEVICE_LIST"):
        assert k not in os.environ
    return subprocess.run([MAIN, SPHERE, str(W), str(H), str(samples), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The plain run's file after d samples, rendered once per d."""
    d = tmp_path_factory.mktemp("plain")
    files = {}

    def at(samples):
        if samples not in files:
            r = _run(d / f"{samples}.ppm", samples=samples)
            assert r.returncode == 0 and "FINISH" in r.stderr and "noise" not in r.stderr, r.stderr
            files[samples] = (d / f"{samples}.ppm").read_bytes()
        return files[samples]

    return at


@pytest.fixture(scope="module")
def full(tmp_path_factory, plain):
    """A monitored run that never reaches its target: stderr with the noise after every slice from the second on."""
    out = tmp_path_factory.mktemp("full") / "o.ppm"
    r = _run(out, RTAMD_SLICE=str(SLICE), RTAMD_TARGET_NOISE="1e-9")
    assert r.returncode == 0 and "FINISH" in r.stderr and "CONVERGED" not in r.stderr, r.stderr
    assert out.read_bytes() == plain(SPP)
    return r.stderr


def test_a_loose_target_stops_at_the_fourth_slice(tmp_path, plain, full):
    out = tmp_path / "o.ppm"
    r = _run(out, RTAMD_SLICE=str(SLICE), RTAMD_TARGET_NOISE="1e9")
    assert r.returncode == 0 and "CONVERGED after 4 slices at 16 of 32" in r.stderr and "FINISH" in r.stderr, r.stderr
    assert r.stderr.count("slice ") == 4 and out.read_bytes() == plain(16)
    # the numbers printed up to there are the full run's
    assert NOISE_LINE.findall(r.stderr) == NOISE_LINE.findall(full)[:3]
    # two device entries: the same numbers and the same file
    out2 = tmp_path / "o2.ppm"
    r2 = _run(out2, RTAMD_SLICE=str(SLICE), RTAMD_TARGET_NOISE="1e9", RTAMD_DEVICE_LIST="0,0")
    assert r2.returncode == 0 and "CONVERGED after 4 slices at 16 of 32" in r2.stderr, r2.stderr
    assert NOISE_LINE.findall(r2.stderr) == NOISE_LINE.findall(r.stderr) and out2.read_bytes() == plain(16)
    # RTAMD_NOISE_MIN_BATCHES moves the earliest stop; without RTAMD_SLICE a slice is a sixteenth of the samples
    r = _run(out, RTAMD_TARGET_NOISE="1e9", RTAMD_NOISE_MIN_BATCHES="2")
    assert r.returncode == 0 and "CONVERGED after 2 slices at 4 of 32" in r.stderr and out.read_bytes() == plain(4), r.stderr


def test_a_target_never_reached_runs_to_the_end(full):
    lines = NOISE_LINE.findall(full)
    assert [int(k) for k, _, _, _ in lines] == list(range(2, SPP // SLICE + 1)) and full.count("slice ") == SPP // SLICE
    assert all(float(n) > 0 and float(t) >= float(n) for _, _, n, t in lines)


def test_a_middle_target_stops_where_the_printed_numbers_say(tmp_path, plain, full):
    lines = [(int(k), int(d), float(n)) for k, d, n, _ in NOISE_LINE.findall(full)]
    values = sorted({n for _, _, n in lines})
    assert len(values) >= 2
    target = (values[0] + values[1]) / 2
    stop = next(((k, d) for k, d, n in lines if k >= 4 and n <= target), None)
    out = tmp_path / "o.ppm"
    r = _run(out, RTAMD_SLICE=str(SLICE), RTAMD_TARGET_NOISE=repr(target))
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    print(f"noise per slice {[(k, n) for k, _, n in lines]}, target {target!r}, expected stop {stop}")
    if stop is None:
        assert "CONVERGED" not in r.stderr and out.read_bytes() == plain(SPP)
    else:
        assert f"CONVERGED after {stop[0]} slices at {stop[1]} of {SPP}" in r.stderr, r.stderr
        assert out.read_bytes() == plain(stop[1])


@pytest.mark.parametrize("value", ["0", "-1", "abc", "inf", "nan", "1e-3x"])
def test_bad_targets_are_refused(tmp_path, value):
    r = _run(tmp_path / "o.ppm", RTAMD_TARGET_NOISE=value)
    assert r.returncode == 1 and "RTAMD_TARGET_NOISE" in r.stderr and not (tmp_path / "o.ppm").exists(), r.stderr


def test_noise_map_is_the_python_map_at_the_stopping_point(rt, sphere_scene, tmp_path):
    out, pfm = tmp_path / "o.ppm", tmp_path / "se.pfm"
    r = _run(out, RTAMD_SLICE=str(SLICE), RTAMD_TARGET_NOISE="1e9", RTAMD_NOISE_MAP=str(pfm))
    assert r.returncode == 0 and "CONVERGED after 4 slices at 16 of 32" in r.stderr, r.stderr
    data = pfm.read_bytes()
    head = f"Pf\n{W} {H}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 4 and not (tmp_path / "se.pfm.part").exists()
    got = np.frombuffer(data, "<f4", W * H, len(head)).reshape(H, W)[::-1]   # a PFM's rows run from the bottom up
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(W, H)
    mon = acc.noise_monitor()
    for _ in range(4):
        acc.render(SLICE)
        mon.update()
    se, s = mon.estimate()
    scene.close()
    assert np.array_equal(got, se) and se.max() > 0
    assert float(NOISE_LINE.findall(r.stderr)[-1][2]) == float("%.9g" % s.noise)

"""The CLI's progressive surface: RTAMD_SLICE renders in slices and rewrites the PPM after each, RTAMD_CHECKPOINT carries a frame
over from one run to the next; the finished file is byte for byte the plain run's (GPU needed: it renders)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")


def _run(out, samples=24, size=("48", "32"), **env):
    for k in ("RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_SLICE_LIMIT"):
        assert k not in os.environ
    return subprocess.run([MAIN, SPHERE, size[0], size[1], str(samples), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def test_cli_slices_write_the_plain_runs_file(tmp_path):
    plain, sliced = tmp_path / "plain.ppm", tmp_path / "sliced.ppm"
    r = _run(plain)
    assert r.returncode == 0 and "FINISH" in r.stderr and "slice" not in r.stderr, r.stderr
    r = _run(sliced, RTAMD_SLICE="8")
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    assert r.stderr.count("slice ") == 3 and "(24 of 24)" in r.stderr
    assert sliced.read_bytes() == plain.read_bytes()
    assert not (tmp_path / "sliced.ppm.part").exists()
    # a slice length that does not divide the samples: the last slice is shorter
    r = _run(sliced, RTAMD_SLICE="10")
    assert r.returncode == 0 and r.stderr.count("slice ") == 3 and "slice 3: 4 samples" in r.stderr, r.stderr
    assert sliced.read_bytes() == plain.read_bytes()
    r = _run(sliced, RTAMD_SLICE="0")
    assert r.returncode != 0 and "RTAMD_SLICE" in r.stderr


def test_cli_checkpoint_stops_and_carries_on(tmp_path):
    plain, out, ck = tmp_path / "plain.ppm", tmp_path / "o.ppm", tmp_path / "frame.ckpt"
    assert _run(plain).returncode == 0
    eight = tmp_path / "eight.ppm"
    assert _run(eight, samples=8).returncode == 0
    # first run: stopped after one slice of 8 (the process ends by itself); the picture so far is the 8-sample frame
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck), RTAMD_SLICE_LIMIT="1")
    assert r.returncode == 0 and "STOPPED after 1 slices at 8 of 24" in r.stderr and "FINISH" not in r.stderr, r.stderr
    assert ck.exists() and not (tmp_path / "frame.ckpt.part").exists()
    assert out.read_bytes() == eight.read_bytes()
    # second run: carries on from the checkpoint
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck))
    assert r.returncode == 0 and "FINISH" in r.stderr and "8 of 24 samples done" in r.stderr and r.stderr.count("slice ") == 2, r.stderr
    assert out.read_bytes() == plain.read_bytes()
    # the checkpoint now holds the whole frame: a third run just resolves it
    out.unlink()
    r = _run(out, RTAMD_CHECKPOINT=str(ck))
    assert r.returncode == 0 and "FINISH" in r.stderr and "slice " not in r.stderr, r.stderr
    assert out.read_bytes() == plain.read_bytes()
    # fewer samples than it holds, or another frame: an error, never a silent restart; the checkpoint stays
    before = ck.read_bytes()
    r = _run(out, samples=16, RTAMD_CHECKPOINT=str(ck))
    assert r.returncode != 0 and "more than the 16 asked for" in r.stderr, r.stderr
    r = _run(out, size=("40", "32"), RTAMD_CHECKPOINT=str(ck))
    assert r.returncode != 0 and "does not match" in r.stderr and "width" in r.stderr, r.stderr
    assert ck.read_bytes() == before
    # a checkpoint alone (no RTAMD_SLICE): one slice of everything that is left
    ck2 = tmp_path / "whole.ckpt"
    r = _run(out, RTAMD_CHECKPOINT=str(ck2))
    assert r.returncode == 0 and r.stderr.count("slice ") == 1 and out.read_bytes() == plain.read_bytes(), r.stderr
    assert ck2.read_bytes()[128:] == before[128:]

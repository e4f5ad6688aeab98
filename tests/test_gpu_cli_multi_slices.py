"""The CLI's progressive surface on several devices: with RTAMD_DEVICE_LIST the slices and the checkpoint go through rt_multi_accum_*,
the files are byte for byte the single-device run's, and a checkpoint written by one kind of run is finished by the other (GPU
needed: it renders).  The list repeats device 0: two physical GPUs are never involved."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
LIST = "0,0,0"


def _run(out, samples=24, **env):
    for k in ("RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_SLICE_LIMIT", "RTAMD_DEVICE_LIST"):
        assert k not in os.environ
    # RTAMD_DEVICES=1: a run without the list is the single-device run on any machine
    return subprocess.run([MAIN, SPHERE, "48", "32", str(samples), str(out)], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, RTAMD_DEVICES="1", **env))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The plain single-device run's PPM and the single-device sliced run's finished checkpoint."""
    d = tmp_path_factory.mktemp("plain")
    r = _run(d / "plain.ppm")
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    r = _run(d / "single.ppm", RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(d / "single.ckpt"))
    assert r.returncode == 0 and "FINISH" in r.stderr and "GPUs" not in r.stderr, r.stderr
    assert (d / "single.ppm").read_bytes() == (d / "plain.ppm").read_bytes()
    return (d / "plain.ppm").read_bytes(), (d / "single.ckpt").read_bytes()


def test_cli_sliced_on_a_device_list_writes_the_plain_runs_file(tmp_path, plain):
    out = tmp_path / "sliced.ppm"
    r = _run(out, RTAMD_SLICE="8", RTAMD_DEVICE_LIST=LIST)
    assert r.returncode == 0 and "FINISH" in r.stderr and "one device" not in r.stderr, r.stderr
    assert r.stderr.count("slice ") == 3 and "(24 of 24)" in r.stderr
    assert out.read_bytes() == plain[0]
    assert not (tmp_path / "sliced.ppm.part").exists()
    # the list applies to an unsliced render too
    r = _run(out, RTAMD_DEVICE_LIST=LIST)
    assert r.returncode == 0 and "render: 3 GPUs" in r.stderr and "slice " not in r.stderr, r.stderr
    assert out.read_bytes() == plain[0]


def test_cli_checkpoint_from_a_device_list_is_finished_on_one_device(tmp_path, plain):
    out, ck = tmp_path / "o.ppm", tmp_path / "frame.ckpt"
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck), RTAMD_SLICE_LIMIT="1", RTAMD_DEVICE_LIST=LIST)
    assert r.returncode == 0 and "STOPPED after 1 slices at 8 of 24" in r.stderr and "FINISH" not in r.stderr, r.stderr
    assert ck.exists() and not (tmp_path / "frame.ckpt.part").exists()
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck))          # no list: one device
    assert r.returncode == 0 and "FINISH" in r.stderr and "8 of 24 samples done" in r.stderr and r.stderr.count("slice ") == 2, r.stderr
    assert out.read_bytes() == plain[0]
    assert ck.read_bytes() == plain[1]                                # the finished checkpoint, all bytes


def test_cli_checkpoint_from_one_device_is_finished_on_a_device_list(tmp_path, plain):
    out, ck = tmp_path / "o.ppm", tmp_path / "frame.ckpt"
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck), RTAMD_SLICE_LIMIT="1")
    assert r.returncode == 0 and "STOPPED after 1 slices at 8 of 24" in r.stderr, r.stderr
    r = _run(out, RTAMD_SLICE="8", RTAMD_CHECKPOINT=str(ck), RTAMD_DEVICE_LIST=LIST)
    assert r.returncode == 0 and "FINISH" in r.stderr and "8 of 24 samples done" in r.stderr and r.stderr.count("slice ") == 2, r.stderr
    assert out.read_bytes() == plain[0]
    assert ck.read_bytes() == plain[1]
    # the error texts are the single-device run's
    before = ck.read_bytes()
    r = _run(out, samples=16, RTAMD_CHECKPOINT=str(ck), RTAMD_DEVICE_LIST=LIST)
    assert r.returncode != 0 and "more than the 16 asked for" in r.stderr, r.stderr
    r = subprocess.run([MAIN, SPHERE, "40", "32", "24", str(out)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, RTAMD_CHECKPOINT=str(ck), RTAMD_DEVICE_LIST=LIST))
    assert r.returncode != 0 and "does not match" in r.stderr and "width" in r.stderr, r.stderr
    assert ck.read_bytes() == before


@pytest.mark.parametrize("bad", ["", "0,,0", "0,x", "-1", "0,99999", "0;0", "0,"])
def test_cli_bad_device_list(tmp_path, bad):
    r = _run(tmp_path / "o.ppm", RTAMD_DEVICE_LIST=bad)
    assert r.returncode != 0 and "RTAMD_DEVICE_LIST" in r.stderr and "FINISH" not in r.stderr, r.stderr
    assert not (tmp_path / "o.ppm").exists()

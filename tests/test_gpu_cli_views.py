"""The CLI's view sets on the sphere scene at 40x24: RTAMD_CAMERAS=file renders the file's three cameras as one view set and writes
out_000.ppm .. out_002.ppm beside the named output, byte-equal to the library's views, in one slice or with RTAMD_SLICE in several; a
malformed line ends the run with an error that names the line.  (GPU needed: it renders.)"""
import os
import subprocess

import numpy as np
import pytest

import view_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
W, H, SPP = 40, 24, 8
NAMES = ("own", "inside", "beside")
KNOBS = ("RTAMD_CAMERAS", "RTAMD_ADAPTIVE", "RTAMD_SLICE", "RTAMD_CHECKPOINT", "RTAMD_TARGET_NOISE", "RTAMD_NOISE_MAP", "RTAMD_DEVICE_LIST", "RTAMD_DEVICES",
         "RTAMD_SNAPSHOT", "RTAMD_DENOISE", "RTAMD_STREAMS")


def _run(out, **env):
    for k in KNOBS:
        assert k not in os.environ
    return subprocess.run([MAIN, SPHERE, str(W), str(H), str(SPP), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RTAMD_DEVICES="1", **env))


def _pixels(path):
    data = path.read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + W * H * 3
    return np.frombuffer(data, np.uint8, W * H * 3, len(head)).reshape(H, W, 3)


def _lines(sphere_scene):
    t = vc.table(sphere_scene)
    return [" ".join("%.9g" % x for x in vc.fields(t[n])) for n in NAMES]


@pytest.fixture(scope="module")
def library(rt, sphere_scene):
    """The three views' bytes by the library, default depth, 8 samples in one slice."""
    scene = rt.Scene(sphere_scene)
    t = vc.table(sphere_scene)
    views = scene.views(W, H, [t[n] for n in NAMES])
    views.render(SPP)
    out = [views.resolve(v, want_float=False)[1] for v in range(3)]
    views.close(); scene.close()
    return out


@pytest.mark.parametrize("slices", [None, "3"])
def test_cameras_file_writes_the_library_views(rt, sphere_scene, library, tmp_path, slices):
    cams = tmp_path / "cams.txt"
    cams.write_text("# position right up forward fov_y\n" + "\n\n".join(_lines(sphere_scene)) + "\n")
    out = tmp_path / "o.ppm"
    env = dict(RTAMD_CAMERAS=str(cams))
    if slices:
        env["RTAMD_SLICE"] = slices
    r = _run(out, **env)
    assert r.returncode == 0 and "FINISH" in r.stderr, r.stderr
    assert r.stderr.count("slice: 3 views drew") == (3 if slices else 0)      # 3 + 3 + 2 samples
    for v in range(3):
        assert np.array_equal(_pixels(tmp_path / ("o_%03d.ppm" % v)), library[v]), v
    assert not out.exists() and not (tmp_path / "o_003.ppm").exists()


def test_a_malformed_line_names_itself(rt, sphere_scene, tmp_path):
    good = _lines(sphere_scene)
    for bad in (" ".join(good[1].split()[:12]), good[1] + " 1.0", good[1].replace(" ", " x", 1)):
        cams = tmp_path / "bad.txt"
        cams.write_text("\n".join([good[0], "# a comment", bad, good[2]]) + "\n")
        out = tmp_path / "b.ppm"
        r = _run(out, RTAMD_CAMERAS=str(cams))
        assert r.returncode != 0 and "FINISH" not in r.stderr
        assert "RTAMD_CAMERAS" in r.stderr and "line 3" in r.stderr and "RT_ERR_PARSE" in r.stderr, r.stderr
        assert not (tmp_path / "b_000.ppm").exists()
    r = _run(tmp_path / "c.ppm", RTAMD_CAMERAS=str(tmp_path / "none.txt"))
    assert r.returncode != 0 and "cannot open" in r.stderr
    r = _run(tmp_path / "d.ppm", RTAMD_CAMERAS=str(tmp_path / "bad.txt"), RTAMD_SNAPSHOT="hw7")
    assert r.returncode != 0 and "RTAMD_CAMERAS: it runs the hw8 integrator only" in r.stderr

"""The CLI's guide images: run.sh with RTAMD_GUIDES=prefix writes prefix_albedo.pfm, prefix_normal.pfm ("PF") and prefix_depth.pfm ("Pf")
holding rt_render_guides' planes at the frame's size, bottom row first as PFM has it, and out.ppm is byte for byte the run's without
the knob.  (GPU needed: it renders.)  run.sh starts ./build/main, which build.sh links to the built CLI; the test makes that link in a
directory of its own and runs the script there."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "raytracing-course-hw_amd", "rtamd_main")
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere.gltf")
W, H, SPP = 48, 32, 2


def _run_sh(cwd, out, **env):
    assert "RTAMD_GUIDES" not in os.environ
    os.makedirs(cwd / "build", exist_ok=True)
    if not os.path.lexists(cwd / "build" / "main"):
        os.symlink(MAIN, cwd / "build" / "main")
    return subprocess.run(["bash", os.path.join(ROOT, "run.sh"), SPHERE, str(W), str(H), str(SPP), str(out)], cwd=cwd, capture_output=True, text=True,
                          timeout=300, env=dict(os.environ, **env))


def _read_pfm(path, magic, channels):
    raw = open(path, "rb").read()
    head = f"{magic}\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + W * H * channels * 4, (raw[:32], len(raw))
    a = np.frombuffer(raw[len(head):], "<f4").reshape(H, W, channels)[::-1]        # PFM: bottom row first
    return a[..., 0] if channels == 1 else a


def test_run_sh_writes_the_guides_and_the_same_picture(rt, tmp_path):
    r0 = _run_sh(tmp_path, tmp_path / "plain.ppm")
    assert r0.returncode == 0 and "FINISH" in r0.stderr and "guides" not in r0.stderr, r0.stdout + r0.stderr
    prefix = tmp_path / "g"
    r = _run_sh(tmp_path, tmp_path / "out.ppm", RTAMD_GUIDES=str(prefix))
    assert r.returncode == 0 and "FINISH" in r.stderr and "guides: " in r.stderr, r.stdout + r.stderr
    assert (tmp_path / "out.ppm").read_bytes() == (tmp_path / "plain.ppm").read_bytes()
    scene = rt.Scene(rt.load_gltf(SPHERE))
    try:
        want, _ = scene.render_guides(W, H)
    finally:
        scene.close()
    hit = want["depth"] > 0
    assert hit.sum() > 100 and (~hit).sum() > 100
    for name, magic, channels in (("albedo", "PF", 3), ("normal", "PF", 3), ("depth", "Pf", 1)):
        got = _read_pfm(f"{prefix}_{name}.pfm", magic, channels)
        assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name
    assert sorted(p.name for p in tmp_path.glob("g_*")) == ["g_albedo.pfm", "g_depth.pfm", "g_normal.pfm"]

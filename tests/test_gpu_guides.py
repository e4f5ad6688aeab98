"""rt_render_guides is a composition: every plane equals, bit for bit, what the four public calls answer for the camera rays through
the pixel centres -- rt_camera_rays, rt_query_closest, rt_query_surface, rt_query_environment, and one float32 product for the albedo.
That definition is the test; the pieces are pinned to the oracle in test_gpu_query.py and test_gpu_query_surface.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = sc.MISS
PLANES = ("albedo", "normal", "depth", "emission")


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = rt.Scene(sc.scene_data(name), **kw)
        return made[key]
    yield get
    for s in made.values():
        s.close()


def compose(scene, w, h):
    """The planes from the four public calls, and the hits they were made of."""
    o, d = scene.camera_rays(w, h, sc.centres(w, h))
    hits, _ = scene.query_closest(o, d)
    surf, _ = scene.query_surface(hits)
    env, _ = scene.query_environment(o, d)
    hit = hits["triangle"] != MISS
    zero = np.zeros((w * h, 3), np.float32)
    planes = {"albedo": np.where(hit[:, None], surf["base_color"] * surf["color"], env), "normal": np.where(hit[:, None], surf["sn"], zero),
              "depth": np.where(hit, hits["t"], np.float32(0)), "emission": np.where(hit[:, None], surf["emission"], zero)}
    assert all(p.dtype == np.float32 for p in planes.values())
    return {k: p.reshape((h, w) if k == "depth" else (h, w, 3)) for k, p in planes.items()}, hits


_composed = {}


def composed(scenes, name, w, h, **kw):
    key = (name, w, h, tuple(sorted(kw.items())))
    if key not in _composed:
        _composed[key] = compose(scenes(name, **kw), w, h)
    return _composed[key]


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("w,h", [(50, 30), (30, 50)])
@pytest.mark.parametrize("name", ["sphere_env", "soup_a_env"])
def test_guides_are_the_composition_of_the_public_calls(rt, scenes, monkeypatch, name, w, h, chunk):
    want, hits = composed(scenes, name, w, h)
    hit = hits["triangle"] != MISS
    assert hit.sum() > 100 and (~hit).sum() > 100
    if chunk:
        monkeypatch.setenv("RTAMD_QUERY_CHUNK", str(chunk))
    got, st = scenes(name).render_guides(w, h)
    chunks = -(-w * h // chunk) if chunk else 1
    print(f"{name} {w}x{h} chunk {chunk}: {st.launches} launches, {st.exact_walks} exact walks, {st.kernel_ms:.3f} ms")
    assert st.rays == w * h and st.invalid_rays == 0 and st.launches == chunks * 7 and st.reference_exact == 1
    for k in PLANES:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
        assert same_bits(got[k], want[k]), (k, np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))[:5])
    assert np.any(got["emission"]) == (name == "soup_a_env") and np.any(got["albedo"][~hit.reshape(h, w)])


def test_any_plane_may_be_left_out(rt, scenes):
    w, h = 50, 30
    scene = scenes("soup_a_env")
    want, _ = composed(scenes, "soup_a_env", w, h)
    for k in PLANES:
        alone, _ = scene.render_guides(w, h, **{p: p == k for p in PLANES})
        assert list(alone) == [k] and same_bits(alone[k], want[k])
        others, _ = scene.render_guides(w, h, **{p: p != k for p in PLANES})
        assert sorted(others) == sorted(p for p in PLANES if p != k) and all(same_bits(others[p], want[p]) for p in others)
    none, st = scene.render_guides(w, h, albedo=False, normal=False, depth=False, emission=False)
    assert none == {} and st.rays == w * h


def _tied_pixels(sd, o, d, hits):
    """Pixels whose closest hit has a second triangle at the same distance (relative 1e-5), by brute force in float64."""
    tri = sd.positions.reshape(-1, 3, 3).astype(np.float64)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    tied = np.zeros(len(o), bool)
    for i in np.nonzero(hits["triangle"] != MISS)[0]:
        oo, dd = o[i].astype(np.float64), d[i].astype(np.float64)
        p = np.cross(dd, e2)
        det = (e1 * p).sum(axis=1)
        with np.errstate(all="ignore"):
            s = oo - a
            u = (s * p).sum(axis=1) / det
            q = np.cross(s, e1)
            v = (q * dd).sum(axis=1) / det
            t = (q * e2).sum(axis=1) / det
        inside = (np.abs(det) > 0) & (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9)
        near = inside & (np.abs(t - float(hits["t"][i])) <= 1e-5 * float(hits["t"][i]))
        near[hits["triangle"][i]] = False
        tied[i] = near.any()
    return tied


def test_device_built_scene_gives_the_same_guides(rt, scenes):
    """RT_BUILD_DEVICE_BVH: the same depth everywhere; the other planes wherever both scenes name the same triangle (two triangles at
    the same t are told apart by index order, which differs), and that is at least 99 % of the hit pixels.  The oracle's closest hits at
    the pixel centres show, on the CPU, that ties are that rare on sphere.gltf; the soups are made with duplicated and coplanar
    triangles (a sixth of their hit pixels tie), so they are not used here."""
    import test_gpu_query as tq
    name, w, h = "sphere_env", 50, 30
    sd = sc.scene_data(name)
    xy = sc.centres(w, h)
    host = scenes(name)
    o, d = host.camera_rays(w, h, xy)
    want_hits = tq._expected_hits(sc.oracle(name), sd, o, d)
    tied = _tied_pixels(sd, o, d, want_hits)
    n_hit = int((want_hits["triangle"] != MISS).sum())
    print(f"{name}: {n_hit} hit pixels, {tied.sum()} tied")
    assert n_hit > 100 and tied.sum() < 0.01 * n_hit
    dev = scenes(name, build_flags=rt.RT_BUILD_DEVICE_BVH)
    assert dev.info().bvh_on_device == 1
    want, hits_host = composed(scenes, name, w, h)
    got, st = dev.render_guides(w, h)
    hits_dev, _ = dev.query_closest(o, d)
    assert st.reference_exact == 0
    assert same_bits(got["depth"], want["depth"])
    same = (hits_dev["triangle"] == hits_host["triangle"]).reshape(h, w)
    hit = (hits_host["triangle"] != MISS).reshape(h, w)
    assert (same & hit).sum() >= 0.99 * hit.sum()
    for k in ("albedo", "normal", "emission"):
        assert same_bits(got[k][same], want[k][same]), k


DEVICE_PLANES = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
scene = rt.Scene(sc.scene_data("soup_a_env"))
w, h = 50, 30
want, st = scene.render_guides(w, h)
planes = {{k: torch.full(want[k].shape, -1.0, dtype=torch.float32, device="cuda") for k in want}}
torch.cuda.synchronize()
st_d = scene.render_guides_device(w, h, *[planes[k].data_ptr() for k in ("albedo", "normal", "depth", "emission")])
assert st_d.rays == w * h and st_d.launches == st.launches and st_d.exact_walks == st.exact_walks
for k in want:
    assert np.array_equal(planes[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
depth = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
scene.render_guides_device(w, h, depth_ptr=depth.data_ptr())
assert np.array_equal(depth.cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))
print("DEVICE PLANES EQUAL")
"""


def test_device_pointer_planes_hold_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with torch tensors as planes.  In a process of its own, where torch opens the GPU before the library does."""
    r = subprocess.run([sys.executable, "-c", DEVICE_PLANES.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE PLANES EQUAL" in r.stdout, r.stdout + r.stderr

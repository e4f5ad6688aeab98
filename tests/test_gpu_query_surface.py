"""The first-hit layer on the GPU (rt_query_surface, rt_query_environment, rt_camera_rays) against the CPU oracle, bit for bit.

Surfaces: for the camera set (48x32) and the bounce set of test_gpu_query.py's recipe the GPU's own rt_hit records (that file pins them
to the oracle) go through rt_query_surface; every word of every rt_surface equals the record made of the oracle's texture taps
(rto_sample_texture at the hit's texcoord), tests/surface_model.py's normal map, alpha and emission, and the scene's own factors.
End to end, with nothing restated: the oracle's depth-1 render is the first hit's emission or the miss colour, per pixel.
Scenes: the three golden spheres and two soups whose textures are dealt by a fixed table (surface_cases.TABLES)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import pin_cases
import surface_cases as sc
import surface_model as sm
import test_gpu_query as tq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = sc.MISS
SURFACE_SCENES = ["sphere", "sphere_emissive", "sphere_roughness", "soup_a", "soup_b"]
NEW = ["rt_query_surface", "rt_query_environment", "rt_camera_rays", "rt_render_guides"]


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = rt.Scene(sc.scene_data(name))
        return made[name]
    yield get
    for s in made.values():
        s.close()


def _bounce_rays(o1, d1, hits):
    """test_gpu_query._rays(name, "bounce") from hits of the GPU's own: half random, half grazing into the surface."""
    on = hits["triangle"] != MISS
    ng = hits["ng"][on].astype(np.float64)
    x = (o1[on] + hits["t"][on, None] * d1[on] + np.float32(1e-4) * hits["ng"][on]).astype(np.float32)
    x, ng = x[:2048], ng[:2048]
    rng = np.random.default_rng(5)
    d = pin_cases.unit(rng.normal(0, 1, x.shape))
    half = len(x) // 2
    graze = tq._orthogonal(rng, ng[half:]) - rng.uniform(1e-4, 0.05, (len(x) - half, 1)) * ng[half:]
    d[half:] = pin_cases.unit(graze)
    return x, d


def _gpu_hits(scene, name):
    """The GPU's rt_hit records of the camera set and of the bounce set made from it."""
    o1, d1 = tq._camera_rays(sc.scene_data(name))
    cam, _ = scene.query_closest(o1, d1)
    ob, db = _bounce_rays(o1, d1, cam)
    bounce, _ = scene.query_closest(ob, db)
    return cam, bounce


def test_texture_tables_cover_every_kind():
    """On the CPU, before the GPU is touched: each kind on at least two of the six materials and absent on at least one, one material
    with all four, and the scenes really carry what the table says, with image sizes from 2x2 to 32x32."""
    for name, table in sc.TABLES.items():
        assert sc.table_is_fair(table), name
        sd = sc.scene_data(name)
        got = tuple(tuple(int(getattr(sd.materials[i], k) >= 0) for k in sc.KINDS) for i in range(6))
        assert got == table, (name, got)
        shapes = {im.shape[:2] for im in sd.images}
        assert (2, 2) in shapes and (32, 32) in shapes and all(2 <= s <= 32 for sh in shapes for s in sh)
        assert sd.texcoords.min() < -0.9 and sd.texcoords.max() > 1.9


@pytest.mark.parametrize("name", SURFACE_SCENES)
def test_surfaces_are_the_oracles_bits(rt, scenes, name):
    scene, sd = scenes(name), sc.scene_data(name)
    tap = sm.oracle_tap(sd)
    for which, hits in zip(("camera", "bounce"), _gpu_hits(scene, name)):
        got, st = scene.query_surface(hits)
        want = sm.expected_surfaces(rt, sd, hits, tap)
        n_hit = int((hits["triangle"] != MISS).sum())
        print(f"{name}/{which}: {len(hits)} records, {n_hit} hits, {st.launches} launches, {st.kernel_ms:.3f} ms")
        assert n_hit > 100 and st.rays == len(hits) and st.invalid_rays == 0 and st.exact_walks == 0 and st.reference_exact == 1
        assert np.array_equal(sc.words(got), sc.words(want)), sc.first_difference(sc.words(got), sc.words(want))
        assert np.all(got["material"][hits["triangle"] == MISS] == MISS)
        if name.startswith("soup"):
            assert len(np.unique(got["material"][hits["triangle"] != MISS])) == 6       # every row of the table was met


@pytest.mark.parametrize("w,h", [(24, 16), (16, 24)])
@pytest.mark.parametrize("name", ["sphere_emissive", "sphere_emissive_env", "soup_a"])
def test_depth_one_render_is_emission_or_environment(rt, scenes, name, w, h):
    """Hw8Oracle.render(W, H, 1, ray_depth=1) returns, per pixel, the first hit's emission or the miss colour of the camera ray that
    rto_hw8_trace_pixel reports: rt_query_closest, rt_query_surface and rt_query_environment must give those floats (-0 equals +0).
    Every frame holds both hits and misses, but one: sphere_emissive's camera sees nothing but geometry through the 16x24 frame (the
    oracle's own trace: 384 hits, 0 misses), so there the pixels that hit are all there is to compare; which pixels hit is the
    oracle's answer in every frame."""
    scene = scenes(name)
    o, d, oracle_hit = sc.traced_frame(name, w, h)
    ref, _, _ = sc.oracle(name).render(w, h, 1, ray_depth=1)
    ref = ref.reshape(-1, 3)
    hits, _ = scene.query_closest(o, d)
    surf, _ = scene.query_surface(hits)
    env, st = scene.query_environment(o, d)
    hit = hits["triangle"] != MISS
    print(f"{name} {w}x{h}: {hit.sum()} pixels hit, {(~hit).sum()} miss")
    assert np.array_equal(hit, oracle_hit) and st.invalid_rays == 0
    assert hit.any() and ((~hit).any() or (name.startswith("sphere_emissive") and (w, h) == (16, 24)))
    assert np.isfinite(ref).all()
    assert np.array_equal(surf["emission"][hit], ref[hit]), np.nonzero(np.any(surf["emission"] != ref, axis=1) & hit)[0][:8]
    assert np.array_equal(env[~hit], ref[~hit]), np.nonzero(np.any(env != ref, axis=1) & ~hit)[0][:8]
    if name == "soup_a":
        assert len(np.unique(ref[hit], axis=0)) > 10       # emissive texture taps among them


def _env_directions():
    d = pin_cases.env_uv_directions()
    edge = d[20000:]
    assert len(edge) < 2048
    return np.ascontiguousarray(np.concatenate([d[:2048 - len(edge)], edge]))


def test_environment_lookup_is_the_oracles_bits(rt, scenes):
    L = oracle_lib.lib()
    d = _env_directions()
    o = np.zeros_like(d)
    env = sc.env_map()
    uv = oracle_lib.env_uv(L, "rto_hw8_env_uv", d)
    want = np.zeros((len(d), 3), np.float32)
    for i in range(len(d)):
        L.rto_sample_texture(env.shape[1], env.shape[0], env.ctypes.data, float(uv[i, 0]), float(uv[i, 1]), 1, want[i].ctypes.data)
    got, st = scenes("sphere_emissive_env").query_environment(o, d)
    assert len(d) == 2048 and st.rays == 2048 and st.invalid_rays == 0 and st.launches == 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), sc.first_difference(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(got, axis=0)) > 500


def test_without_a_map_the_background_answers_and_invalid_rays_answer_zero(rt, scenes):
    d = _env_directions()[:512].copy()
    o = np.zeros_like(d)
    bad = np.arange(5, 512, 11)
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        c = k % 7
        if c == 6:
            d[i] = 0
        else:
            (o if c < 3 else d)[i, c % 3] = poison[(k // 7) % 3]
    valid = np.ones(512, bool)
    valid[bad] = False
    for name in ("soup_a", "soup_a_env"):
        got, st = scenes(name).query_environment(o, d)
        assert st.invalid_rays == len(bad) and st.rays == 512
        assert np.all(got[~valid].view(np.uint32) == 0)
        if name == "soup_a":
            assert np.all(got[valid].view(np.uint32) == np.float32(sc.scene_data(name).bg).view(np.uint32))
        else:
            clean, _ = scenes(name).query_environment(np.zeros_like(d[valid]), d[valid])
            assert np.array_equal(got[valid].view(np.uint32), clean.view(np.uint32))


@pytest.mark.parametrize("w,h", [(24, 16), (16, 24), (1, 1)])
def test_camera_rays_are_the_renderers(rt, scenes, w, h):
    """nx = x + u1, ny = y + u2 with the two draws the renderer makes first: the ray of the oracle's first query of that pixel."""
    o, d = scenes("sphere_emissive").camera_rays(w, h, sc.jitter(w, h))
    want_o, want_d, _ = sc.traced_frame("sphere_emissive", w, h)
    assert np.array_equal(o.view(np.uint32), want_o.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), sc.first_difference(d.view(np.uint32), want_d.view(np.uint32))


def test_camera_rays_refuse_bad_frames_and_points(rt, scenes):
    scene = scenes("sphere_emissive")
    for w, h in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(rt.RtError) as e:
            scene.camera_rays(w, h, np.zeros((1, 2), np.float32))
        assert e.value.code == rt.RT_ERR_INVALID_ARG and str(e.value).find("rt_camera_rays: ") >= 0
    for v in (np.nan, np.inf, -np.inf):
        xy = sc.centres(4, 4)
        xy[7, 1] = v
        with pytest.raises(rt.RtError) as e:
            scene.camera_rays(4, 4, xy)
        assert e.value.code == rt.RT_ERR_INVALID_ARG and "rt_camera_rays: " in str(e.value)
    o, d = scene.camera_rays(4, 4, np.zeros((0, 2), np.float32))
    assert o.shape == (0, 3)


def _poisoned(rt, hits, n_tris):
    """hits with bad records placed among the valid ones: (records, indices of misses, of out-of-range triangles, of non-finite ones)."""
    h = hits.copy()
    blank = np.zeros(1, rt.HIT_DTYPE)
    blank["triangle"] = MISS
    miss = np.arange(2, len(h), 29)
    h[miss] = blank
    h["flags"][miss[::2]] = rt.RT_HIT_INVALID_RAY
    h["texcoord"][miss[1::4]] = np.nan                    # a miss is a miss whatever else its record holds
    beyond = np.arange(7, len(h), 31)
    h["triangle"][beyond[0::2]] = n_tris
    h["triangle"][beyond[1::2]] = 0xFFFFFFFE
    nonfinite = np.arange(11, len(h), 13)
    nonfinite = nonfinite[~np.isin(nonfinite, np.concatenate([miss, beyond]))]
    fields = [("texcoord", 0), ("texcoord", 1), ("ns", 0), ("ns", 1), ("ns", 2), ("tangent", 0), ("tangent", 1), ("tangent", 2), ("tangent", 3)]
    for k, i in enumerate(nonfinite):
        f, c = fields[k % 9]
        h[f][i, c] = [np.nan, np.inf, -np.inf][(k // 9) % 3]
    assert len(nonfinite) >= 27
    return h, miss, beyond, nonfinite


@pytest.mark.parametrize("name", ["sphere", "soup_a"])
def test_bad_records_are_never_read_through(rt, scenes, name):
    scene = scenes(name)
    cam, bounce = _gpu_hits(scene, name)
    hits = np.concatenate([bounce[bounce["triangle"] != MISS], cam[cam["triangle"] != MISS]])[:600]
    clean, _ = scene.query_surface(hits)
    bad, miss, beyond, nonfinite = _poisoned(rt, hits, scene.info().n_triangles)
    got, st = scene.query_surface(bad)
    off = np.concatenate([miss, beyond, nonfinite])
    valid = np.ones(len(hits), bool)
    valid[off] = False
    assert st.invalid_rays == len(beyond) + len(nonfinite) and st.rays == len(hits)
    blank = np.zeros(16, np.uint32)
    blank[11] = MISS
    assert np.all(sc.words(got[off]) == blank)
    assert np.array_equal(sc.words(got[valid]), sc.words(clean[valid])) and len(hits) == 600 and valid.sum() > 400


def test_no_records_is_ok_without_a_launch(rt, scenes):
    scene = scenes("sphere")
    got, st = scene.query_surface(np.zeros(0, rt.HIT_DTYPE))
    assert got.shape == (0,) and (st.rays, st.launches, st.invalid_rays, st.kernel_ms) == (0, 0, 0, 0.0)
    got, st = scene.query_environment(np.zeros((0, 3)), np.zeros((0, 3)))
    assert got.shape == (0, 3) and st.launches == 0
    for fn in ("rt_query_surface", "rt_query_environment"):
        assert getattr(rt.lib, fn)(scene._h, None, 0, 0, None, None) == rt.RT_OK


def test_chunk_seams_change_no_answer(rt, scenes, monkeypatch):
    """RTAMD_QUERY_CHUNK=64 (it shrinks the chunk, never an answer): the bits of the unchunked calls, one launch per chunk."""
    scene = scenes("soup_a")
    cam, bounce = _gpu_hits(scene, "soup_a")
    hits = np.concatenate([cam[:301], bounce[:300]])
    o, d = tq._camera_rays(sc.scene_data("soup_a"))
    xy = sc.jitter(24, 16)
    surf, st = scene.query_surface(hits)
    env, st_e = scenes("soup_a_env").query_environment(o[:333], d[:333])
    rays = scene.camera_rays(24, 16, xy)
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "64")
    surf_c, st_c = scene.query_surface(hits)
    env_c, st_ec = scenes("soup_a_env").query_environment(o[:333], d[:333])
    rays_c = scene.camera_rays(24, 16, xy)
    assert st.launches == 1 and st_c.launches == -(-len(hits) // 64) and st_ec.launches == -(-333 // 64) and st_c.rays == len(hits)
    assert np.array_equal(sc.words(surf_c), sc.words(surf)) and np.array_equal(env_c.view(np.uint32), env.view(np.uint32))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rays_c, rays))


DEVICE_POINTERS = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
import test_gpu_query as tq
scene = rt.Scene(sc.scene_data("soup_a_env"))
o, d = tq._camera_rays(sc.scene_data("soup_a_env"))
n = len(o)
hits, _ = scene.query_closest(o, d)
surf, st = scene.query_surface(hits)
env, _ = scene.query_environment(o, d)
xy = sc.jitter(24, 16)
co, cd = scene.camera_rays(24, 16, xy)
dev = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1, cols).copy()).cuda()
d_hits, d_rays, d_xy = dev(hits, 16), dev(rt.pack_rays(o, d), 6), dev(xy, 2)
d_surf = torch.full((n, 16), -1.0, dtype=torch.float32, device="cuda")
d_env = torch.full((n, 3), -1.0, dtype=torch.float32, device="cuda")
d_cam = torch.full((len(xy), 6), -1.0, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
st_d = scene.query_surface_device(d_hits.data_ptr(), n, d_surf.data_ptr())
scene.query_environment_device(d_rays.data_ptr(), n, d_env.data_ptr())
scene.camera_rays_device(24, 16, d_xy.data_ptr(), len(xy), d_cam.data_ptr())
assert st_d.rays == n and st_d.launches == st.launches
assert np.array_equal(d_surf.cpu().numpy().view(np.uint32), surf.view(np.uint32).reshape(-1, 16))
assert np.array_equal(d_env.cpu().numpy().view(np.uint32), env.view(np.uint32))
assert np.array_equal(d_cam.cpu().numpy().view(np.uint32), np.concatenate([co, cd], axis=1).view(np.uint32))
# a non-finite point in a device array comes out as a NaN direction, which the queries answer as an invalid ray
d_xy[5, 0] = float("inf")
torch.cuda.synchronize()
scene.camera_rays_device(24, 16, d_xy.data_ptr(), len(xy), d_cam.data_ptr())
bad = d_cam.cpu().numpy()
assert np.isnan(bad[5, 3:]).all() and np.isfinite(np.delete(bad, 5, axis=0)).all()
st_b = scene.query_closest_device(d_cam.data_ptr(), len(xy), d_surf.data_ptr())
assert st_b.invalid_rays == 1
for off_in, off_out in ((4, 0), (0, 8)):
    code = rt.lib.rt_query_surface(scene._h, d_hits.data_ptr() + off_in, 1, rt.RT_QUERY_DEVICE_POINTERS, d_surf.data_ptr() + off_out, None)
    msg = rt.lib.rt_last_error().decode()
    assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_query_surface: ") and "16-byte aligned" in msg, (code, msg)
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with torch tensors in and out: the host path's bits; a misaligned array is refused.  In a process of its
    own, where torch opens the GPU before the library does (the order bench.py keeps)."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def _raw(rt, fn, scene, n=4, flags=0, first=True, out=True, stats=None, size=(8, 8)):
    """One raw call with four good records; returns (code, message)."""
    h = scene._h if scene is not None else None
    st = C.byref(stats) if stats is not None else None
    rays = rt.pack_rays(np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1)))
    hits = np.zeros(4, rt.HIT_DTYPE)
    hits["triangle"] = MISS
    buf = np.zeros(4 * 16, np.uint32)
    if fn == "rt_query_surface":
        code = rt.lib.rt_query_surface(h, hits.ctypes.data if first else None, n, flags, buf.ctypes.data if out else None, st)
    elif fn == "rt_query_environment":
        code = rt.lib.rt_query_environment(h, rays.ctypes.data if first else None, n, flags, buf.ctypes.data if out else None, st)
    elif fn == "rt_camera_rays":
        xy = sc.centres(2, 2)
        code = rt.lib.rt_camera_rays(h, size[0], size[1], xy.ctypes.data if first else None, n, flags, buf.ctypes.data if out else None)
    else:
        planes = np.zeros((4, max(1, size[0] * size[1] * 3)), np.float32)
        code = rt.lib.rt_render_guides(h, size[0], size[1], flags, *[p.ctypes.data for p in planes], st)
    return code, rt.lib.rt_last_error().decode()


def _stats(rt, struct_size=None):
    st = rt.rt_query_stats()
    st.struct_size = C.sizeof(st) if struct_size is None else struct_size
    return st


@pytest.mark.parametrize("fn", NEW)
def test_hw6_and_txt_scenes_are_unsupported(rt, fn):
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    sd, *_ = rt.load_txt(os.path.join(pin_cases.SCENES, "txt", "hw1_sample.txt"), rt.RT_INTEGRATOR_HW1)
    txt = rt.Scene(sd)
    try:
        for scene in (hw6, txt):
            code, msg = _raw(rt, fn, scene)
            assert code == rt.RT_ERR_UNSUPPORTED and msg.startswith(fn + ": ") and "hw8 / hw7" in msg, (code, msg)
    finally:
        hw6.close()
        txt.close()


@pytest.mark.parametrize("fn", NEW)
def test_bad_arguments(rt, scenes, fn):
    sphere = scenes("sphere_emissive")
    code, msg = _raw(rt, fn, None)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"
    if fn != "rt_render_guides":                                  # its planes are all nullable
        for kw in ({"first": False}, {"out": False}):
            code, msg = _raw(rt, fn, sphere, **kw)
            assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument", (kw, code, msg)
    for flags in (2, 4, 8, 0x80000000, 1 | 16):                   # RT_QUERY_REFERENCE_WALK is not theirs either
        code, msg = _raw(rt, fn, sphere, flags=flags)
        assert code == rt.RT_ERR_INVALID_ARG and msg.startswith(fn + ": flags other than RT_QUERY_DEVICE_POINTERS"), (flags, code, msg)
    if fn != "rt_camera_rays":                                    # it takes no stats
        for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
            code, msg = _raw(rt, fn, sphere, stats=_stats(rt, size))
            assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": struct_size mismatch (ABI skew)", (size, code, msg)
    if fn in ("rt_camera_rays", "rt_render_guides"):
        for size in ((0, 8), (8, 0), (-3, 8)):
            code, msg = _raw(rt, fn, sphere, size=size)
            assert code == rt.RT_ERR_INVALID_ARG and msg.startswith(fn + ": width and height"), (size, code, msg)
    st = _stats(rt)
    code, msg = _raw(rt, fn, sphere, stats=st)
    assert code == rt.RT_OK, msg
    if fn != "rt_camera_rays":
        assert st.rays == (64 if fn == "rt_render_guides" else 4) and st.launches > 0


def test_nothing_else_moved(rt):
    """The first surface query leaves rt_scene_info.device_bytes alone, and a render after the queries equals the one before."""
    sd = sc.scene_data("soup_a_env")
    scene = rt.Scene(sd)
    try:
        before_bytes = scene.info().device_bytes
        before, before8, _ = scene.render(32, 24, 3)
        o, d = tq._camera_rays(sd)
        hits, _ = scene.query_closest(o, d)
        scene.query_surface(hits)
        scene.query_environment(o, d)
        scene.camera_rays(8, 8, sc.centres(8, 8))
        scene.render_guides(20, 12)
        assert scene.info().device_bytes == before_bytes
        after, after8, _ = scene.render(32, 24, 3)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and np.array_equal(before8, after8)
    finally:
        scene.close()

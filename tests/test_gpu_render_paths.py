"""rt_render_paths and rt_render_bake on the GPU against their referees, rt_trace_paths and rt_bake (RT_BAKE_IRRADIANCE): the same
32-bit words in the answer and in the engines, on scenes whose renders report reference_exact = 1.

Scenes, rays, engines and points are test_gpu_bake.py's and test_gpu_scatter.py's: the 48x32 jittered camera set and its first-bounce
rays (the scatter's (o, d) of the hits), engines seeded 1 + 7919 * j, points at the GPU's closest hits (at most 256), SAMPLES = 8,
DEPTH = 4, K in {1, 4}."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pin_cases
import scatter_model as model
import surface_cases as sc
import test_gpu_bake as tb
import test_gpu_query as tq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MISS = sc.MISS
SAMPLES, DEPTH = tb.SAMPLES, tb.DEPTH
SCENES = ["soup_a", "soup_b", "sphere_emissive_env", "sphere_emissive"]
BAKE_CASES = [(name, K) for name, mode, K in tb.CASES if mode == tb.bm.IRRADIANCE]

scenes = tb.scenes
_engines, _words, _same = tb._engines, tb._words, tb._same


_RAYS = {}


def _rays(scene, name):
    """The camera set and the first-bounce rays of its hits, with their engines (seeded 1 + 7919 * j): camera and surface origins.  Made
    once per scene.  Where the referee returns no radiance for half of them or more (a black background), rays without radiance are
    left out, evenly, until three of seven are left: a path depends on its ray and its engine alone, so the others' paths stay.
    Returns (o, d, rays from the camera among them, engines)."""
    if name not in _RAYS:
        o, d = tq._camera_rays(sc.scene_data(name))
        hits, _ = scene.query_closest(o, d)
        on = hits["triangle"] != MISS
        surf, _ = scene.query_surface(np.ascontiguousarray(hits[on]))
        scat, _ = scene.query_scatter(np.ascontiguousarray(o[on]), np.ascontiguousarray(d[on]), np.ascontiguousarray(hits[on]), surf,
                                      model.seed(5 + 104729 * np.arange(int(on.sum()))))
        go = scat["flags"] == 0
        o2 = np.concatenate([o, scat["o"][go]]).astype(F)
        d2 = np.concatenate([d, scat["d"][go]]).astype(F)
        from_camera = np.arange(len(o2)) < len(o)
        rng = _engines(len(o2))
        ref, _ = scene.trace_paths(o2, d2, rng.copy(), ray_depth=DEPTH)
        lit = ref.view(np.uint32).any(axis=1)
        if 2 * lit.sum() <= len(o2):
            dark = np.nonzero(~lit)[0]
            keep = lit.copy()
            keep[dark[np.linspace(0, len(dark) - 1, 3 * int(lit.sum()) // 4).astype(int)]] = True
            o2, d2, from_camera, rng = o2[keep], d2[keep], from_camera[keep], rng[keep]
        o2, d2, rng = np.ascontiguousarray(o2), np.ascontiguousarray(d2), np.ascontiguousarray(rng)
        for a in (o2, d2, rng):
            a.setflags(write=False)
        _RAYS[name] = (o2, d2, int(from_camera.sum()), rng)
    return _RAYS[name]


def _endings(scene, o, d, rng, depth):
    """How each path of rt_trace_paths ends, by the single calls it is a composition of: 0 miss, 1 END_BRDF / END_CLAMP, 2 depth spent."""
    n = len(o)
    o, d = np.array(o, F), np.array(d, F)
    end = np.full(n, 2)
    live = np.arange(n)
    for _ in range(depth):
        hits, _ = scene.query_closest(o[live], d[live])
        miss = hits["triangle"] == MISS
        end[live[miss]] = 0
        live, hits = live[~miss], np.ascontiguousarray(hits[~miss])
        if not len(live):
            break
        surf, _ = scene.query_surface(hits)
        engines = np.ascontiguousarray(rng[live])
        scat, _ = scene.query_scatter(np.ascontiguousarray(o[live]), np.ascontiguousarray(d[live]), hits, surf, engines)
        rng[live] = engines
        ended = scat["flags"] != 0
        end[live[ended]] = 1
        live, scat = live[~ended], scat[~ended]
        o[live], d[live] = scat["o"], scat["d"]
    return end


def _equal_calls(scene, o, d, rng, depth):
    """Both calls on copies of the engines; asserts equality; returns the referee's answer and both stats."""
    ref_rng, got_rng = rng.copy(), rng.copy()
    ref, st_r = scene.trace_paths(o, d, ref_rng, ray_depth=depth)
    got, st = scene.render_paths(o, d, got_rng, ray_depth=depth)
    assert _same(got, ref), sc.first_difference(_words(got), _words(ref))
    assert _same(got_rng, ref_rng), sc.first_difference(_words(got_rng), _words(ref_rng))
    assert (st.rays, st.invalid_rays, st.reference_exact) == (len(o), st_r.invalid_rays, 1) and st_r.reference_exact == 1
    return ref, st_r, st


@pytest.mark.parametrize("depth", [DEPTH, 0])
@pytest.mark.parametrize("name", SCENES)
def test_render_paths_are_trace_paths_bits(rt, scenes, name, depth):
    scene = scenes(name)
    o, d, n_cam, rng = _rays(scene, name)
    n = len(o)
    assert n_cam > 32 and n - n_cam > 32                     # camera and surface origins occur
    ref, st_r, st = _equal_calls(scene, o, d, rng, depth)
    # the conditions on the inputs, on the referee's answer
    nonzero = int(ref.view(np.uint32).any(axis=1).sum())
    ends = np.bincount(_endings(scene, o, d, rng.copy(), depth or 6), minlength=3)
    print(f"{name} depth {depth}: {n} rays, {nonzero} with radiance, ends miss / END_* / depth {ends.tolist()}, launches {st.launches} against {st_r.launches}, "
          f"exact walks {st.exact_walks} against {st_r.exact_walks}")
    assert nonzero > n // 2 and (ends > 0).all(), (nonzero, ends)
    assert st.launches < st_r.launches
    # engines that enter with has_saved = 1, made by one rt_bake_rays call
    saved = _engines(n)
    scene.bake_rays(rt.pack_bake_points(np.zeros((n, 3), F), np.tile(np.array([0, 1, 0], F), (n, 1))), saved)
    assert saved["has_saved"].all()
    _equal_calls(scene, o, d, saved, depth)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1536])
def test_sizes_at_the_kernels_edges(rt, scenes, n):
    """64-slot groups, 256-thread workgroups, more groups than one workgroup holds."""
    scene = scenes("soup_a")
    o, d, _, _ = _rays(scene, "soup_a")
    pick = np.arange(n) * (len(o) // n)                      # camera and surface origins at every size
    _equal_calls(scene, np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick]), _engines(n), DEPTH)


@pytest.mark.parametrize("name", ["soup_a", "sphere_emissive_env"])
def test_the_frame_identity(rt, scenes, name):
    """Per pixel rt_rng_seed(y * W + x), two rt_rng_uniform, rt_camera_rays, rt_render_paths: rt_render(samples = 1)'s linear floats."""
    w, h = 48, 32
    scene = scenes(name)
    rng = rt.rng_seed(np.arange(w * h))
    px, py = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    xy = np.stack([px.reshape(-1) + rt.rng_uniform(rng), py.reshape(-1) + rt.rng_uniform(rng)], axis=1).astype(F)
    o, d = scene.camera_rays(w, h, xy)
    got, st = scene.render_paths(o, d, rng)
    want, _, _ = scene.render(w, h, 1)
    assert st.invalid_rays == 0 and st.reference_exact == 1
    a, b = got.reshape(-1, 3).view(np.uint32), (F(1.0) * want).reshape(-1, 3).view(np.uint32)
    assert np.array_equal(a, b), sc.first_difference(a, b)
    assert len(np.unique(a, axis=0)) > 32


def test_first_rays_off_the_fast_list(rt, scenes):
    """Origins above the scene's box looking in, an origin beyond origin_bound, a direction with an exact zero component, |d| = 1e-3
    and 100: the referee's bits, and every one of them walked by the exact role."""
    scene, sd = scenes("soup_a"), sc.scene_data("soup_a")
    pts = np.concatenate([sd.positions.reshape(-1, 3), np.array([sd.camera.position], F)])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext = float((hi - lo).max())
    o, d, _, _ = _rays(scene, "soup_a")
    hits, _ = scene.query_closest(o[:256], d[:256])
    on = hits["triangle"] != MISS
    target = (o[:256][on] + hits["t"][on][:, None] * d[:256][on]).astype(F)[:64]
    assert len(target) == 64
    rays_o, rays_d = [], []
    above = target.copy()
    above[:, 1] = hi[1] + F(0.5) * F(ext)                    # above the box (and the grid over it), within max |coordinate| or not
    rays_o.append(above[:16]); rays_d.append((target[:16] - above[:16]) / np.linalg.norm(target[:16] - above[:16], axis=1, keepdims=True))
    far = target[16:32] + F(64.0 * max(ext, float(np.abs(pts).max()))) * np.array([0.6, 0.0, 0.8], F)   # beyond origin_bound
    rays_o.append(far); rays_d.append((target[16:32] - far) / np.linalg.norm(target[16:32] - far, axis=1, keepdims=True))
    zero = d[32:48].copy()
    zero[:, 0] = 0                                           # an exact zero component
    rays_o.append(o[32:48]); rays_d.append(zero)
    rays_o.append(o[48:56]); rays_d.append(d[48:56] * F(1e-3))
    rays_o.append(o[56:64]); rays_d.append(d[56:64] * F(100))
    o2, d2 = np.ascontiguousarray(np.concatenate(rays_o).astype(F)), np.ascontiguousarray(np.concatenate(rays_d).astype(F))
    n = len(o2)
    assert n == 64 and np.isfinite(o2).all() and np.isfinite(d2).all()
    ref, st_r, st = _equal_calls(scene, o2, d2, _engines(n), DEPTH)
    print(f"off the fast list: {n} rays, exact walks {st.exact_walks} against {st_r.exact_walks}, {int(ref.any(axis=1).sum())} with radiance")
    assert st.exact_walks >= n and st.invalid_rays == 0
    assert ref.any(axis=1).sum() > 8                         # they see the scene


POISONED = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import scatter_model as model
import surface_cases as sc
import test_gpu_bake as tb
import test_gpu_query as tq
scene = rt.Scene(sc.scene_data("soup_a"))
dev = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()   # words, not floats: no copy may touch a NaN
host = lambda t: t.cpu().numpy().view(np.uint32)
o, d = tq._camera_rays(sc.scene_data("soup_a"))
n = 300
o, d = np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])
rng = model.seed(1 + 7919 * np.arange(n))
L, st = scene.render_paths(o, d, rng.copy())
ref, st_r = scene.trace_paths(o, d, rng.copy())
assert np.array_equal(L.view(np.uint32), ref.view(np.uint32))
# device pointers give the host arrays' bytes
d_rays, d_rng = dev(rt.pack_rays(o, d), 6), dev(rng, 4)
d_L = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_d = scene.render_paths_device(d_rays.data_ptr(), d_rng.data_ptr(), n, d_L.data_ptr())
after = rng.copy()
scene.render_paths(o, d, after)
assert (st_d.rays, st_d.invalid_rays, st_d.exact_walks, st_d.launches) == (n, 0, st.exact_walks, st.launches)
assert np.array_equal(host(d_L), L.view(np.uint32)) and np.array_equal(host(d_rng), after.view(np.uint32).reshape(-1, 4))
assert np.array_equal(host(d_rays), rt.pack_rays(o, d).view(np.uint32).reshape(-1, 6))
code = rt.lib.rt_render_paths(scene._h, d_rays.data_ptr(), d_rng.data_ptr() + 8, 1, 0, rt.RT_QUERY_DEVICE_POINTERS, d_L.data_ptr(), None)
msg = rt.lib.rt_last_error().decode()
assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_render_paths: ") and "16-byte aligned" in msg, (code, msg)
# from device memory an engine of 0 and of 2^31 - 1: zeros, the engine bytes untouched, counted
bad = rng.copy()
bad["x"][7], bad["x"][130] = 0, 2**31 - 1
bad["saved"][7], bad["reserved"][130] = 5.0, 77
d_bad = dev(bad, 4)
d_L2 = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_b = scene.render_paths_device(d_rays.data_ptr(), d_bad.data_ptr(), n, d_L2.data_ptr())
got, got_rng = host(d_L2), host(d_bad)
assert st_b.invalid_rays == 2 and not got[[7, 130]].any()
assert np.array_equal(got_rng[[7, 130]], bad.view(np.uint32).reshape(-1, 4)[[7, 130]])
good = np.ones(n, bool); good[[7, 130]] = False
assert np.array_equal(got[good], L.view(np.uint32)[good]) and np.array_equal(got_rng[good], after.view(np.uint32).reshape(-1, 4)[good])
# the bake: device pointers give the host arrays' bytes
points = tb._points(rt, scene, "soup_a")[:100]
K = 4
brng = model.seed(1 + 7919 * np.arange(len(points) * K))
want_rng = brng.copy()
want, st_w = scene.render_bake(points, want_rng, tb.SAMPLES, K, ray_depth=tb.DEPTH)
d_pts, d_brng = dev(points, 6), dev(brng, 4)
d_out = torch.full((len(points), 3), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_bd = scene.render_bake_device(d_pts.data_ptr(), d_brng.data_ptr(), len(points), d_out.data_ptr(), tb.SAMPLES, K, ray_depth=tb.DEPTH)
assert (st_bd.points, st_bd.invalid_points, st_bd.paths, st_bd.launches) == (len(points), 0, st_w.paths, st_w.launches)
assert np.array_equal(host(d_out), want.view(np.uint32)) and np.array_equal(host(d_brng), want_rng.view(np.uint32).reshape(-1, 4))
# one bad engine among a point's K, from device memory: the point answers zeros, keeps all its engines, is counted once
bad = brng.copy()
bad["x"][11 * K + 3] = 2**31 - 1
d_bad = dev(bad, 4)
d_out2 = torch.full((len(points), 3), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_bb = scene.render_bake_device(d_pts.data_ptr(), d_bad.data_ptr(), len(points), d_out2.data_ptr(), tb.SAMPLES, K, ray_depth=tb.DEPTH)
got, got_rng = host(d_out2), host(d_bad)
assert st_bb.invalid_points == 1 and st_bb.paths == st_w.paths - tb.SAMPLES and not got[11].any()
own = slice(11 * K, 12 * K)
assert np.array_equal(got_rng[own], bad.view(np.uint32).reshape(-1, 4)[own])
good = np.ones(len(points), bool); good[11] = False
assert np.array_equal(got[good], want.view(np.uint32)[good]) and np.array_equal(got_rng[np.repeat(good, K)], want_rng.view(np.uint32).reshape(-1, 4)[np.repeat(good, K)])
ref_out = torch.full((len(points), 3), -1, dtype=torch.int32, device="cuda")
d_bad2 = dev(bad, 4)
torch.cuda.synchronize()
st_ref = scene.bake_device(d_pts.data_ptr(), d_bad2.data_ptr(), len(points), ref_out.data_ptr(), tb.SAMPLES, K, ray_depth=tb.DEPTH)
assert st_ref.invalid_points == 1 and np.array_equal(host(ref_out), got) and np.array_equal(host(d_bad2), got_rng)
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_and_bad_device_engines():
    """RT_QUERY_DEVICE_POINTERS with torch tensors for both calls: the host path's bytes, engines included; an engine of 0 and of 2^31-1
    in device memory answers zeros, keeps its bytes and is counted.  In a process of its own, where torch opens the GPU first."""
    r = subprocess.run([sys.executable, "-c", POISONED.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def test_invalid_records(rt, scenes):
    """NaN or inf in o or d, d == 0: zeros, the engine untouched, counted; a bad engine in a host array is refused with the record named."""
    scene = scenes("soup_a")
    o, d, _, _ = _rays(scene, "soup_a")
    n = 256
    pick = np.arange(n) * (len(o) // n)
    o, d = np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick])
    clean_rng = _engines(n)
    clean, _ = scene.render_paths(o, d, clean_rng, ray_depth=DEPTH)
    o2, d2 = o.copy(), d.copy()
    bad = np.arange(3, n, 17)
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        c = k % 7
        if c == 6:
            d2[i] = 0
        else:
            (o2 if c < 3 else d2)[i, c % 3] = poison[(k // 7) % 3]
    rng = _engines(n)
    rng["saved"][bad[0]] = 5.0                               # bytes that only an untouched engine keeps
    before = rng.copy()
    got, st = scene.render_paths(o2, d2, rng, ray_depth=DEPTH)
    ref_rng = before.copy()
    ref, st_r = scene.trace_paths(o2, d2, ref_rng, ray_depth=DEPTH)
    assert st.invalid_rays == st_r.invalid_rays == len(bad) and st.rays == n
    assert not got[bad].view(np.uint32).any() and np.array_equal(rng[bad], before[bad])
    assert _same(got, ref) and _same(rng, ref_rng)
    good = np.ones(n, bool)
    good[bad] = False
    assert _same(got[good], clean[good]) and np.array_equal(rng[good], clean_rng[good])
    for x in (0, 2**31 - 1):
        rng = _engines(n)
        rng["x"][41] = x
        before = rng.copy()
        out = np.full((n, 3), 7, F)
        st = rt.rt_query_stats()
        st.struct_size, st.launches = C.sizeof(st), 77
        code = rt.lib.rt_render_paths(scene._h, rt.pack_rays(o, d).ctypes.data, rng.ctypes.data, n, DEPTH, 0, out.ctypes.data, C.byref(st))
        msg = rt.lib.rt_last_error().decode()
        assert code == rt.RT_ERR_INVALID_ARG and msg == f"rt_render_paths: rng[41].x = {x} is no state of the engine (1 .. 2147483646)"
        assert st.launches == 77 and np.array_equal(rng, before) and (out == 7).all()
    e = np.zeros((0, 3), F)
    L, st = scene.render_paths(e, e, model.seed(np.arange(1))[:0].copy())
    assert L.shape == (0, 3) and (st.launches, st.rays) == (0, 0)
    assert rt.lib.rt_render_paths(scene._h, None, None, 0, 0, 0, None, None) == rt.RT_OK


@pytest.mark.parametrize("name,K", BAKE_CASES)
def test_render_bake_is_bakes_bits(rt, scenes, name, K):
    scene = scenes(name)
    points = tb._points(rt, scene, name)
    n = len(points)
    assert n > 32
    ref_rng, got_rng = _engines(n * K), _engines(n * K)
    q = SAMPLES // K
    for call in range(2):                                    # the second with the engines the first left
        ref, st_r = scene.bake(points, ref_rng, SAMPLES, K, tb.bm.IRRADIANCE, DEPTH)
        got, st = scene.render_bake(points, got_rng, SAMPLES, K, ray_depth=DEPTH)
        assert _same(got, ref), (call, sc.first_difference(_words(got), _words(ref)))
        assert _same(got_rng, ref_rng), (call, sc.first_difference(_words(got_rng), _words(ref_rng)))
        assert (st.points, st.invalid_points, st.paths, st.reference_exact) == (n, 0, n * K * q, 1) and st_r.paths == st.paths
        assert (st.rounds, st.ray_slots, st.live_ray_slots) == (0, 0, 0) and st.launches < st_r.launches
        assert np.isfinite(got).all() and len(np.unique(got, axis=0)) > n // 2
    print(f"{name} K {K}: {n} points, launches {st.launches} against {st_r.launches}, exact walks {st.exact_walks} against {st_r.exact_walks}")
    # invalid points: a NaN p, n == 0, one bad engine among a point's K
    pts, rng = points.copy(), _engines(n * K)
    pts["p"][5, 1] = np.nan
    pts["n"][9] = 0
    rng_bad = 11 * K + (K - 1)
    d_rng = rng.copy()
    d_rng["x"][rng_bad] = 0                                  # a host array is refused; device memory: test_device_pointers_and_bad_device_engines
    with pytest.raises(rt.RtError) as e:
        scene.render_bake(pts, d_rng.copy(), SAMPLES, K, ray_depth=DEPTH)
    assert e.value.code == rt.RT_ERR_INVALID_ARG and f"rt_render_bake: rng[{rng_bad}].x = 0" in str(e.value)
    before = rng.copy()
    got, st = scene.render_bake(pts, rng, SAMPLES, K, ray_depth=DEPTH)
    ref_rng = before.copy()
    ref, st_r = scene.bake(pts, ref_rng, SAMPLES, K, tb.bm.IRRADIANCE, DEPTH)
    assert st.invalid_points == st_r.invalid_points == 2 and st.paths == st_r.paths == (n - 2) * K * q
    assert not got[[5, 9]].view(np.uint32).any()
    slots = np.concatenate([np.arange(p * K, p * K + K) for p in (5, 9)])
    assert np.array_equal(rng[slots], before[slots])
    assert _same(got, ref) and _same(rng, ref_rng)



def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seam_case(rt, scene):
    """300 rays, and 100 points x K = 4 with one invalid point: the digests of both calls' outputs and engines, and their launches."""
    o, d = tq._camera_rays(sc.scene_data("soup_a"))
    r = _engines(300)
    L, st = scene.render_paths(o[:300], d[:300], r, ray_depth=DEPTH)
    points = tb._points(rt, scene, "soup_a")[:100].copy()
    points["n"][37] = 0
    b = _engines(400)
    out, st_b = scene.render_bake(points, b, SAMPLES, 4, ray_depth=DEPTH)
    assert st_b.invalid_points == 1
    return _digest(L, r, out, b), (st.launches, st_b.launches)


SEAMS = """
import importlib, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
import test_gpu_render_paths as t
scene = rt.Scene(sc.scene_data("soup_a"))
digest, launches = t._seam_case(rt, scene)
print("SEAMS", digest, *launches)
"""


def test_chunk_seams_change_no_answer(rt, scenes):
    """RTAMD_QUERY_CHUNK=128 in a fresh child process: three chunks for 300 rays, four for 100 points of 4 slots; the bytes of the one chunk here."""
    digest, launches = _seam_case(rt, scenes("soup_a"))
    env = dict(os.environ, RTAMD_QUERY_CHUNK="128")
    r = subprocess.run([sys.executable, "-c", SEAMS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SEAMS" in r.stdout, r.stdout + r.stderr
    got = r.stdout.split("SEAMS", 1)[1].split()
    assert got[0] == digest
    assert [int(v) for v in got[1:3]] == [3 * launches[0], 4 * launches[1]], (got, launches)


WAVEFRONT = """
import importlib, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import scatter_model as model
import surface_cases as sc
scene = rt.Scene(sc.scene_data("soup_a"))
o, d = np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1))
for call in (lambda: scene.render_paths(o, d, model.seed(1 + np.arange(4))),
             lambda: scene.render_bake(rt.pack_bake_points(o, -d), model.seed(1 + np.arange(4)), 2)):
    try:
        call()
        raise SystemExit("served")
    except rt.RtError as e:
        assert e.code == rt.RT_ERR_UNSUPPORTED and "no fallback" in str(e), str(e)
print("REFUSED")
"""


def test_nothing_else_moves_and_what_is_unsupported(rt, scenes):
    sd = sc.scene_data("soup_a")
    scene = rt.Scene(sd)
    try:
        first, _, _ = scene.render(24, 16, 2)
        acc = scene.accumulator(24, 16)
        acc.render(4)
        blob, bytes_before = acc.save(), scene.info().device_bytes
        o, d = tq._camera_rays(sd)
        scene.render_paths(o[:200], d[:200], _engines(200), ray_depth=DEPTH)
        scene.render_bake(tb._points(rt, scene, "soup_a")[:50], _engines(200), SAMPLES, 4, ray_depth=DEPTH)
        assert acc.save() == blob and scene.info().device_bytes == bytes_before
        acc.render(4)
        after, _ = acc.resolve()
        whole, _, _ = scene.render(24, 16, 8)
        assert np.array_equal(after.view(np.uint32), whole.view(np.uint32))
        again, _, _ = scene.render(24, 16, 2)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
        with pytest.raises(rt.RtError) as e:
            scene.render_bake(tb._points(rt, scene, "soup_a")[:8], _engines(8), 4, 1, mode=rt.RT_BAKE_SH9)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "rt_render_bake: RT_BAKE_SH9" in str(e.value) and "rt_bake" in str(e.value)
        for depth in (17, 1000):
            with pytest.raises(rt.RtError) as e:
                scene.render_paths(o[:8], d[:8], _engines(8), ray_depth=depth)
            assert e.value.code == rt.RT_ERR_LIMIT and "rt_render_paths: ray_depth above 16" in str(e.value)
    finally:
        scene.close()
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    try:
        o, d = np.zeros((4, 3), F), np.tile(np.array([0, 0, -1], F), (4, 1))
        for fn, call in (("rt_render_paths", lambda: hw6.render_paths(o, d, model.seed(1 + np.arange(4)))),
                         ("rt_render_bake", lambda: hw6.render_bake(rt.pack_bake_points(o, -d), model.seed(1 + np.arange(4)), 2))):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt.RT_ERR_UNSUPPORTED and f"{fn}: " in str(e.value) and "hw8 / hw7" in str(e.value)
    finally:
        hw6.close()
    env = dict(os.environ, RTAMD_KERNEL="wavefront")
    r = subprocess.run([sys.executable, "-c", WAVEFRONT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "REFUSED" in r.stdout, r.stdout + r.stderr

"""rt_render_probes on the GPU against its referee, rt_bake (RT_BAKE_SH9, itself pinned to tests/bake_model.py by tests/test_gpu_bake.py):
the same 27 coefficients per point and the same engines, word for word, from the persistent render kernel with the probe source
(device/rt_path_source.h, src_mode 3).  Every slot has two or more samples somewhere in each test (q >= 2): a slot's first direction is
overwritten when its next sample's ray is drawn, so a projection in the wrong place gives other bits.  The referee is always
scene.bake(..., bm.SH9, ...) on copies of the engines.  SAMPLES = 8, DEPTH = 4 (test_gpu_bake's)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bake_model as bm
import pin_cases
import scatter_model as model
import surface_cases as sc
import test_gpu_bake as tb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SAMPLES, DEPTH = tb.SAMPLES, tb.DEPTH
scenes = tb.scenes
_points, _engines, _same, _words = tb._points, tb._engines, tb._same, tb._words


def _equal_calls(scene, points, K, samples=SAMPLES, rng=None):
    """Referee and new call on copies of the same engines: asserts equal words, returns (out, engines after, new stats, referee's stats)."""
    n = len(points)
    start = _engines(n * K) if rng is None else rng
    ref_rng, got_rng = start.copy(), start.copy()
    ref, st_r = scene.bake(points, ref_rng, samples, K, bm.SH9, DEPTH)
    got, st = scene.render_probes(points, got_rng, samples, K, ray_depth=DEPTH)
    assert got.shape == (n, 9, 3) and got.dtype == F
    assert _same(got, ref), sc.first_difference(_words(got), _words(ref))
    assert _same(got_rng, ref_rng), sc.first_difference(_words(got_rng), _words(ref_rng))
    assert (st.points, st.invalid_points, st.paths) == (n, st_r.invalid_points, st_r.paths)
    assert (st.rounds, st.ray_slots, st.live_ray_slots) == (0, 0, 0)
    assert st.reference_exact == st_r.reference_exact == 1
    return ref, ref_rng, st, st_r


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", ["soup_a", "soup_b", "sphere_emissive_env"])
def test_render_probes_are_bakes_bits(rt, scenes, name, K):
    scene = scenes(name)
    points = _points(rt, scene, name)
    n, q = len(points), SAMPLES // K
    assert n > 32 and q >= 2
    rng = _engines(n * K)
    for call in range(2):                                    # the second with the engines the first left
        ref, rng, st, st_r = _equal_calls(scene, points, K, rng=rng)
        assert st.paths == n * K * q and st.launches < st_r.launches, (call, st.launches, st_r.launches)
        # the inputs exercise what is compared: finite, rows that differ, every band present
        assert np.isfinite(ref).all()
        assert len(np.unique(ref.reshape(n, 27), axis=0)) > n // 2
        assert all(np.any(ref[:, m, :] != 0) for m in range(9))
    print(f"{name} K {K}: {n} points, launches {st.launches} against {st_r.launches}, exact walks {st.exact_walks} against {st_r.exact_walks}")


@pytest.mark.parametrize("K,n,samples", [(1, 1, 8), (1, 63, 8), (1, 64, 8), (1, 65, 8), (1, 257, 8), (4, 16, 8), (4, 17, 8), (3, 22, 6),
                                         (64, 1, 64), (64, 3, 64), (64, 1, 128), (64, 3, 128)])
def test_sizes_at_the_kernels_edges(rt, scenes, K, n, samples):
    """Whole and broken 64-slot groups, one and several workgroups' worth, a point whose streams straddle a group (K = 3: point 21 has
    slots 63 .. 65), and the most streams a point can have with one and two samples each."""
    scene = scenes("soup_a")
    points = _points(rt, scene, "soup_a", limit=257)[:n]
    assert len(points) == n
    ref, _, st, _ = _equal_calls(scene, points, K, samples)
    assert st.paths == n * samples and st.invalid_points == 0 and ref.any()


def test_probes_off_the_surfaces(rt, scenes):
    """A probe's ray starts at p itself and p may lie anywhere: the surface points lifted by a quarter of the scene's extent along ng, the
    box centre, and 16 points above the scene's box and the node grid over it, all of whose samples are the exact role's."""
    scene, sd = scenes("soup_a"), sc.scene_data("soup_a")
    xyz = np.concatenate([np.asarray(sd.positions, F).reshape(-1, 3), np.array([sd.camera.position], F)])
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    ext = F((hi - lo).max())
    on = _points(rt, scene, "soup_a", limit=64)
    lifted = (on["p"] + F(0.25) * ext * on["n"]).astype(F)
    centre = ((lo + hi) * F(0.5)).astype(F)[None, :]
    above = on["p"][:16].copy()
    above[:, 1] = hi[1] + F(0.5) * ext
    for what, p, floor in (("lifted", lifted, 0), ("centre", centre, 0), ("above", above, 16 * SAMPLES)):
        points = rt.pack_bake_points(np.ascontiguousarray(p), np.zeros_like(p))                  # n == 0: not read
        for K in (1, 4):
            ref, _, st, st_r = _equal_calls(scene, points, K)
            assert st.invalid_points == 0 and st.exact_walks >= floor, (what, K, st.exact_walks)
            print(f"{what} K {K}: {len(p)} probes, exact walks {st.exact_walks} against {st_r.exact_walks}, band 0 non-zero for {int(ref[:, 0, :].any(axis=1).sum())}")
            if what == "lifted":
                assert ref[:, 0, :].any(axis=1).sum() > 8    # they see the scene
    both = rt.pack_bake_points(np.concatenate([lifted, centre, above]), np.zeros((len(lifted) + 17, 3), F))
    ref, _, st, _ = _equal_calls(scene, both, 4)
    assert ref[:, 0, :].any(axis=1).sum() > 8 and st.exact_walks >= 16 * SAMPLES


def test_invalid_points(rt, scenes):
    """A NaN or an infinity in p: 27 zeros, all K engines kept, counted once.  n is not read: n == 0 and a NaN n are served as the clean
    point is.  One bad engine among a point's K in a host array is refused with the record named, and nothing is written."""
    scene, K = scenes("soup_a"), 4
    points = _points(rt, scene, "soup_a")[:64]
    n = len(points)
    clean, clean_rng, _, _ = _equal_calls(scene, points, K)
    pts = points.copy()
    pts["p"][5, 1] = np.nan
    pts["p"][20, 0] = np.inf
    pts["p"][21, 2] = -np.inf
    pts["n"][9] = 0
    pts["n"][30] = np.nan
    rng = _engines(n * K)
    rng["saved"][5 * K + 1] = 5.0                             # bytes that only an untouched engine keeps
    before = rng.copy()
    ref, after, st, st_r = _equal_calls(scene, pts, K, rng=rng)
    bad = [5, 20, 21]
    assert st.invalid_points == st_r.invalid_points == 3 and st.paths == (n - 3) * SAMPLES
    assert not ref[bad].view(np.uint32).any()
    slots = np.concatenate([np.arange(p * K, p * K + K) for p in bad])
    assert np.array_equal(after[slots], before[slots])
    good = np.ones(n, bool)
    good[bad] = False
    assert _same(ref[good], clean[good]) and np.array_equal(after[np.repeat(good, K)], clean_rng[np.repeat(good, K)])
    assert good[[9, 30]].all()                               # n == 0 and a NaN n: served, the clean point's answer and the referee's
    for x in (0, 2**31 - 1):
        rng = _engines(n * K)
        at = 11 * K + (K - 1)
        rng["x"][at] = x
        before = rng.copy()
        out = np.full((n, 27), 7, F)
        st = rt.rt_bake_stats()
        st.struct_size, st.launches = C.sizeof(st), 77
        params = rt.make_bake_params(SAMPLES, K, rt.RT_BAKE_SH9, DEPTH, 0)
        code = rt.lib.rt_render_probes(scene._h, points.ctypes.data, n, C.byref(params), rng.ctypes.data, out.ctypes.data, C.byref(st))
        msg = rt.lib.rt_last_error().decode()
        assert code == rt.RT_ERR_INVALID_ARG and msg == f"rt_render_probes: rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)", msg
        assert st.launches == 77 and np.array_equal(rng, before) and (out == 7).all()
    # no points: RT_OK without a launch, with and without arrays
    out, st = scene.render_probes(points[:0], _engines(1)[:0].copy(), SAMPLES, K, ray_depth=DEPTH)
    assert out.shape == (0, 9, 3) and (st.launches, st.points, st.paths) == (0, 0, 0)
    params = rt.make_bake_params(SAMPLES, K, rt.RT_BAKE_SH9, DEPTH, 0)
    assert rt.lib.rt_render_probes(scene._h, None, 0, C.byref(params), None, None, None) == rt.RT_OK
    with pytest.raises(rt.RtError) as e:                     # the other mode is rt_render_bake's
        rt._check(rt.lib.rt_render_probes(scene._h, points.ctypes.data, n, C.byref(rt.make_bake_params(SAMPLES, K, rt.RT_BAKE_IRRADIANCE, DEPTH, 0)),
                                          _engines(n * K).ctypes.data, np.zeros((n, 27), F).ctypes.data, None))
    assert e.value.code == rt.RT_ERR_INVALID_ARG and "rt_render_probes: params.mode = RT_BAKE_IRRADIANCE" in str(e.value) and "rt_render_bake" in str(e.value)


DEVICE = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import bake_model as bm
import scatter_model as model
import surface_cases as sc
import test_gpu_bake as tb
scene = rt.Scene(sc.scene_data("soup_a"))
dev = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()   # words, not floats: no copy may touch a NaN
host = lambda t: t.cpu().numpy().view(np.uint32)
points = tb._points(rt, scene, "soup_a")[:100]
n, K = len(points), 4
brng = model.seed(1 + 7919 * np.arange(n * K))
want_rng = brng.copy()
want, st_w = scene.render_probes(points, want_rng, tb.SAMPLES, K, ray_depth=tb.DEPTH)
want = want.reshape(n, 27)
# device pointers give the host arrays' bytes
d_pts, d_brng = dev(points, 6), dev(brng, 4)
d_out = torch.full((n, 27), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_d = scene.render_probes_device(d_pts.data_ptr(), d_brng.data_ptr(), n, d_out.data_ptr(), tb.SAMPLES, K, ray_depth=tb.DEPTH)
assert (st_d.points, st_d.invalid_points, st_d.paths, st_d.launches, st_d.exact_walks) == (n, 0, st_w.paths, st_w.launches, st_w.exact_walks)
assert np.array_equal(host(d_out), want.view(np.uint32)) and np.array_equal(host(d_brng), want_rng.view(np.uint32).reshape(-1, 4))
assert np.array_equal(host(d_pts), points.view(np.uint32).reshape(-1, 6))
# one bad engine among a point's K, from device memory: the point answers 27 zeros, keeps all its engines' bytes, is counted once
bad = brng.copy()
bad["x"][11 * K + 3], bad["x"][40 * K] = 2**31 - 1, 0
bad["saved"][11 * K + 1], bad["reserved"][40 * K + 2] = 5.0, 77
d_bad = dev(bad, 4)
d_out2 = torch.full((n, 27), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
st_b = scene.render_probes_device(d_pts.data_ptr(), d_bad.data_ptr(), n, d_out2.data_ptr(), tb.SAMPLES, K, ray_depth=tb.DEPTH)
got, got_rng = host(d_out2), host(d_bad)
assert st_b.invalid_points == 2 and st_b.paths == st_w.paths - 2 * tb.SAMPLES and not got[[11, 40]].any()
own = np.concatenate([np.arange(11 * K, 12 * K), np.arange(40 * K, 41 * K)])
assert np.array_equal(got_rng[own], bad.view(np.uint32).reshape(-1, 4)[own])
good = np.ones(n, bool); good[[11, 40]] = False
assert np.array_equal(got[good], want.view(np.uint32)[good])
assert np.array_equal(got_rng[np.repeat(good, K)], want_rng.view(np.uint32).reshape(-1, 4)[np.repeat(good, K)])
# ... as the referee has it from the same device memory
ref_out = torch.full((n, 27), -1, dtype=torch.int32, device="cuda")
d_bad2 = dev(bad, 4)
torch.cuda.synchronize()
st_ref = scene.bake_device(d_pts.data_ptr(), d_bad2.data_ptr(), n, ref_out.data_ptr(), tb.SAMPLES, K, mode=bm.SH9, ray_depth=tb.DEPTH)
assert st_ref.invalid_points == 2 and np.array_equal(host(ref_out), got) and np.array_equal(host(d_bad2), got_rng)
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_and_bad_device_engines():
    """RT_QUERY_DEVICE_POINTERS with torch tensors: the host path's bytes, engines included; a bad engine in device memory makes its point
    invalid (27 zeros, all K engines' bytes kept, counted once).  In a process of its own, where torch opens the GPU first."""
    r = subprocess.run([sys.executable, "-c", DEVICE.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seam_case(rt, scene):
    """100 points x K = 4 with one invalid point: the digest of coefficients and engines, and the launches."""
    points = _points(rt, scene, "soup_a")[:100].copy()
    points["p"][37, 1] = np.nan
    b = _engines(400)
    out, st = scene.render_probes(points, b, SAMPLES, 4, ray_depth=DEPTH)
    assert st.invalid_points == 1 and st.paths == 99 * SAMPLES
    return _digest(out, b), st.launches


SEAMS = """
import importlib, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
import test_gpu_render_probes as t
scene = rt.Scene(sc.scene_data("soup_a"))
digest, launches = t._seam_case(rt, scene)
print("SEAMS", digest, launches)
"""


def test_chunk_seams_change_no_answer(rt, scenes):
    """RTAMD_QUERY_CHUNK=128 in a fresh child process: four chunks of 32 whole points for 100 points of 4 slots; the bytes of the one chunk here."""
    digest, launches = _seam_case(rt, scenes("soup_a"))
    env = dict(os.environ, RTAMD_QUERY_CHUNK="128")
    r = subprocess.run([sys.executable, "-c", SEAMS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SEAMS" in r.stdout, r.stdout + r.stderr
    got = r.stdout.split("SEAMS", 1)[1].split()
    assert got[0] == digest
    assert int(got[1]) == 4 * launches, (got, launches)


WAVEFRONT = """
import importlib, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import scatter_model as model
import surface_cases as sc
scene = rt.Scene(sc.scene_data("soup_a"))
p = np.zeros((4, 3), np.float32)
try:
    scene.render_probes(rt.pack_bake_points(p, p), model.seed(1 + np.arange(4)), 2)
    raise SystemExit("served")
except rt.RtError as e:
    assert e.code == rt.RT_ERR_UNSUPPORTED and "rt_render_probes: " in str(e) and "no fallback" in str(e), str(e)
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
        points = _points(rt, scene, "soup_a")[:50]
        _equal_calls(scene, points, 4)
        assert acc.save() == blob and scene.info().device_bytes == bytes_before
        acc.render(4)
        after, _ = acc.resolve()
        whole, _, _ = scene.render(24, 16, 8)
        assert np.array_equal(after.view(np.uint32), whole.view(np.uint32))
        again, _, _ = scene.render(24, 16, 2)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
        # the irradiance source kernel on the same scene afterwards: rt_bake's bits still
        ref_rng, got_rng = _engines(200), _engines(200)
        ref, _ = scene.bake(points, ref_rng, SAMPLES, 4, bm.IRRADIANCE, DEPTH)
        got, _ = scene.render_bake(points, got_rng, SAMPLES, 4, ray_depth=DEPTH)
        assert _same(got, ref) and _same(got_rng, ref_rng)
    finally:
        scene.close()
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    try:
        p = np.zeros((4, 3), F)
        with pytest.raises(rt.RtError) as e:
            hw6.render_probes(rt.pack_bake_points(p, p), model.seed(1 + np.arange(4)), 2)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "rt_render_probes: " in str(e.value) and "hw8 / hw7" in str(e.value)
    finally:
        hw6.close()
    env = dict(os.environ, RTAMD_KERNEL="wavefront")
    r = subprocess.run([sys.executable, "-c", WAVEFRONT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "REFUSED" in r.stdout, r.stdout + r.stderr

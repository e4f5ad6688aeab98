"""The baker on the GPU (rt_bake_rays, rt_bake) against tests/bake_model.py and against the loop of public calls it is a composition of.

Points: the GPU's own closest hits of test_gpu_query.py's 48x32 camera set, p = o + t * d, n = ng, at most 256; samples = 8, K in {1, 4},
ray_depth = 4; the engine of candidate slot j is seeded 1 + 7919 * j.  The scheduling statistics need every slot to hold at least one
path shorter than ray_depth (else regeneration cannot save a round): the model is run over the candidates first and the points whose
K slots all satisfy that are kept, with their engines -- a slot's paths depend on its point and its engine alone, so the subset's paths
are the candidates' paths.  On every scene and K used here more than 32 points remain."""
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
import test_gpu_query as tq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MISS = sc.MISS
SAMPLES, DEPTH = 8, 4
CASES = [(name, mode, K) for name in ("soup_a", "soup_b", "sphere_emissive_env") for mode in (bm.IRRADIANCE, bm.SH9) for K in (1, 4)]


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


def _points(rt, scene, name, limit=256):
    """BAKE_POINT_DTYPE records at the GPU's own closest hits of the camera set."""
    o, d = tq._camera_rays(sc.scene_data(name))
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != MISS
    o, d, hits = o[on][:limit], d[on][:limit], hits[on][:limit]
    p = (o + hits["t"][:, None] * d).astype(F)
    return rt.pack_bake_points(p, hits["ng"])


def _engines(n):
    return model.seed(1 + 7919 * np.arange(n))


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def _same(a, b):
    return np.array_equal(_words(a), _words(b))


_CASE = {}


def _case(rt, scenes, name, mode, K):
    """Per case, once: the kept points and engines, the model's answer over the Scene's single calls, and its query counts."""
    key = (name, mode, K)
    if key not in _CASE:
        scene = scenes(name)
        cand = _points(rt, scene, name)
        rng = _engines(len(cand) * K)
        _, queries, valid = bm.bake(model.GpuCalls(scene), cand, rng.copy(), SAMPLES, K, mode, DEPTH)
        assert valid.all()
        short = (queries.reshape(len(cand), K, -1).min(axis=2) < DEPTH).all(axis=1)      # every slot of the point has a shorter path
        points, engines = np.ascontiguousarray(cand[short]), np.ascontiguousarray(rng.reshape(len(cand), K)[short].reshape(-1))
        assert len(points) > 32, (key, len(points))
        after = engines.copy()
        want, queries, _ = bm.bake(model.GpuCalls(scene), points, after, SAMPLES, K, mode, DEPTH)
        for a in (points, engines, after, want, queries):
            a.setflags(write=False)
        _CASE[key] = (points, engines, after, want, queries)
    return _CASE[key]


@pytest.mark.parametrize("name", ["sphere_emissive", "soup_a"])
@pytest.mark.parametrize("mode", [bm.IRRADIANCE, bm.SH9])
def test_bake_rays_are_the_models_bits(rt, scenes, name, mode):
    scene = scenes(name)
    points = _points(rt, scene, name)
    n = len(points)
    want_rng = _engines(n)
    want, invalid = bm.expected_rays(points, want_rng, mode)
    assert invalid == 0 and want_rng["has_saved"].all()
    got_rng = _engines(n)
    got, st = scene.bake_rays(points, got_rng, mode)
    assert (st.rays, st.invalid_rays, st.launches) == (n, 0, 1)
    assert _same(got, want), sc.first_difference(_words(got), _words(want))
    assert _same(got_rng, want_rng), sc.first_difference(_words(got_rng), _words(want_rng))
    if mode == bm.IRRADIANCE:
        assert ((got["d"] * points["n"]).sum(axis=1) > 0).all()
    else:
        assert np.array_equal(got["o"], points["p"]) and ((got["d"] * points["n"]).sum(axis=1) < 0).sum() > n // 4
    # records that enter with has_saved = 1, made by one earlier irradiance-mode call on the same engines
    saved_rng = _engines(n)
    scene.bake_rays(points, saved_rng, bm.IRRADIANCE)
    assert saved_rng["has_saved"].all()
    want_rng = saved_rng.copy()
    want, _ = bm.expected_rays(points, want_rng, mode)
    got, st = scene.bake_rays(points, saved_rng, mode)
    assert st.invalid_rays == 0 and not want_rng["has_saved"].any() and not want_rng["saved"].any()
    assert _same(got, want), sc.first_difference(_words(got), _words(want))
    assert _same(saved_rng, want_rng), sc.first_difference(_words(saved_rng), _words(want_rng))


@pytest.mark.parametrize("name,mode,K", CASES)
def test_lockstep_is_the_loop_of_public_calls(rt, scenes, name, mode, K):
    """bake_rays, trace_paths and a numpy fold per sample, on the GPU: rt_bake's bits under RT_BAKE_LOCKSTEP, outputs and engines."""
    scene = scenes(name)
    points, engines, after, want_model, queries = _case(rt, scenes, name, mode, K)
    loop_rng = engines.copy()
    make = lambda pts, rng, m: (scene.bake_rays(pts, rng, m)[0], 0)
    tracer = lambda o, d, rng: (scene.trace_paths(o, d, rng, ray_depth=DEPTH)[0], None)
    want, _, _ = bm.bake(None, points, loop_rng, SAMPLES, K, mode, DEPTH, make_rays=make, tracer=tracer)
    got_rng = engines.copy()
    got, st = scene.bake(points, got_rng, SAMPLES, K, mode, DEPTH, flags=rt.RT_BAKE_LOCKSTEP)
    q = SAMPLES // K
    print(f"{name} mode {mode} K {K}: {len(points)} points, lockstep {st.rounds} rounds, {st.live_ray_slots} of {st.ray_slots} ray slots live, {st.launches} launches")
    assert (st.points, st.invalid_points, st.paths, st.reference_exact) == (len(points), 0, len(points) * K * q, 1)
    assert st.rounds == q * DEPTH and st.ray_slots == q * DEPTH * len(points) * K and st.live_ray_slots == queries.sum()
    assert _same(got, want), sc.first_difference(_words(got), _words(want))
    assert _same(got_rng, loop_rng), sc.first_difference(_words(got_rng), _words(loop_rng))
    assert _same(want, want_model) and _same(loop_rng, after)        # and both are the model's over the single calls
    assert np.isfinite(got).all() and len(np.unique(got.reshape(len(points), -1), axis=0)) > len(points) // 2


@pytest.mark.parametrize("name,mode,K", CASES)
def test_regeneration_is_locksteps_bits_in_fewer_rounds(rt, scenes, name, mode, K):
    scene = scenes(name)
    points, engines, after, want, queries = _case(rt, scenes, name, mode, K)
    q = SAMPLES // K
    # the condition on the inputs first: every slot has a path shorter than the depth, so regeneration must save a round
    per_slot = queries.sum(axis=1)
    assert (queries.min(axis=1) < DEPTH).all() and per_slot.max() < q * DEPTH
    lock_rng, got_rng = engines.copy(), engines.copy()
    lock, st_l = scene.bake(points, lock_rng, SAMPLES, K, mode, DEPTH, flags=rt.RT_BAKE_LOCKSTEP)
    got, st = scene.bake(points, got_rng, SAMPLES, K, mode, DEPTH)
    print(f"{name} mode {mode} K {K}: {st.rounds} rounds against {st_l.rounds}, {st.live_ray_slots} of {st.ray_slots} ray slots live against {st_l.ray_slots}")
    assert _same(got, lock), sc.first_difference(_words(got), _words(lock))
    assert _same(got_rng, lock_rng), sc.first_difference(_words(got_rng), _words(lock_rng))
    assert _same(got, want) and _same(got_rng, after)
    assert st.live_ray_slots == st_l.live_ray_slots == queries.sum()
    assert st.rounds == per_slot.max() < st_l.rounds == q * DEPTH
    assert st.ray_slots == st.rounds * len(points) * K and st.paths == st_l.paths == len(points) * K * q
    # forcing the reference-order walks changes no bit
    ref_rng = engines.copy()
    ref, st_r = scene.bake(points, ref_rng, SAMPLES, K, mode, DEPTH, flags=rt.RT_QUERY_REFERENCE_WALK)
    assert _same(ref, got) and _same(ref_rng, got_rng) and st_r.exact_walks >= st.exact_walks and st_r.rounds == st.rounds


@pytest.mark.parametrize("mode", [bm.IRRADIANCE, bm.SH9])
def test_the_cpu_referee_gives_rt_bakes_bits(rt, scenes, mode):
    """32 points x 4 samples at depth 3 on soup_a, traced on the CPU through scatter_model.OracleCalls."""
    scene = scenes("soup_a")
    points = np.ascontiguousarray(_points(rt, scene, "soup_a")[::7][:32])
    assert len(points) == 32
    calls = model.OracleCalls(sc.scene_data("soup_a"), sc.oracle("soup_a"))
    for K in (1, 2):
        want_rng = _engines(32 * K)
        want, queries, _ = bm.bake(calls, points, want_rng, 4, K, mode, 3)
        assert len(np.unique(queries)) == 3
        got_rng = _engines(32 * K)
        got, st = scene.bake(points, got_rng, 4, K, mode, 3)
        assert st.live_ray_slots == queries.sum() and st.rounds == queries.sum(axis=1).max()
        assert _same(got, want), sc.first_difference(_words(got), _words(want))
        assert _same(got_rng, want_rng), sc.first_difference(_words(got_rng), _words(want_rng))


def test_above_the_scene_every_path_sees_the_background(rt):
    """Derived, not measured: points one unit above the scene's bounding box with n = (0, 1, 0) and a background B.  Every cosine path
    misses, so the irradiance is (pi / samples) * (B + ... + B): within samples * 2^-23 relative of pi * B (a rounding per addition,
    one for the scale, one for the product).  Where the model says that all of a record's uniform directions miss too, SH coefficient
    0 lies within the same margin of 4 pi * 0.282095 * B.  The points stand above the four corners of the box, 16 engines each."""
    B = np.array([0.25, 0.5, 0.75], F)
    sd = sc._with(sc.scene_data("soup_a"), bg=tuple(float(v) for v in B))
    scene = rt.Scene(sd)
    try:
        xyz = np.asarray(sd.positions, F).reshape(-1, 3)
        lo, hi = xyz.min(axis=0), xyz.max(axis=0)
        corners = np.array([[x, hi[1] + F(1), z] for x in (lo[0], hi[0]) for z in (lo[2], hi[2])], F)
        p = np.repeat(corners, 16, axis=0)
        points = rt.pack_bake_points(p, np.tile(np.array([0, 1, 0], F), (len(p), 1)))
        margin = SAMPLES * 2.0 ** -23
        calls = model.GpuCalls(scene)
        for mode in (bm.IRRADIANCE, bm.SH9):
            want_rng = _engines(len(p))
            missed = []                                       # per sample: the records whose first query misses

            def tracer(o, d, rng):
                missed.append(calls.closest(o, d)["triangle"] == MISS)
                return bm.trace_counted(calls, o, d, rng, DEPTH)
            want, queries, _ = bm.bake(calls, points, want_rng, SAMPLES, 1, mode, DEPTH, tracer=tracer)
            got_rng = _engines(len(p))
            got, st = scene.bake(points, got_rng, SAMPLES, 1, mode, DEPTH)
            assert _same(got, want) and _same(got_rng, want_rng)
            if mode == bm.IRRADIANCE:
                assert np.all(missed) and (queries == 1).all() and st.live_ray_slots == SAMPLES * len(p) and st.rounds == SAMPLES
                assert np.abs(got.astype(np.float64) / (np.pi * B.astype(np.float64)) - 1).max() <= margin
            else:
                clear = np.all(missed, axis=0)
                assert clear.sum() >= 4, clear.sum()
                c0 = got[clear][:, 0, :].astype(np.float64)
                assert np.abs(c0 / (4 * np.pi * float(F(0.282095)) * B.astype(np.float64)) - 1).max() <= margin
    finally:
        scene.close()


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seam_case(rt, scene):
    """100 points of soup_a, K = 4: the digest of both modes' outputs and engines, and the rounds."""
    points = np.ascontiguousarray(_points(rt, scene, "soup_a")[:100])
    assert len(points) == 100
    r1, r2 = _engines(400), model.seed(5 + 104729 * np.arange(400))
    irr, st1 = scene.bake(points, r1, SAMPLES, 4, bm.IRRADIANCE, DEPTH)
    sh, st2 = scene.bake(points, r2, SAMPLES, 4, bm.SH9, DEPTH, flags=rt.RT_BAKE_LOCKSTEP)
    return _digest(irr, r1, sh, r2), (st1.live_ray_slots, st2.live_ray_slots, st2.rounds)


SEAMS = """
import importlib, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
import test_gpu_bake as t
scene = rt.Scene(sc.scene_data("soup_a"))
digest, figures = t._seam_case(rt, scene)
print("SEAMS", digest, *figures)
"""


def test_chunk_seams_change_no_answer(rt, scenes):
    """RTAMD_QUERY_CHUNK=64 in a fresh child process: 16 points of four streams per chunk, seven chunks for 100 points, the bytes of
    the one chunk here; the lockstep rounds add up over the chunks."""
    digest, figures = _seam_case(rt, scenes("soup_a"))
    env = dict(os.environ, RTAMD_QUERY_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", SEAMS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SEAMS" in r.stdout, r.stdout + r.stderr
    got = r.stdout.split("SEAMS", 1)[1].split()
    assert got[0] == digest
    assert [int(v) for v in got[1:4]] == [figures[0], figures[1], 7 * figures[2]], (got, figures)


DEVICE_POINTERS = """
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
import test_gpu_bake as t
scene = rt.Scene(sc.scene_data("soup_a"))
points = t._points(rt, scene, "soup_a")
n, K = len(points), 4
dev = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()   # words, not floats
host = lambda x: x.cpu().numpy().view(np.uint32)
d_points = dev(points, 6)
for mode, floats in ((bm.IRRADIANCE, 3), (bm.SH9, 27)):
    rng_r = t._engines(n)
    rays, st_r = scene.bake_rays(points, rng_r, mode)
    d_rng_r, d_rays = dev(t._engines(n), 4), torch.full((n, 6), -1, dtype=torch.int32, device="cuda")
    st = scene.bake_rays_device(d_points.data_ptr(), d_rng_r.data_ptr(), n, d_rays.data_ptr(), mode)
    assert (st.rays, st.invalid_rays, st.launches) == (n, 0, st_r.launches)
    assert np.array_equal(host(d_rays), rays.view(np.uint32).reshape(-1, 6)) and np.array_equal(host(d_rng_r), rng_r.view(np.uint32).reshape(-1, 4))
    for flags in (0, rt.RT_BAKE_LOCKSTEP):
        rng = t._engines(n * K)
        out, st_h = scene.bake(points, rng, t.SAMPLES, K, mode, t.DEPTH, flags=flags)
        d_rng, d_out = dev(t._engines(n * K), 4), torch.full((n, floats), -1, dtype=torch.int32, device="cuda")
        st = scene.bake_device(d_points.data_ptr(), d_rng.data_ptr(), n, d_out.data_ptr(), t.SAMPLES, K, mode, t.DEPTH, flags=flags)
        assert (st.rounds, st.ray_slots, st.live_ray_slots, st.paths, st.launches, st.exact_walks) == (st_h.rounds, st_h.ray_slots, st_h.live_ray_slots, st_h.paths, st_h.launches, st_h.exact_walks)
        assert np.array_equal(host(d_out), out.view(np.uint32).reshape(n, floats)) and np.array_equal(host(d_rng), rng.view(np.uint32).reshape(-1, 4))
assert np.array_equal(host(d_points), points.view(np.uint32).reshape(-1, 6))
P = lambda x, off=0: x.data_ptr() + off
code = rt.lib.rt_bake_rays(scene._h, P(d_points), P(d_rng_r, 8), 1, 0, rt.RT_QUERY_DEVICE_POINTERS, P(d_rays), None)
msg = rt.lib.rt_last_error().decode()
assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_bake_rays: ") and "16-byte aligned" in msg, (code, msg)
params = rt.make_bake_params(t.SAMPLES, K, 0, t.DEPTH, rt.RT_QUERY_DEVICE_POINTERS)
code = rt.lib.rt_bake(scene._h, P(d_points), 1, params, P(d_rng, 4), P(d_out), None)
msg = rt.lib.rt_last_error().decode()
assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_bake: ") and "16-byte aligned" in msg, (code, msg)
print("DEVICE POINTERS EQUAL")

# a bad engine from device memory: the point answers zeros, all its engines stay, it is counted once; the neighbours keep their bits
clean_rng = t._engines(n * K)
clean, _ = scene.bake(points, clean_rng, t.SAMPLES, K, 0, t.DEPTH)
bad_points = np.array([3, 40, 41, n - 1])
bad = t._engines(n * K)
before = bad.copy()
for j, (i, x) in enumerate(zip(bad_points, (0, 2**31 - 1, 2**32 - 1, 0))):
    bad["x"][i * K + j % K] = x
    before["x"][i * K + j % K] = x
d_rng, d_out = dev(bad, 4), torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
st = scene.bake_device(d_points.data_ptr(), d_rng.data_ptr(), n, d_out.data_ptr(), t.SAMPLES, K, 0, t.DEPTH)
got, got_rng = host(d_out), host(d_rng).reshape(n, K, 4)
ok = np.ones(n, bool)
ok[bad_points] = False
assert st.invalid_points == len(bad_points) and st.paths == (n - len(bad_points)) * t.SAMPLES
assert not got[bad_points].any() and np.array_equal(got_rng[bad_points], before.view(np.uint32).reshape(n, K, 4)[bad_points])
assert np.array_equal(got[ok], clean.view(np.uint32)[ok]) and np.array_equal(got_rng[ok], clean_rng.view(np.uint32).reshape(n, K, 4)[ok])
d_rng_r, d_rays = dev(bad[:n], 4), torch.full((n, 6), -1, dtype=torch.int32, device="cuda")
st = scene.bake_rays_device(d_points.data_ptr(), d_rng_r.data_ptr(), n, d_rays.data_ptr(), 0)
rows = np.nonzero(~np.array([model.valid_state(x) for x in bad["x"][:n]]))[0]
assert st.invalid_rays == len(rows) >= 1 and np.all(host(d_rays)[rows] == bm.NO_RAY) and np.array_equal(host(d_rng_r)[rows], bad[:n].view(np.uint32).reshape(-1, 4)[rows])
print("BAD DEVICE ENGINES ANSWER ZEROS")
"""


@pytest.fixture(scope="module")
def device_run():
    """The child process of the two device-memory tests, where torch opens the GPU before the library does (the order bench.py keeps)."""
    return subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)


def test_device_pointers_give_the_host_arrays_bytes(device_run):
    assert "DEVICE POINTERS EQUAL" in device_run.stdout, device_run.stdout + device_run.stderr


def test_a_bad_engine_from_device_memory_makes_its_point_invalid(device_run):
    assert device_run.returncode == 0 and "BAD DEVICE ENGINES ANSWER ZEROS" in device_run.stdout, device_run.stdout + device_run.stderr


@pytest.mark.parametrize("mode", [bm.IRRADIANCE, bm.SH9])
def test_invalid_points_answer_zeros_and_keep_their_engines(rt, scenes, mode):
    scene = scenes("soup_a")
    points = _points(rt, scene, "soup_a")
    n, K = len(points), 4
    clean_rng = _engines(n * K)
    clean, st_c = scene.bake(points, clean_rng, SAMPLES, K, mode, DEPTH)
    assert st_c.invalid_points == 0
    dirty = points.copy()
    nan_p, zero_n = np.arange(3, n, 17), np.arange(5, n, 19)
    zero_n = zero_n[~np.isin(zero_n, nan_p)]
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(nan_p):
        dirty["p"][i, k % 3] = poison[(k // 3) % 3]
    dirty["n"][zero_n] = 0
    dirty["n"][zero_n[::2], 1] = np.nan if mode == bm.IRRADIANCE else 0     # a non-finite n as well, where n is read
    invalid = np.union1d(nan_p, zero_n) if mode == bm.IRRADIANCE else nan_p   # a zero n is valid in SH9: n is not read
    rng = _engines(n * K)
    got, st = scene.bake(dirty, rng, SAMPLES, K, mode, DEPTH)
    ok = np.ones(n, bool)
    ok[invalid] = False
    assert len(invalid) >= 10 and st.invalid_points == len(invalid) and st.points == n and st.paths == ok.sum() * SAMPLES
    assert not got[invalid].view(np.uint32).any()
    assert np.array_equal(rng.reshape(n, K)[invalid], _engines(n * K).reshape(n, K)[invalid])
    assert _same(got[ok], clean[ok]) and np.array_equal(rng.reshape(n, K)[ok], clean_rng.reshape(n, K)[ok])
    lock_rng = _engines(n * K)
    lock, st_l = scene.bake(dirty, lock_rng, SAMPLES, K, mode, DEPTH, flags=rt.RT_BAKE_LOCKSTEP)
    assert _same(lock, got) and np.array_equal(lock_rng, rng) and st_l.invalid_points == len(invalid)
    # rt_bake_rays: the same records get the invalid ray, keep their engines and are counted
    rays_rng = _engines(n)
    rays, st_r = scene.bake_rays(dirty, rays_rng, mode)
    assert st_r.invalid_rays == len(invalid) and np.all(_words(rays)[invalid] == bm.NO_RAY) and np.array_equal(rays_rng[invalid], _engines(n)[invalid])
    want_rng = _engines(n)
    want, count = bm.expected_rays(dirty, want_rng, mode)
    assert count == len(invalid) and _same(rays, want) and _same(rays_rng, want_rng)


def test_hw6_is_unsupported_and_a_bake_moves_nothing_else(rt):
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    try:
        points = rt.pack_bake_points(np.zeros((4, 3), F), np.tile(np.array([0, 1, 0], F), (4, 1)))
        for fn, call in (("rt_bake_rays", lambda: hw6.bake_rays(points, _engines(4))), ("rt_bake", lambda: hw6.bake(points, _engines(4), 4))):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt.RT_ERR_UNSUPPORTED and f"{fn}: " in str(e.value) and "hw8 / hw7" in str(e.value)
    finally:
        hw6.close()
    scene = rt.Scene(sc.scene_data("soup_a"))
    try:
        o, d = tq._camera_rays(sc.scene_data("soup_a"))
        o, d = np.ascontiguousarray(o[:256]), np.ascontiguousarray(d[:256])
        r0 = _engines(256)
        L0, st0 = scene.trace_paths(o, d, r0)
        frame0, _, _ = scene.render(24, 16, 2)
        bytes_before = scene.info().device_bytes
        points = _points(rt, scene, "soup_a", 64)
        scene.bake(points, _engines(64 * 4), SAMPLES, 4, bm.SH9, DEPTH)
        scene.bake(points, _engines(64), SAMPLES, 1, bm.IRRADIANCE, DEPTH, flags=rt.RT_BAKE_LOCKSTEP)
        scene.bake_rays(points, _engines(64))
        r1 = _engines(256)
        L1, st1 = scene.trace_paths(o, d, r1)
        frame1, _, _ = scene.render(24, 16, 2)
        assert np.array_equal(L1.view(np.uint32), L0.view(np.uint32)) and np.array_equal(r1, r0) and st1.launches == st0.launches
        assert np.array_equal(frame1.view(np.uint32), frame0.view(np.uint32)) and scene.info().device_bytes == bytes_before
        empty, st = scene.bake(points[:0], _engines(1)[:0].copy(), SAMPLES)
        assert empty.shape == (0, 3) and (st.launches, st.rounds, st.points) == (0, 0, 0)
    finally:
        scene.close()

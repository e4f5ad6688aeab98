"""Occlusion queries on the GPU (rt_query_occluded) against the CPU oracle: bit 0 of every valid ray's byte is `the oracle's closest hit
exists and its t < tmax`, a strict float32 compare, and where oracle/_ref holds the compiled reference the same of Ref8.  The expected
bit never comes from the code under test.  Scenes, ray sets (at most 2,048 rays each) and the oracle's cached answers are those of
tests/test_gpu_query.py.

tmax sets, with T the oracle's closest t of the ray (the scene's coordinate bound for a ray that misses):
  none NULL | inf +inf | equal T (answer 0) | above nextafter(T, inf) (answer 1 on a hit) | below nextafter(T, 0) | near T (1 +- 2^-20)
  behind T (1 + 2^-6), just past the walkers' relative look-behind | random T * uniform(0.2, 1.8) | limits 1e4, 2e4, 9999.999, 1e-30"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_query as T

pytestmark = pytest.mark.gpu

MISS = T.MISS
TMAX_SETS = ["none", "inf", "equal", "above", "below", "near", "behind", "random", "limits"]


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = rt.Scene(T._scene_data(name), **kw)
        return made[key]
    yield get
    for s in made.values():
        s.close()


def _hit_and_t(hits, name):
    """(hit?, T) of rt_hit records: T is the closest t, or the scene's bound for a miss."""
    hit = hits["triangle"] != MISS
    t = np.where(hit, hits["t"], np.float32(T._bound(T._scene_data(name)))).astype(np.float32)
    return hit, t


@functools.lru_cache(maxsize=None)
def _oracle_closest(name, which):
    hit, t = _hit_and_t(T._answers(name, which)[0], name)
    hit.setflags(write=False)
    t.setflags(write=False)
    return hit, t


def _closest_of(impl, o, d):
    """(hit?, t) of an implementation's closest_hit, ray by ray."""
    hit, t = np.zeros(len(o), bool), np.zeros(len(o), np.float32)
    for i in range(len(o)):
        idx, v = impl.closest_hit(o[i], d[i])
        hit[i], t[i] = idx >= 0, v[0] if idx >= 0 else 0
    return hit, t


@functools.lru_cache(maxsize=None)
def _ref_closest(name, which):
    ref = T._ref8(name)
    return None if ref is None else _closest_of(ref, *T._rays(name, which))


def _tmax(kind, t, seed=17):
    """The tmax array of a set for rays whose T is t (None: no array)."""
    t = np.asarray(t, np.float32)
    n = len(t)
    if kind == "none":
        return None
    if kind == "inf":
        return np.full(n, np.inf, np.float32)
    if kind == "equal":
        return t.copy()
    if kind == "above":
        return np.nextafter(t, np.float32(np.inf))
    if kind == "below":
        return np.nextafter(t, np.float32(0))
    if kind == "near":
        return (t * np.where(np.arange(n) % 2 == 0, np.float32(1 + 2.0 ** -20), np.float32(1 - 2.0 ** -20))).astype(np.float32)
    if kind == "behind":
        return (t * np.float32(1 + 2.0 ** -6)).astype(np.float32)
    if kind == "random":
        return (t * np.random.default_rng(seed).uniform(0.2, 1.8, n).astype(np.float32)).astype(np.float32)
    if kind == "limits":
        return np.resize(np.array([1e4, 2e4, 9999.999, 1e-30], np.float32), n)
    raise KeyError(kind)


def _expected(hit, t, tmax):
    return (hit if tmax is None else hit & (t < tmax)).astype(np.uint8)


def _diff(got, want):
    rows = np.nonzero(got != want)[0]
    return f"{len(rows)} of {len(got)} rays differ, first {rows[:8].tolist()}: got {got[rows[:8]].tolist()}, want {want[rows[:8]].tolist()}"


def _check_against(rt, scene, o, d, tmax, want, fast_path_ran, ref_want=None, label=""):
    fast, st = scene.query_occluded(o, d, tmax)
    slow, st_ref = scene.query_occluded(o, d, tmax, flags=rt.RT_QUERY_REFERENCE_WALK)
    print(f"{label}: {st.rays} rays, {int(want.sum())} occluded, {st.exact_walks} exact walks, {st.launches} launches, {st.kernel_ms:.3f} ms")
    assert fast.dtype == np.uint8 and st.reference_exact == 1 and st.rays == len(o) and st.invalid_rays == 0 and st_ref.invalid_rays == 0
    assert np.array_equal(fast & 1, want), _diff(fast & 1, want)
    assert np.array_equal(slow & 1, want), _diff(slow & 1, want)
    mask = np.uint8(0xFF ^ rt.RT_OCCLUSION_EXACT_WALK)
    assert np.array_equal(fast & mask, slow & mask) and not np.any(fast & ~np.uint8(3))
    assert int(((fast & rt.RT_OCCLUSION_EXACT_WALK) != 0).sum()) == st.exact_walks
    assert int(((slow & rt.RT_OCCLUSION_EXACT_WALK) != 0).sum()) == st_ref.exact_walks
    if fast_path_ran:
        assert st.exact_walks < st.rays
    if ref_want is not None:
        assert np.array_equal(fast & 1, ref_want), _diff(fast & 1, ref_want)
    return fast, st


@pytest.mark.parametrize("kind", TMAX_SETS)
@pytest.mark.parametrize("which", T.SETS)
@pytest.mark.parametrize("name", list(T.SCENES))
def test_occlusion_is_the_oracles_closest_hit_below_tmax(rt, scenes, name, which, kind):
    o, d = T._rays(name, which)
    hit, t = _oracle_closest(name, which)
    tmax = _tmax(kind, t)
    want = _expected(hit, t, tmax)
    if kind == "equal":
        assert not want.any()
    if kind in ("above", "none", "inf"):
        assert np.array_equal(want, hit.astype(np.uint8))
    live = _ref_closest(name, which)
    ref_want = None if live is None else _expected(live[0], live[1], tmax)
    _check_against(rt, scenes(name), o, d, tmax, want, which in ("camera", "bounce"), ref_want, f"{name}/{which}/{kind}")


@functools.lru_cache(maxsize=None)
def _segments(name, stretch):
    """The camera rays as segments: d scaled by stretch * T, so the hit lies near t = 1 / stretch; the oracle asked on the scaled rays."""
    o, d = T._rays(name, "camera")
    _, t = _oracle_closest(name, "camera")
    ds = (np.float32(stretch) * t[:, None] * d).astype(np.float32)
    return o, ds, _closest_of(T._oracle(name), o, ds)


@pytest.mark.parametrize("end", ["at", "above", "below"])
@pytest.mark.parametrize("stretch", [1, 4])
@pytest.mark.parametrize("name", list(T.SCENES))
def test_segments_to_the_hit_point(rt, scenes, name, stretch, end):
    """stretch 1: the segment ends at the hit point, tmax 1 and its float neighbours.  stretch 4: the hit at a quarter of a segment four
    times as long, whose |d| lies partly beyond 16 on these scenes: those rays take the exact list by rq_classify's rule."""
    o, ds, (hit, t) = _segments(name, stretch)
    at = np.float32(1.0 / stretch)
    bound = {"at": at, "above": np.nextafter(at, np.float32(2)), "below": np.nextafter(at, np.float32(0))}[end]
    tmax = np.full(len(o), bound, np.float32)
    length = np.sqrt((ds.astype(np.float64) ** 2).sum(axis=1))
    outside = int(((length < 0.0625 * (1 - 1e-6)) | (length > 16 * (1 + 1e-6))).sum())
    print(f"{name}: |d| in [{length.min():.3g}, {length.max():.3g}], {outside} of {len(o)} outside [1/16, 16]")
    ref = T._ref8(name)
    ref_want = None
    if ref is not None:
        ref_want = _expected(*_closest_of(ref, o, ds), tmax)
    _, st = _check_against(rt, scenes(name), o, ds, tmax, _expected(hit, t, tmax), False, ref_want, f"{name}/segments x{stretch}/{end}")
    assert st.exact_walks >= outside


def _mixed_rays(name):
    parts = [T._rays(name, w) for w in ("camera", "bounce", "far")]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("variant", ["default", "device_bvh", "no_exact_boxes"])
def test_consistent_with_query_closest_on_the_same_scene(rt, scenes, monkeypatch, variant):
    name = "sphere_emissive"
    o, d = _mixed_rays(name)
    n_far = len(T._rays(name, "far")[0])
    if variant == "no_exact_boxes":
        monkeypatch.setenv("RTAMD_NO_EXACT_BOXES", "1")
        scene = rt.Scene(T._scene_data(name))
    else:
        scene = scenes(name, **({"build_flags": rt.RT_BUILD_DEVICE_BVH} if variant == "device_bvh" else {}))
    try:
        hits, st_c = scene.query_closest(o, d)
        hit, t = _hit_and_t(hits, name)
        for kind in TMAX_SETS:
            tmax = _tmax(kind, t)
            for flags in (0, rt.RT_QUERY_REFERENCE_WALK):
                occ, st = scene.query_occluded(o, d, tmax, flags=flags)
                want = _expected(hit, t, tmax)
                assert np.array_equal(occ & 1, want), (kind, flags, _diff(occ & 1, want))
                assert st.reference_exact == (1 if variant == "default" else 0) == st_c.reference_exact
                assert int(((occ & rt.RT_OCCLUSION_EXACT_WALK) != 0).sum()) == st.exact_walks
                if variant != "default" and flags == 0:
                    assert st.exact_walks == st_c.exact_walks == n_far, (kind, st.exact_walks, st_c.exact_walks)
    finally:
        if variant == "no_exact_boxes":
            scene.close()


@pytest.mark.parametrize("name", ["sphere_emissive", "practice7_1"])
def test_invalid_and_trivial_rays_among_valid_ones(rt, scenes, name):
    scene = scenes(name)
    o, d = (a[:512].copy() for a in T._rays(name, "camera"))
    hit, t = (a[:512] for a in _oracle_closest(name, "camera"))
    tmax = _tmax("random", t)
    clean, _ = scene.query_occluded(o, d, tmax)
    bad = np.arange(3, 512, 7)                                        # the poison pattern of test_invalid_rays_are_flagged_and_change_nothing
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        c = k % 7
        if c == 6:
            d[i] = 0
        else:
            (o if c < 3 else d)[i, c % 3] = poison[(k // 7) % 3]
    d[bad[-1]] = (-0.0, 0.0, -0.0)
    nan_t = np.arange(5, 512, 35)                                     # 5 mod 7: none of them a poisoned ray
    trivial = np.arange(6, 512, 21)                                   # 6 mod 7
    tmax[nan_t] = np.nan
    tmax[trivial] = np.resize(np.array([0.0, -0.0, -1.0, -np.inf], np.float32), len(trivial))
    tmax[bad[:8]] = np.resize(np.array([0.0, np.nan, -1.0], np.float32), 8)   # an invalid ray stays invalid whatever its bound
    invalid = np.zeros(512, bool)
    invalid[bad] = invalid[nan_t] = True
    untouched = ~invalid
    untouched[trivial] = False
    want = _expected(hit, t, tmax)
    for flags in (0, rt.RT_QUERY_REFERENCE_WALK):
        occ, st = scene.query_occluded(o, d, tmax, flags=flags)
        assert st.rays == 512 and st.invalid_rays == int(invalid.sum()) == len(bad) + len(nan_t)
        assert np.all(occ[invalid] == rt.RT_OCCLUSION_INVALID_RAY) and not np.any(occ[~invalid] & rt.RT_OCCLUSION_INVALID_RAY)
        assert np.all(occ[trivial] == 0)                              # valid, not occluded, never walked: no exact-walk flag either
        assert np.array_equal(occ[~invalid] & 1, want[~invalid])
        if flags == 0:
            assert np.array_equal(occ[untouched], clean[untouched])
        else:
            assert st.exact_walks == 512 - int(invalid.sum()) - len(trivial)
    occ, st = scene.query_occluded(o, d)                              # without bounds only the poisoned rays are invalid
    assert st.invalid_rays == len(bad) and np.array_equal(occ[~invalid] & 1, hit[~invalid].astype(np.uint8))


def _many(scene, name):
    """T._many_rays with bounds around query_closest's own t: the launch-shape tests compare the call with itself."""
    o, d = T._many_rays(name)
    _, t = _hit_and_t(scene.query_closest(o, d)[0], name)
    return o, d, _tmax("random", t, seed=23)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_size_changes_no_answer(rt, scenes, n):
    scene = scenes("sphere_emissive")
    o, d, tmax = _many(scene, "sphere_emissive")
    everything, _ = scene.query_occluded(o, d, tmax)
    anything, _ = scene.query_occluded(o, d)
    head, st = scene.query_occluded(o[:n], d[:n], tmax[:n])
    assert st.rays == n and np.array_equal(head, everything[:n])
    tail, _ = scene.query_occluded(o[-n:], d[-n:], tmax[-n:])
    assert np.array_equal(tail, everything[-n:])
    head, _ = scene.query_occluded(o[:n], d[:n])
    assert np.array_equal(head, anything[:n])


def test_chunk_seams_change_no_answer(rt, scenes, monkeypatch):
    scene = scenes("sphere_emissive")
    o, d, tmax = _many(scene, "sphere_emissive")
    occ, st = scene.query_occluded(o, d, tmax)
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "1000")
    occ_c, st_c = scene.query_occluded(o, d, tmax)
    assert st_c.launches == -(-len(o) // 1000) * st.launches
    assert st_c.exact_walks == st.exact_walks and st_c.rays == len(o) and np.array_equal(occ_c, occ)


@pytest.mark.parametrize("which", T.SETS)
def test_spill_variant_answers_the_same_bytes(rt, scenes, monkeypatch, which):
    """RTAMD_WF_LDS_STACK=3, as tests/test_gpu_edge_cases.py sets it: three stack entries in LDS, the rest in the overflow area."""
    name = "practice7_1"
    scene = scenes(name)
    o, d = T._rays(name, which)
    hit, t = _oracle_closest(name, which)
    for kind in ("none", "random", "near"):
        tmax = _tmax(kind, t)
        plain, st = scene.query_occluded(o, d, tmax)
        monkeypatch.setenv("RTAMD_WF_LDS_STACK", "3")
        spill, st_s = scene.query_occluded(o, d, tmax)
        monkeypatch.delenv("RTAMD_WF_LDS_STACK")
        assert scene.info().bvh_depth > 3
        assert np.array_equal(spill, plain) and st_s.exact_walks == st.exact_walks
        assert np.array_equal(spill & 1, _expected(hit, t, tmax))


def test_no_rays_is_ok_without_a_launch(rt, scenes):
    scene = scenes("sphere_emissive")
    st = rt.rt_query_stats()
    st.struct_size = C.sizeof(st)
    assert rt.lib.rt_query_occluded(scene._h, None, None, 0, 0, None, C.byref(st)) == rt.RT_OK
    assert (st.rays, st.exact_walks, st.invalid_rays, st.launches, st.kernel_ms) == (0, 0, 0, 0, 0.0) and st.reference_exact == 1
    occ, st = scene.query_occluded(np.zeros((0, 3)), np.zeros((0, 3)))
    assert occ.shape == (0,) and st.launches == 0


def test_scenes_it_does_not_serve_and_bad_arguments(rt, scenes):
    import pin_cases
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    rays = rt.pack_rays(np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1)))
    out = np.zeros(4, np.uint8)
    try:
        code = rt.lib.rt_query_occluded(hw6._h, rays.ctypes.data, None, 4, 0, out.ctypes.data, None)
        assert code == rt.RT_ERR_UNSUPPORTED and "hw8 / hw7" in rt.lib.rt_last_error().decode()
    finally:
        hw6.close()
    scene = scenes("sphere_emissive")
    code = rt.lib.rt_query_occluded(scene._h, None, None, 4, 0, out.ctypes.data, None)
    assert code == rt.RT_ERR_INVALID_ARG and rt.lib.rt_last_error().decode() == "rt_query_occluded: null argument (rays)"
    code = rt.lib.rt_query_occluded(scene._h, 256, 258, 1, rt.RT_QUERY_DEVICE_POINTERS, 257, None)
    assert code == rt.RT_ERR_INVALID_ARG and "4-byte aligned" in rt.lib.rt_last_error().decode()


DEVICE_POINTERS = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import test_gpu_query as T
scene = rt.Scene(T._scene_data("sphere_emissive"))
w, h = 96, 64
n = w * h
xy = np.stack([np.tile(np.arange(w, dtype=np.float32) + 0.5, h), np.repeat(np.arange(h, dtype=np.float32) + 0.5, w)], axis=1)
d_xy = torch.from_numpy(xy).cuda()
rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
scene.camera_rays_device(w, h, d_xy.data_ptr(), n, rays.data_ptr())
host = rays.cpu().numpy()
o, d = host[:, :3].copy(), host[:, 3:].copy()
hits, _ = scene.query_closest(o, d)
t = np.where(hits["triangle"] != T.MISS, hits["t"], np.float32(1)).astype(np.float32)
tmax = (t * np.random.default_rng(29).uniform(0.2, 1.8, n).astype(np.float32)).astype(np.float32)
d_tmax = torch.from_numpy(tmax).cuda()
for flags in (0, rt.RT_QUERY_REFERENCE_WALK):
    for bounds, d_bounds in ((tmax, d_tmax.data_ptr()), (None, None)):
        occ, st = scene.query_occluded(o, d, bounds, flags=flags)
        store = torch.full((n + 2,), 0xFF, dtype=torch.uint8, device="cuda")
        out = store[1:n + 1]                         # one byte into the allocation: the output is byte-addressed
        assert out.data_ptr() == store.data_ptr() + 1
        torch.cuda.synchronize()
        st_d = scene.query_occluded_device(rays.data_ptr(), d_bounds, n, out.data_ptr(), flags=flags)
        got = store.cpu().numpy()
        assert st_d.rays == n and st_d.exact_walks == st.exact_walks and st_d.invalid_rays == 0
        assert got[0] == 0xFF and got[-1] == 0xFF and np.array_equal(got[1:-1], occ)
        assert 0 < int((occ & 1).sum()) < n
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with rays made by camera_rays_device and torch tensors as bounds and output, the output one byte into
    its allocation and pre-filled with 0xFF: the host call's bytes, with and without bounds.  In a process of its own, torch first."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=T.ROOT, tests=os.path.join(T.ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def test_the_call_only_reads(rt, scenes):
    """An rt_accum checkpoint and a query_closest answer taken before and after occlusion queries are the same bytes."""
    scene = scenes("sphere_emissive")
    o, d = T._rays("sphere_emissive", "bounce")
    _, t = _oracle_closest("sphere_emissive", "bounce")
    acc = scene.accumulator(32, 32)
    acc.render(2)
    blob = bytes(acc.save())
    hits, _ = scene.query_closest(o, d)
    scene.query_occluded(o, d)
    scene.query_occluded(o, d, _tmax("random", t))
    scene.query_occluded(o, d, _tmax("near", t), flags=rt.RT_QUERY_REFERENCE_WALK)
    assert bytes(acc.save()) == blob
    again, _ = scene.query_closest(o, d)
    acc.close()
    assert np.array_equal(again.view(np.uint32), hits.view(np.uint32))

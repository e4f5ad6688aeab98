"""Batched ray queries on the GPU (rt_query_closest, rt_query_light_pdf) against the CPU oracle, bit for bit: every valid ray's 64-byte
rt_hit equals the record made of Hw8Oracle.closest_hit's answer (index mapped through figure_order() to LOAD order), every light pdf
has the bits of Hw8Oracle.light_pdf.  Where oracle/_ref holds the compiled reference, the same against Ref8.  The oracle is asked once
per scene and ray set (at most 2,048 rays each) and the answers are shared.

Ray sets (fixed seeds, float32):  1 camera rays of a 48x32 frame;  2 bounce rays from their hit points, half random, half grazing into
the surface;  3 adversarial: axis directions with exact zeros, origins on the scene box's faces and corners, origins 10x and 10^4x
beyond the scene's coordinate bound, the camera rays with d scaled by 0.25 and by 8, rays that miss;  4 invalid rays among valid ones.

The light pdf queried is hw8's (shading normal), on every scene that has lights; practice7_1 is an hw7 example scene, created and
queried as the hw8 scene it loads as."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"sphere": lambda rt: rt.load_gltf(os.path.join(pin_cases.SCENES, "hw8_sphere", "sphere.gltf")),
          "sphere_emissive": lambda rt: pin_cases.load_sphere(),
          "practice7_1": lambda rt: pin_cases.load_hw7("practice7_1")}
SETS = ["camera", "bounce", "adversarial"]
MISS = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _scene_data(name):
    return SCENES[name](pin_cases.rt)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle_lib.Hw8Oracle(_scene_data(name))


@functools.lru_cache(maxsize=None)
def _ref8(name):
    return oracle_lib.Ref8(_scene_data(name)) if oracle_lib.ref_path("libref_hw8.so") else None


def _bound(sd):
    """max |coordinate| of scene and camera: what the gate's margin is derived for."""
    return float(max(np.abs(sd.positions).max(), np.abs(np.array(sd.camera.position, np.float32)).max()))


def _camera_rays(sd, w=48, h=32, seed=3):
    cam = sd.camera
    rng = np.random.default_rng(seed)
    px = (np.arange(w, dtype=np.float32)[None, :] + rng.uniform(0, 1, (h, w)).astype(np.float32)).reshape(-1)
    py = (np.arange(h, dtype=np.float32)[:, None] + rng.uniform(0, 1, (h, w)).astype(np.float32)).reshape(-1)
    tan_y = np.float32(np.tan(np.float64(cam.fov_y) / 2))
    tan_x = np.float32(tan_y * np.float32(w) / np.float32(h))
    cx = tan_x * (np.float32(2) * px / np.float32(w) - np.float32(1))
    cy = tan_y * (np.float32(2) * py / np.float32(h) - np.float32(1))
    right, up, fwd = (np.array(v, np.float32) for v in (cam.right, cam.up, cam.forward))
    d = cx[:, None] * right - cy[:, None] * up + fwd
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.broadcast_to(np.array(cam.position, np.float32), d.shape).copy()
    return o, d


def _expected_hits(impl, sd, o, d):
    """The rt_hit records an implementation's closest_hit answers amount to."""
    rt = pin_cases.rt
    order = impl.figure_order()
    exp = np.zeros(len(o), rt.HIT_DTYPE)
    for i in range(len(o)):
        idx, v = impl.closest_hit(o[i], d[i])
        if idx < 0:
            exp[i]["triangle"] = MISS
            continue
        exp[i]["t"], exp[i]["triangle"] = v[0], order[idx]
        exp[i]["ng"], exp[i]["texcoord"], exp[i]["ns"], exp[i]["tangent"] = v[1:4], v[4:6], v[6:9], v[9:13]
        exp[i]["flags"] = rt.RT_HIT_INSIDE if v[13] != 0 else 0
    return exp


def _orthogonal(rng, n):
    """Unit vectors orthogonal to the unit vectors n."""
    r = rng.normal(0, 1, n.shape)
    r -= (r * n).sum(axis=1, keepdims=True) * n
    return r / np.linalg.norm(r, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _rays(name, which):
    """(o, d) of a set, float32; "far" is the far-origin part of the adversarial set on its own."""
    sd = _scene_data(name)
    o1, d1 = _camera_rays(sd)
    if which == "camera":
        return o1, d1
    if which == "bounce":
        hits = _answers(name, "camera")[0]
        on = hits["triangle"] != MISS
        ng = hits["ng"][on].astype(np.float64)
        x = (o1[on] + hits["t"][on, None] * d1[on] + np.float32(1e-4) * hits["ng"][on]).astype(np.float32)
        x, ng = x[:2048], ng[:2048]
        rng = np.random.default_rng(5)
        d = pin_cases.unit(rng.normal(0, 1, x.shape))
        half = len(x) // 2
        graze = _orthogonal(rng, ng[half:]) - rng.uniform(1e-4, 0.05, (len(x) - half, 1)) * ng[half:]   # into the surface, nearly along it
        d[half:] = pin_cases.unit(graze)
        return x, d
    lo, hi = sd.positions.reshape(-1, 3).min(axis=0), sd.positions.reshape(-1, 3).max(axis=0)
    centre = ((lo + hi) / 2).astype(np.float32)
    bound = _bound(sd)
    rng = np.random.default_rng(9)
    if which == "far":
        dirs = pin_cases.unit(rng.normal(0, 1, (64, 3)))
        o = np.concatenate([centre + np.float32(10 * bound) * dirs[:32], centre + np.float32(1e4 * bound) * dirs[32:]]).astype(np.float32)
        target = centre + rng.uniform(-0.3, 0.3, (64, 3)).astype(np.float32) * (hi - lo)
        return o, pin_cases.unit(target - o)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    parts = []
    starts = np.concatenate([np.array([sd.camera.position], np.float32), centre + rng.uniform(-0.6, 0.6, (15, 3)).astype(np.float32) * (hi - lo)])
    parts.append((np.repeat(starts, 6, axis=0), np.tile(axes, (len(starts), 1))))                       # axis directions, exact zeros
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float32)
    faces = np.array([np.where(np.arange(3) == a, (lo, hi)[s][a], centre[a]) for a in range(3) for s in range(2)], np.float32)
    on_box = np.concatenate([corners, faces])
    parts.append((on_box, pin_cases.unit(centre - on_box)))                                             # from the box, at its centre
    parts.append((np.repeat(on_box, 6, axis=0), np.tile(axes, (len(on_box), 1))))                      # ... and along the axes, in its faces
    parts.append(_rays(name, "far"))
    pick = np.arange(0, len(o1), 4)
    parts.append((o1[pick], (np.float32(0.25) * d1[pick]).astype(np.float32)))
    parts.append((o1[pick], (np.float32(8) * d1[pick]).astype(np.float32)))
    away = pin_cases.unit(rng.normal(0, 1, (64, 3)))
    parts.append(((centre + np.float32(2 * bound) * away).astype(np.float32), away))                    # leaving: they miss everything
    o = np.concatenate([p[0] for p in parts]).astype(np.float32)
    d = np.concatenate([p[1] for p in parts]).astype(np.float32)
    assert len(o) <= 2048
    return o, d


@functools.lru_cache(maxsize=None)
def _answers(name, which):
    """The oracle's answers, computed once: (rt_hit records, light pdf or None)."""
    sd = _scene_data(name)
    o, d = _rays(name, which)
    orc = _oracle(name)
    pdf = np.array([orc.light_pdf(o[i], d[i]) for i in range(len(o))], np.float32) if len(orc.light_order()) else None
    hits = _expected_hits(orc, sd, o, d)
    hits.setflags(write=False)
    return hits, pdf


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = rt.Scene(_scene_data(name), **kw)
        return made[key]
    yield get
    for s in made.values():
        s.close()


def _words(rt, hits):
    """The 16 words of each rt_hit with RT_HIT_EXACT_WALK masked out of the flags."""
    w = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 16).copy()
    w[:, 14] &= ~np.uint32(rt.RT_HIT_EXACT_WALK)
    return w


def _first_difference(a, b):
    rows = np.nonzero(np.any(a != b, axis=1))[0]
    return f"{len(rows)} of {len(a)} rays differ, first {rows[:5].tolist()}: {a[rows[0]].tolist()} != {b[rows[0]].tolist()}" if len(rows) else ""


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", list(SCENES))
def test_closest_hits_are_the_oracles_bits(rt, scenes, name, which):
    scene = scenes(name)
    o, d = _rays(name, which)
    want = _words(rt, _answers(name, which)[0])
    fast, st = scene.query_closest(o, d)
    slow, st_ref = scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    print(f"{name}/{which}: {st.rays} rays, {st.exact_walks} exact walks, {st.launches} launches, {st.kernel_ms:.3f} ms; hits {(fast['triangle'] != MISS).sum()}")
    assert st.reference_exact == 1 and st.rays == len(o) and st.invalid_rays == 0
    assert st_ref.exact_walks == len(o) and np.all(slow["flags"] & rt.RT_HIT_EXACT_WALK)
    assert np.array_equal(_words(rt, fast), want), _first_difference(_words(rt, fast), want)
    assert np.array_equal(_words(rt, slow), want), _first_difference(_words(rt, slow), want)
    assert np.array_equal(_words(rt, fast), _words(rt, slow))
    assert int(((fast["flags"] & rt.RT_HIT_EXACT_WALK) != 0).sum()) == st.exact_walks
    if which in ("camera", "bounce"):
        assert st.exact_walks < st.rays          # the fast path ran
    ref = _ref8(name)
    if ref is not None:
        live = _words(rt, _expected_hits(ref, _scene_data(name), o, d))
        assert np.array_equal(_words(rt, fast), live), _first_difference(_words(rt, fast), live)


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", ["sphere_emissive", "practice7_1"])
def test_light_pdfs_are_the_oracles_bits(rt, scenes, name, which):
    scene = scenes(name)
    o, d = _rays(name, which)
    want = _answers(name, which)[1]
    fast, st = scene.query_light_pdf(o, d)
    slow, st_ref = scene.query_light_pdf(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    print(f"{name}/{which}: {st.rays} rays, {st.exact_walks} exact walks, {st.launches} launches, {st.kernel_ms:.3f} ms; nonzero {(fast != 0).sum()}")
    assert st.reference_exact == 1 and st.rays == len(o) and st.invalid_rays == 0 and st_ref.exact_walks == len(o)
    assert fast.dtype == np.float32
    assert np.array_equal(fast.view(np.uint32), want.view(np.uint32)), np.nonzero(fast.view(np.uint32) != want.view(np.uint32))[0][:8]
    assert np.array_equal(slow.view(np.uint32), want.view(np.uint32))
    if which in ("camera", "bounce"):
        assert st.exact_walks < st.rays
    ref = _ref8(name)
    if ref is not None:
        live = np.array([ref.light_pdf(o[i], d[i]) for i in range(len(o))], np.float32)
        assert np.array_equal(fast.view(np.uint32), live.view(np.uint32))


@pytest.mark.parametrize("name", ["sphere_emissive", "practice7_1"])
def test_far_origins_all_take_the_exact_walk(rt, scenes, name):
    scene = scenes(name)
    o, d = _rays(name, "far")
    hits, st = scene.query_closest(o, d)
    assert st.exact_walks == len(o) == st.rays and np.all(hits["flags"] & rt.RT_HIT_EXACT_WALK)
    pdf, st = scene.query_light_pdf(o, d)
    assert st.exact_walks == len(o)


@pytest.mark.parametrize("name", ["sphere_emissive", "practice7_1"])
def test_invalid_rays_are_flagged_and_change_nothing(rt, scenes, name):
    scene = scenes(name)
    o, d = (a[:512].copy() for a in _rays(name, "camera"))
    want_hits, want_pdf = _answers(name, "camera")
    want_hits, want_pdf = want_hits[:512], want_pdf[:512]
    bad = np.arange(3, 512, 7)
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        c = k % 7
        if c == 6:
            d[i] = 0
        else:
            (o if c < 3 else d)[i, c % 3] = poison[(k // 7) % 3]
    d[bad[-1]] = (-0.0, 0.0, -0.0)
    valid = np.ones(512, bool)
    valid[bad] = False
    hits, st = scene.query_closest(o, d)
    assert st.invalid_rays == len(bad) and st.rays == 512
    assert np.array_equal(_words(rt, hits[valid]), _words(rt, want_hits[valid]))
    blank = np.zeros(1, rt.HIT_DTYPE)
    blank["triangle"], blank["flags"] = MISS, rt.RT_HIT_INVALID_RAY
    assert np.all(hits[~valid].view(np.uint32).reshape(-1, 16) == blank.view(np.uint32).reshape(1, 16))
    assert not np.any(hits[valid]["flags"] & rt.RT_HIT_INVALID_RAY)
    hits_ref, st_ref = scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    assert st_ref.invalid_rays == len(bad) and st_ref.exact_walks == 512 - len(bad)
    assert np.array_equal(_words(rt, hits_ref), _words(rt, hits))
    pdf, st = scene.query_light_pdf(o, d)
    assert st.invalid_rays == len(bad)
    assert np.array_equal(pdf[valid].view(np.uint32), want_pdf[valid].view(np.uint32)) and np.all(pdf[~valid].view(np.uint32) == 0)


def _many_rays(name):
    o, d = _camera_rays(_scene_data(name), 96, 64, seed=13)                       # 6,144 rays
    ob, db = _rays(name, "bounce")
    return np.concatenate([o, ob[:512]]), np.concatenate([d, db[:512]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_size_changes_no_answer(rt, scenes, n):
    """Partial waves, the slice rounding to 64 and the steal chunks: the first n rays alone answer as they do inside the larger batch."""
    scene = scenes("sphere_emissive")
    o, d = _many_rays("sphere_emissive")
    all_hits, _ = scene.query_closest(o, d)
    all_pdf, _ = scene.query_light_pdf(o, d)
    hits, st = scene.query_closest(o[:n], d[:n])
    assert st.rays == n and np.array_equal(_words(rt, hits), _words(rt, all_hits[:n]))
    pdf, _ = scene.query_light_pdf(o[:n], d[:n])
    assert np.array_equal(pdf.view(np.uint32), all_pdf[:n].view(np.uint32))
    tail, _ = scene.query_closest(o[-n:], d[-n:])
    assert np.array_equal(_words(rt, tail), _words(rt, all_hits[-n:]))


def test_chunk_seams_change_no_answer(rt, scenes, monkeypatch):
    """A call larger than one staging chunk (RTAMD_QUERY_CHUNK shrinks the chunk, never an answer): same bytes, more launches."""
    scene = scenes("sphere_emissive")
    o, d = _many_rays("sphere_emissive")
    hits, st = scene.query_closest(o, d)
    pdf, st_l = scene.query_light_pdf(o, d)
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "1000")
    hits_c, st_c = scene.query_closest(o, d)
    pdf_c, st_lc = scene.query_light_pdf(o, d)
    chunks = -(-len(o) // 1000)
    assert st_c.launches == chunks * st.launches and st_lc.launches == chunks * st_l.launches
    assert st_c.exact_walks == st.exact_walks and st_c.rays == len(o)
    assert np.array_equal(hits_c.view(np.uint32), hits.view(np.uint32)) and np.array_equal(pdf_c.view(np.uint32), pdf.view(np.uint32))


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
o, d = T._many_rays("sphere_emissive")
for flags in (0, rt.RT_QUERY_REFERENCE_WALK):
    hits, st = scene.query_closest(o, d, flags=flags)
    pdf, _ = scene.query_light_pdf(o, d, flags=flags)
    rays = torch.from_numpy(rt.pack_rays(o, d).view(np.float32).reshape(-1, 6).copy()).cuda()
    out = torch.full((len(o), 16), -1, dtype=torch.int32, device="cuda")
    out_pdf = torch.full((len(o),), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st_d = scene.query_closest_device(rays.data_ptr(), len(o), out.data_ptr(), flags=flags)
    scene.query_light_pdf_device(rays.data_ptr(), len(o), out_pdf.data_ptr(), flags=flags)
    assert st_d.rays == len(o) and st_d.exact_walks == st.exact_walks
    assert np.array_equal(out.cpu().numpy().view(np.uint32), hits.view(np.uint32).reshape(-1, 16))
    assert np.array_equal(out_pdf.cpu().numpy().view(np.uint32), pdf.view(np.uint32))
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with torch tensors as rays and outputs: the same bytes as the host-pointer call.  In a process of its
    own, where torch opens the GPU before the library does (the order bench.py keeps)."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def test_queries_only_read_the_scene(rt, scenes):
    """A render before and after a query gives the same pixels; an rt_accum advanced across a query equals the one-shot frame."""
    scene = scenes("sphere_emissive")
    o, d = _rays("sphere_emissive", "bounce")
    before, before8, _ = scene.render(32, 32, 4)
    acc = scene.accumulator(32, 32)
    acc.render(1)
    scene.query_closest(o, d)
    scene.query_light_pdf(o, d)
    acc.render(3)
    scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    got, got8 = acc.resolve()
    acc.close()
    after, after8, _ = scene.render(32, 32, 4)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and np.array_equal(before8, after8)
    assert np.array_equal(got.view(np.uint32), before.view(np.uint32)) and np.array_equal(got8, before8)


def test_gate_switched_off_says_so(rt, scenes, monkeypatch):
    """RTAMD_NO_EXACT_BOXES at scene creation: reference_exact == 0, the padded boxes' closest triangles on both paths."""
    o, d = _rays("sphere_emissive", "camera")
    host, _ = scenes("sphere_emissive").query_closest(o, d)
    monkeypatch.setenv("RTAMD_NO_EXACT_BOXES", "1")
    scene = rt.Scene(_scene_data("sphere_emissive"))
    try:
        fast, st = scene.query_closest(o, d)
        slow, st_ref = scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
        _, st_pdf = scene.query_light_pdf(o, d)
    finally:
        scene.close()
    assert st.reference_exact == 0 and st_ref.reference_exact == 0 and st_pdf.reference_exact == 0 and st.exact_walks == 0
    assert np.array_equal(_words(rt, fast), _words(rt, slow))
    assert np.array_equal(fast["triangle"], host["triangle"]) and np.array_equal(fast["t"].view(np.uint32), host["t"].view(np.uint32))


def test_device_built_scene_says_so_and_finds_the_same_triangles(rt, scenes):
    """RT_BUILD_DEVICE_BVH: reference_exact == 0; on the camera rays the same t and the same LOAD-order triangle as the host-built scene."""
    o, d = _rays("sphere_emissive", "camera")
    host, st_host = scenes("sphere_emissive").query_closest(o, d)
    dev_scene = scenes("sphere_emissive", build_flags=rt.RT_BUILD_DEVICE_BVH)
    assert dev_scene.info().bvh_on_device == 1
    dev, st = dev_scene.query_closest(o, d)
    slow, st_ref = dev_scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    assert st_host.reference_exact == 1 and st.reference_exact == 0 and st_ref.reference_exact == 0
    assert np.array_equal(dev["t"].view(np.uint32), host["t"].view(np.uint32)) and np.array_equal(dev["triangle"], host["triangle"])
    assert np.array_equal(_words(rt, slow), _words(rt, dev))
    _, st_pdf = dev_scene.query_light_pdf(o, d)
    assert st_pdf.reference_exact == 0

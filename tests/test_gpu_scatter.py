"""The bounce step on the GPU (rt_query_scatter, rt_query_bsdf, rt_trace_paths) against tests/scatter_model.py, which
tests/test_scatter_host.py has pinned to the oracle's render, bit for bit.

Records: the GPU's own rt_hit and rt_surface records of test_gpu_query_surface.py's camera set (48x32) and bounce set (at most
2,048 each), one fresh engine per record seeded 1 + 7919 * i.  The scenes' own records reach the END_BRDF floor but never
RT_SCATTER_END_CLAMP: with unit shading normals and base colours up to 1 the weight stays below about 3 (the pdf is a third of each
component's own).  So every set ends in 2 x 32 constructed rt_surface records, copies of its first 32 hits:
  - metallic 1 x 1 with the shading normal turned away from the viewer: the metal branch is off (v.n < 0) and there is no dielectric
    branch, so the brdf is 0 whatever direction is drawn -- RT_SCATTER_END_BRDF;
  - a fully rough dielectric (alpha 1) with base_color 16, 16, 16: wherever the drawn direction is above the horizon the diffuse
    weight alone is far above 6 -- RT_SCATTER_END_CLAMP with finite numbers (a direction below it, mostly a light sample, is END_BRDF or goes on).
The floors are asserted on the expected table before the scatter under test runs."""
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
import test_gpu_query as tq
import test_gpu_query_surface as tqs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = sc.MISS
F = np.float32
SCENES = ["sphere", "sphere_emissive", "sphere_roughness", "soup_a", "soup_b"]
FRAME_SCENES = ["sphere_emissive_env", "soup_a", "soup_b"]
CONSTRUCTED = 32


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


def _constructed(surf, d):
    """2 x CONSTRUCTED surfaces made of the first CONSTRUCTED ones, hit by rays of direction d (module docstring)."""
    dark, bright = surf[:CONSTRUCTED].copy(), surf[:CONSTRUCTED].copy()
    dark["base_metallic"], dark["metallic"] = 1, 1
    away = (d[:CONSTRUCTED] * dark["sn"]).sum(axis=1) > 0        # v = -d: the viewer is below the horizon of sn
    dark["sn"] = np.where(away[:, None], dark["sn"], -dark["sn"])
    bright["base_metallic"], bright["base_color"], bright["alpha"] = 0, 16, 1
    return dark, bright


def _records(scene, name):
    """Per set ("camera", "bounce"): (o, d, hits, surfaces) of the GPU's own hits, then the constructed records."""
    o1, d1 = tq._camera_rays(sc.scene_data(name))
    cam, _ = scene.query_closest(o1, d1)
    ob, db = tqs._bounce_rays(o1, d1, cam)
    bounce, _ = scene.query_closest(ob, db)
    sets = {}
    for which, (o, d, hits) in {"camera": (o1, d1, cam), "bounce": (ob, db, bounce)}.items():
        on = hits["triangle"] != MISS
        o, d, hits = o[on][:2048 - 2 * CONSTRUCTED], d[on][:2048 - 2 * CONSTRUCTED], hits[on][:2048 - 2 * CONSTRUCTED]
        surf, _ = scene.query_surface(hits)
        assert len(hits) > 100 + CONSTRUCTED and not (surf["material"] == MISS).any()
        head = slice(0, CONSTRUCTED)
        o, d, hits = (np.concatenate([a, a[head], a[head]]) for a in (o, d, hits))
        sets[which] = (np.ascontiguousarray(o), np.ascontiguousarray(d), hits, np.concatenate([surf, *_constructed(surf, d)]))
    return sets


def _engines(n):
    return model.seed(1 + 7919 * np.arange(n))


@pytest.mark.parametrize("name", SCENES)
def test_scatter_is_the_models_bits(rt, scenes, name):
    scene, oracle = scenes(name), sc.oracle(name)
    lights = len(oracle.light_order()) > 0
    ends = np.zeros(2, np.int64)
    for which, (o, d, hits, surf) in _records(scene, name).items():
        n = len(hits)
        want_rng = _engines(n)
        want = model.expected_scatter(oracle, o, d, hits, surf, want_rng)
        # the expected table first, so that the comparison below cannot pass empty
        comps = np.bincount(want["component"], minlength=3)
        flags = want["flags"]
        assert not (flags & (model.NO_SURFACE | model.INVALID)).any()
        assert (flags[-2 * CONSTRUCTED:-CONSTRUCTED] == model.END_BRDF).all(), "the constructed dark records"
        assert (flags[-CONSTRUCTED:] == model.END_CLAMP).sum() >= CONSTRUCTED // 4, "the constructed bright records"
        assert np.isfinite(want["pdf"]).all() and np.isfinite(want["brdf"]).all()
        if lights:
            assert comps.min() >= 100, (which, comps)
        else:
            assert comps[2] == 0 and comps[:2].min() >= 100, (which, comps)
        ends += [(flags == model.END_BRDF).sum(), (flags == model.END_CLAMP).sum()]
        got_rng = _engines(n)
        got, st = scene.query_scatter(o, d, hits, surf, got_rng)
        print(f"{name}/{which}: {n} records, components {comps.tolist()}, END_BRDF {(flags == 1).sum()}, END_CLAMP {(flags == 2).sum()}, "
              f"{st.launches} launches, {st.kernel_ms:.3f} ms, {st.exact_walks} exact walks")
        assert st.rays == n and st.invalid_rays == 0 and st.reference_exact == 1 and st.launches >= (4 if lights else 2)
        assert np.array_equal(sc.words(got), sc.words(want)), sc.first_difference(sc.words(got), sc.words(want))
        assert np.array_equal(sc.words(got_rng), sc.words(want_rng)), sc.first_difference(sc.words(got_rng), sc.words(want_rng))
        # the engine after is at the oracle's stream position: its next uniform is the fifth output of rto_hw8_mix_sample_pdf
        fresh = _engines(n)
        for i in range(0, n - 2 * CONSTRUCTED, 7):
            xo = model.hit_point(o[i], d[i], hits["t"][i], hits["ng"][i])
            ans = oracle.mix_sample_pdf(int(fresh["x"][i]), xo, surf["sn"][i], d[i], float(surf["alpha"][i]))
            one = got_rng[i:i + 1].copy()
            assert rt.rng_uniform(one)[0] == ans[4], i
        # forcing the reference-order light walk changes no byte
        ref_rng = _engines(n)
        ref, st_ref = scene.query_scatter(o, d, hits, surf, ref_rng, flags=rt.RT_QUERY_REFERENCE_WALK)
        assert np.array_equal(sc.words(ref), sc.words(got)) and np.array_equal(ref_rng, got_rng)
        if lights:
            assert st_ref.exact_walks == (flags == 0).sum() + (flags == model.END_CLAMP).sum() >= st.exact_walks
    assert ends.min() >= 8, ends             # per scene, so over all scenes too


@pytest.mark.parametrize("name", ["sphere_emissive", "soup_a"])
def test_a_saved_normal_travels(rt, scenes, name):
    """Two scatters in a row: the second call's rays are the first's (o, d), re-queried; its engines enter with a saved normal
    wherever the first bounce was a cosine sample, and must come out as the model's, which restates rng_n01's saved branch."""
    scene, oracle = scenes(name), sc.oracle(name)
    o, d, hits, surf = _records(scene, name)["camera"]
    keep = slice(0, len(hits) - 2 * CONSTRUCTED)
    o, d, hits, surf = o[keep], d[keep], hits[keep], surf[keep]
    rng = _engines(len(hits))
    first, _ = scene.query_scatter(o, d, hits, surf, rng)
    go = first["flags"] == 0
    o2, d2, rng2 = np.ascontiguousarray(first["o"][go]), np.ascontiguousarray(first["d"][go]), np.ascontiguousarray(rng[go])
    hits2, _ = scene.query_closest(o2, d2)
    surf2, _ = scene.query_surface(hits2)
    want_rng = rng2.copy()
    want = model.expected_scatter(oracle, o2, d2, hits2, surf2, want_rng)
    entered = (rng2["has_saved"] == 1) & (hits2["triangle"] != MISS)
    assert np.array_equal(rng2["has_saved"] == 1, first["component"][go] == 0)
    restated = entered & (want["component"] == 0)
    passed_on = entered & (want["component"] != 0)
    print(f"{name}: {go.sum()} second bounces, {entered.sum()} enter with a saved normal, {restated.sum()} use it, {(want['flags'] == model.NO_SURFACE).sum()} miss")
    assert restated.sum() >= 30 and passed_on.sum() >= 30
    assert not want_rng["has_saved"][restated].any() and np.array_equal(want_rng["saved"][passed_on], rng2["saved"][passed_on])
    got_rng = rng2.copy()
    got, st = scene.query_scatter(o2, d2, hits2, surf2, got_rng)
    assert st.invalid_rays == 0
    assert np.array_equal(sc.words(got), sc.words(want)), sc.first_difference(sc.words(got), sc.words(want))
    assert np.array_equal(sc.words(got_rng), sc.words(want_rng)), sc.first_difference(sc.words(got_rng), sc.words(want_rng))
    nosurf = want["flags"] == model.NO_SURFACE
    assert np.array_equal(got_rng[nosurf], rng2[nosurf])          # a record without a surface leaves its engine alone


@pytest.mark.parametrize("name", ["sphere_roughness", "soup_b"])
def test_bsdf_is_the_scatters_and_the_oracles(rt, scenes, name):
    scene, oracle = scenes(name), sc.oracle(name)
    o, d, hits, surf = _records(scene, name)["bounce"]
    rng = _engines(len(hits))
    scat, _ = scene.query_scatter(o, d, hits, surf, rng)
    brdf, pdf, st = scene.query_bsdf(o, d, hits, surf, scat["d"])
    assert st.rays == len(hits) and st.invalid_rays == 0
    assert np.array_equal(brdf.view(np.uint32), scat["brdf"].view(np.uint32))
    evaluated = scat["flags"] != model.END_BRDF
    assert evaluated.sum() > 100 and (~evaluated).sum() >= CONSTRUCTED
    assert np.array_equal(pdf[evaluated].view(np.uint32), scat["pdf"][evaluated].view(np.uint32))
    assert (scat["pdf"][~evaluated] == 0).all()
    # 1,024 directions of the test's own over the records in turn: half anywhere, half in the hemisphere of the geometric normal
    n = 1024
    turn = np.arange(n) % len(hits)
    o, d, hits, surf = np.ascontiguousarray(o[turn]), np.ascontiguousarray(d[turn]), hits[turn], surf[turn]
    gen = np.random.default_rng(29)
    dirs = pin_cases.unit(gen.normal(0, 1, (n, 3))).astype(F)
    flip = (dirs[n // 2:] * hits["ng"][n // 2:]).sum(axis=1) < 0
    dirs[n // 2:][flip] *= -1
    want_brdf, want_pdf = model.expected_bsdf(oracle, o, d, hits, surf, dirs)
    got_brdf, got_pdf, st = scene.query_bsdf(o, d, hits, surf, dirs)
    ref_brdf, ref_pdf, st_ref = scene.query_bsdf(o, d, hits, surf, dirs, flags=rt.RT_QUERY_REFERENCE_WALK)
    print(f"{name}: {n} directions, {(want_brdf.max(axis=1) > 1e-4).sum()} with a brdf above eps, {(want_pdf > 0).sum()} with a pdf, {st.launches} launches")
    assert (want_brdf.max(axis=1) > 1e-4).sum() > 200 and (want_pdf > 0).sum() > 400
    assert np.array_equal(got_brdf.view(np.uint32), want_brdf.view(np.uint32)), sc.first_difference(got_brdf.view(np.uint32), want_brdf.view(np.uint32))
    assert np.array_equal(got_pdf.view(np.uint32), want_pdf.view(np.uint32)), np.nonzero(got_pdf.view(np.uint32) != want_pdf.view(np.uint32))[0][:8]
    assert np.array_equal(ref_brdf.view(np.uint32), got_brdf.view(np.uint32)) and np.array_equal(ref_pdf.view(np.uint32), got_pdf.view(np.uint32))


FRAMES = [(name, w, h, 6) for name in FRAME_SCENES for w, h in ((24, 16), (16, 24))] + [("soup_a", 24, 16, 2), ("soup_a", 16, 24, 2)]


@pytest.mark.parametrize("name,w,h,depth", FRAMES)
def test_the_frame_from_public_calls_is_rt_renders(rt, scenes, name, w, h, depth):
    """Per pixel rt_rng_seed(y * W + x); per sample two rt_rng_uniform, rt_camera_rays, rt_trace_paths, color = color + L in float32; then
    (float)(1. / samples) * color: every word of rt_render's out_rgb_linear and of Hw8Oracle.render.  The same frame driven by the
    single calls (closest, surface, environment, scatter, fold: scatter_model.trace over the Scene) equals it too, engines included."""
    samples = 4
    scene, oracle = scenes(name), sc.oracle(name)
    _, _, lengths, any_miss, any_hit = model.traced_paths(oracle, w, h, samples, depth)
    assert any_miss and any_hit and len(np.unique(lengths)) >= min(3, depth), np.unique(lengths)
    calls = model.GpuCalls(scene)
    camera = lambda s, xy: scene.camera_rays(w, h, xy)
    launches = []

    def tracer(o, d, rng):
        L, st = scene.trace_paths(o, d, rng, ray_depth=depth)
        assert st.rays == len(o) and st.invalid_rays == 0 and st.reference_exact == 1
        launches.append(st.launches)
        return L
    assert np.array_equal(rt.rng_seed(np.arange(w * h)), model.seed(np.arange(w * h)))
    traced, rng_t = model.frame(calls, camera, w, h, samples, depth, tracer)
    composed, rng_c = model.frame(calls, camera, w, h, samples, depth)
    rendered, _, _ = scene.render(w, h, samples, ray_depth=depth)
    want, _, _ = oracle.render(w, h, samples, ray_depth=depth)
    print(f"{name} {w}x{h} depth {depth}: path lengths {np.unique(lengths).tolist()}, launches per rt_trace_paths call {sorted(set(launches))}")
    words = lambda a: a.reshape(-1, 3).view(np.uint32)
    assert np.array_equal(words(traced), words(rendered)), sc.first_difference(words(traced), words(rendered))
    assert np.array_equal(words(traced), words(want)), sc.first_difference(words(traced), words(want))
    assert np.array_equal(words(composed), words(traced)), sc.first_difference(words(composed), words(traced))
    assert np.array_equal(sc.words(rng_t), sc.words(rng_c)), sc.first_difference(sc.words(rng_t), sc.words(rng_c))
    assert np.isfinite(traced).all() and len(np.unique(traced.reshape(-1, 3), axis=0)) > 32


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seam_case(rt, scene):
    """200 records and 200 paths of soup_a: the digests of all three calls' outputs and engines."""
    o, d = tq._camera_rays(sc.scene_data("soup_a"))
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != MISS
    o2, d2, hits = np.ascontiguousarray(o[on][:200]), np.ascontiguousarray(d[on][:200]), hits[on][:200]
    surf, _ = scene.query_surface(hits)
    r1, r2 = model.seed(1 + 7919 * np.arange(200)), model.seed(5 + 104729 * np.arange(200))
    scat, st_s = scene.query_scatter(o2, d2, hits, surf, r1)
    brdf, pdf, st_b = scene.query_bsdf(o2, d2, hits, surf, scat["d"])
    L, st_t = scene.trace_paths(o[:200], d[:200], r2)
    return _digest(scat, r1, brdf, pdf, L, r2), (st_s.launches, st_b.launches, st_t.launches)


SEAMS = """
import importlib, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import surface_cases as sc
import test_gpu_scatter as t
scene = rt.Scene(sc.scene_data("soup_a"))
digest, launches = t._seam_case(rt, scene)
print("SEAMS", digest, *launches)
"""


def test_chunk_seams_change_no_answer(rt, scenes):
    """RTAMD_QUERY_CHUNK=64 in a fresh child process: four chunks for 200 records or paths, the bytes of the one chunk here."""
    digest, launches = _seam_case(rt, scenes("soup_a"))
    env = dict(os.environ, RTAMD_QUERY_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", SEAMS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SEAMS" in r.stdout, r.stdout + r.stderr
    got = r.stdout.split("SEAMS", 1)[1].split()
    assert got[0] == digest
    assert [int(v) for v in got[1:4]] == [4 * k for k in launches], (got, launches)


DEVICE_POINTERS = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import scatter_model as model
import surface_cases as sc
import test_gpu_query as tq
scene = rt.Scene(sc.scene_data("soup_a"))
o, d = tq._camera_rays(sc.scene_data("soup_a"))
hits, _ = scene.query_closest(o, d)
surf, _ = scene.query_surface(hits)         # misses among them: records without a surface
n = len(o)
rng = model.seed(1 + 7919 * np.arange(n))
scat, st = scene.query_scatter(o, d, hits, surf, rng)
brdf, pdf, _ = scene.query_bsdf(o, d, hits, surf, scat["d"])
rng_p = model.seed(3 + 31 * np.arange(n))
L, st_p = scene.trace_paths(o, d, rng_p)
dev = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()   # words, not floats: no copy may touch a NaN
host = lambda t: t.cpu().numpy().view(np.uint32)
d_rays, d_hits, d_surf = dev(rt.pack_rays(o, d), 6), dev(hits, 16), dev(surf, 16)
d_rng, d_rng_p, d_dirs = dev(model.seed(1 + 7919 * np.arange(n)), 4), dev(model.seed(3 + 31 * np.arange(n)), 4), dev(scat["d"], 3)
d_scat = torch.full((n, 16), -1, dtype=torch.int32, device="cuda")
d_brdf = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
d_pdf = torch.full((n,), -1, dtype=torch.int32, device="cuda")
d_L = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
rays_before = host(d_rays).copy()
st_d = scene.query_scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), d_surf.data_ptr(), d_rng.data_ptr(), n, d_scat.data_ptr())
scene.query_bsdf_device(d_rays.data_ptr(), d_hits.data_ptr(), d_surf.data_ptr(), d_dirs.data_ptr(), n, d_brdf.data_ptr(), d_pdf.data_ptr())
st_pd = scene.trace_paths_device(d_rays.data_ptr(), d_rng_p.data_ptr(), n, d_L.data_ptr())
assert (st_d.rays, st_d.launches, st_d.invalid_rays, st_d.exact_walks) == (n, st.launches, 0, st.exact_walks)
assert (st_pd.launches, st_pd.invalid_rays, st_pd.exact_walks) == (st_p.launches, 0, st_p.exact_walks)
assert np.array_equal(host(d_scat), scat.view(np.uint32).reshape(-1, 16)) and np.array_equal(host(d_rng), rng.view(np.uint32).reshape(-1, 4))
assert np.array_equal(host(d_brdf), brdf.view(np.uint32)) and np.array_equal(host(d_pdf), pdf.view(np.uint32))
assert np.array_equal(host(d_L), L.view(np.uint32)) and np.array_equal(host(d_rng_p), rng_p.view(np.uint32).reshape(-1, 4))
assert np.array_equal(host(d_rays), rays_before)          # rt_trace_paths works on a copy of the caller's rays
P = lambda t, off=0: t.data_ptr() + off
for k in range(4):                                        # each 16-byte array in turn, 4 bytes off
    off = [4 if j == k else 0 for j in range(4)]
    code = rt.lib.rt_query_scatter(scene._h, P(d_rays), P(d_hits, off[0]), P(d_surf, off[1]), P(d_rng, off[2]), 1, rt.RT_QUERY_DEVICE_POINTERS, P(d_scat, off[3]), None)
    msg = rt.lib.rt_last_error().decode()
    assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_query_scatter: ") and "16-byte aligned" in msg, (k, code, msg)
for off in ((8, 0), (0, 4)):
    code = rt.lib.rt_query_bsdf(scene._h, P(d_rays), P(d_hits, off[0]), P(d_surf, off[1]), P(d_dirs), 1, rt.RT_QUERY_DEVICE_POINTERS, P(d_brdf), P(d_pdf), None)
    msg = rt.lib.rt_last_error().decode()
    assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_query_bsdf: ") and "16-byte aligned" in msg, (off, code, msg)
code = rt.lib.rt_trace_paths(scene._h, P(d_rays), P(d_rng_p, 8), 1, 0, rt.RT_QUERY_DEVICE_POINTERS, P(d_L), None)
msg = rt.lib.rt_last_error().decode()
assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_trace_paths: ") and "16-byte aligned" in msg, (code, msg)
assert np.array_equal(host(d_scat), scat.view(np.uint32).reshape(-1, 16)) and np.array_equal(host(d_L), L.view(np.uint32))   # a refusal writes nothing
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with torch tensors for all three calls: the host path's bytes, engines included; misaligned records are
    refused with a message.  In a process of its own, where torch opens the GPU before the library does (the order bench.py keeps)."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def _case(rt, scene, n=256):
    o, d = tq._camera_rays(sc.scene_data("soup_a"))
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != MISS
    o, d, hits = np.ascontiguousarray(o[on][:n]), np.ascontiguousarray(d[on][:n]), hits[on][:n]
    surf, _ = scene.query_surface(hits)
    assert len(hits) == n
    return o, d, hits, surf


def test_hw6_scenes_are_unsupported_and_depth_17_is_over_the_limit(rt, scenes):
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    try:
        o, d = np.zeros((4, 3), F), np.tile(np.array([0, 0, -1], F), (4, 1))
        hits, surf = np.zeros(4, rt.HIT_DTYPE), np.zeros(4, rt.SURFACE_DTYPE)
        for fn, call in (("rt_query_scatter", lambda: hw6.query_scatter(o, d, hits, surf, model.seed(np.arange(4)))),
                         ("rt_query_bsdf", lambda: hw6.query_bsdf(o, d, hits, surf, d)),
                         ("rt_trace_paths", lambda: hw6.trace_paths(o, d, model.seed(np.arange(4))))):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt.RT_ERR_UNSUPPORTED and f"{fn}: " in str(e.value) and "hw8 / hw7" in str(e.value)
    finally:
        hw6.close()
    scene = scenes("soup_a")
    o, d, _, _ = _case(rt, scene, 8)
    rng = model.seed(np.arange(8))
    for depth in (17, 1000):
        with pytest.raises(rt.RtError) as e:
            scene.trace_paths(o, d, rng, ray_depth=depth)
        assert e.value.code == rt.RT_ERR_LIMIT and "rt_trace_paths: ray_depth above 16" in str(e.value)
    assert np.array_equal(rng, model.seed(np.arange(8)))
    deep, st = scene.trace_paths(o, d, rng, ray_depth=16)
    six, _ = scene.trace_paths(o, d, model.seed(np.arange(8)), ray_depth=0)
    six_too, _ = scene.trace_paths(o, d, model.seed(np.arange(8)), ray_depth=6)
    assert np.array_equal(six, six_too) and np.isfinite(deep).all() and st.rays == 8


def test_a_bad_host_engine_is_refused_before_any_launch(rt, scenes):
    scene = scenes("soup_a")
    o, d, hits, surf = _case(rt, scene, 64)
    for bad in (0, 2**31 - 1):
        rng = model.seed(1 + np.arange(64))
        rng["x"][41] = bad
        before = rng.copy()
        out = np.full(64, 0, rt.SCATTER_DTYPE)
        out["reserved"] = 0xABCD
        st = rt.rt_query_stats()
        st.struct_size, st.launches = C.sizeof(st), 77
        code = rt.lib.rt_query_scatter(scene._h, rt.pack_rays(o, d).ctypes.data, hits.ctypes.data, surf.ctypes.data, rng.ctypes.data, 64, 0, out.ctypes.data, C.byref(st))
        msg = rt.lib.rt_last_error().decode()
        assert code == rt.RT_ERR_INVALID_ARG and msg == f"rt_query_scatter: rng[41].x = {bad} is no state of the engine (1 .. 2147483646)"
        assert st.launches == 77 and np.array_equal(rng, before) and (out["reserved"] == 0xABCD).all() and not out["flags"].any()
        with pytest.raises(rt.RtError) as e:
            scene.trace_paths(o, d, rng)
        assert e.value.code == rt.RT_ERR_INVALID_ARG and "rng[41].x" in str(e.value) and np.array_equal(rng, before)


def test_invalid_rays_are_counted_and_records_without_a_surface_are_not(rt, scenes):
    scene = scenes("soup_a")
    o, d, hits, surf = _case(rt, scene)
    n = len(hits)
    clean_rng = _engines(n)
    clean, _ = scene.query_scatter(o, d, hits, surf, clean_rng)
    o2, d2, hits2, surf2 = o.copy(), d.copy(), hits.copy(), surf.copy()
    bad_ray = np.arange(3, n, 17)
    poison = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad_ray):
        c = k % 7
        if c == 6:
            d2[i] = 0
        else:
            (o2 if c < 3 else d2)[i, c % 3] = poison[(k // 7) % 3]
    bad_hit = np.arange(5, n, 19)
    bad_hit = bad_hit[~np.isin(bad_hit, bad_ray)]
    for k, i in enumerate(bad_hit):
        if k % 4 == 0:
            hits2["t"][i] = poison[(k // 4) % 3]
        else:
            hits2["ng"][i, k % 4 - 1] = poison[(k // 4) % 3]
    no_hit = np.arange(7, n, 23)
    hits2["triangle"][no_hit] = MISS                       # a miss is a record without a surface whatever else it holds
    no_mat = np.arange(11, n, 29)
    surf2["material"][no_mat] = MISS
    nosurf = np.union1d(no_hit, no_mat)
    invalid = np.setdiff1d(np.union1d(bad_ray, bad_hit), nosurf)
    off = np.union1d(nosurf, invalid)
    assert len(invalid) >= 20 and len(nosurf) >= 15 and len(np.intersect1d(nosurf, np.union1d(bad_ray, bad_hit))) >= 1
    rng = _engines(n)
    got, st = scene.query_scatter(o2, d2, hits2, surf2, rng)
    assert st.invalid_rays == len(invalid) and st.rays == n
    blank = np.zeros(16, np.uint32)
    for rows, flag in ((invalid, model.INVALID), (nosurf, model.NO_SURFACE)):
        blank[7] = flag
        assert np.all(sc.words(got[rows]) == blank), flag
    assert np.array_equal(rng[off], _engines(n)[off])       # untouched engines
    ok = np.ones(n, bool)
    ok[off] = False
    assert np.array_equal(sc.words(got[ok]), sc.words(clean[ok])) and np.array_equal(rng[ok], clean_rng[ok])
    # rt_query_bsdf: the same records answer zeros; a non-finite or zero direction of the caller's is invalid too
    dirs = clean["d"].copy()
    bad_dir = np.setdiff1d(np.arange(2, n, 31), off)
    dirs[bad_dir[0::3], 0], dirs[bad_dir[1::3], 2] = np.nan, np.inf
    dirs[bad_dir[2::3]] = 0
    brdf, pdf, st_b = scene.query_bsdf(o2, d2, hits2, surf2, dirs)
    zero = np.union1d(off, bad_dir)
    assert st_b.invalid_rays == len(invalid) + len(bad_dir)
    assert not brdf[zero].view(np.uint32).any() and not pdf[zero].view(np.uint32).any()
    ok[bad_dir] = False
    assert np.array_equal(brdf[ok].view(np.uint32), clean["brdf"][ok].view(np.uint32))
    # rt_trace_paths: an invalid ray answers 0, 0, 0 with its engine untouched and is counted, once
    prng = _engines(n)
    clean_L, _ = scene.trace_paths(o, d, prng)
    prng2 = _engines(n)
    L, st_t = scene.trace_paths(o2, d2, prng2)
    assert st_t.invalid_rays == len(bad_ray) and not L[bad_ray].view(np.uint32).any() and np.array_equal(prng2[bad_ray], _engines(n)[bad_ray])
    good = np.ones(n, bool)
    good[bad_ray] = False
    assert np.array_equal(L[good].view(np.uint32), clean_L[good].view(np.uint32)) and np.array_equal(prng2[good], prng[good])


def test_no_records_is_ok_without_a_launch(rt, scenes):
    scene = scenes("sphere")
    e = np.zeros((0, 3), F)
    got, st = scene.query_scatter(e, e, np.zeros(0, rt.HIT_DTYPE), np.zeros(0, rt.SURFACE_DTYPE), model.seed(np.arange(1))[:0].copy())
    assert got.shape == (0,) and (st.rays, st.launches, st.invalid_rays, st.kernel_ms) == (0, 0, 0, 0.0)
    L, st = scene.trace_paths(e, e, model.seed(np.arange(1))[:0].copy())
    assert L.shape == (0, 3) and st.launches == 0
    assert rt.lib.rt_query_scatter(scene._h, None, None, None, None, 0, 0, None, None) == rt.RT_OK
    assert rt.lib.rt_query_bsdf(scene._h, None, None, None, None, 0, 0, None, None, None) == rt.RT_OK
    assert rt.lib.rt_trace_paths(scene._h, None, None, 0, 0, 0, None, None) == rt.RT_OK


def test_nothing_else_moved(rt):
    """An rt_accum's checkpoint is the same bytes before and after the three calls on its scene, device_bytes stays, and the frame
    it goes on to render is the one-shot frame."""
    sd = sc.scene_data("soup_a")
    scene = rt.Scene(sd)
    try:
        acc = scene.accumulator(24, 16)
        acc.render(2)
        blob, bytes_before = acc.save(), scene.info().device_bytes
        o, d, hits, surf = _case(rt, scene, 128)
        scene.query_scatter(o, d, hits, surf, _engines(128))
        scene.query_bsdf(o, d, hits, surf, np.ascontiguousarray(-d))
        scene.trace_paths(o, d, _engines(128))
        assert acc.save() == blob and scene.info().device_bytes == bytes_before
        acc.render(2)
        after, _ = acc.resolve()
        whole, _, _ = scene.render(24, 16, 4)
        assert np.array_equal(after.view(np.uint32), whole.view(np.uint32))
    finally:
        scene.close()

"""rt_render_paths and rt_render_bake next to their referees on synth_room_v1, device pointers, depth 6 (profiles/r30_render_paths.txt):
  A        the 2,073,600 camera-ray records of the 1920x1080 frame (profiles/r28_scatter_paths.txt's): rt_trace_paths and rt_render_paths,
           alternating, kernel time and call time, with rt_render(samples = 1) of the same frame beside them as the floor
  texels   the first hits of the frame's pixel centres as points, irradiance, 16 samples, K = 1 (profiles/r29_bake.txt's): rt_bake and
           rt_render_bake, alternating
  probes   4,096 points on a 16^3 grid inside the room, normal +y, irradiance, 4,096 samples, K = 64: likewise
and the new calls again with RTAMD_QUERY_CHUNK lowered (the library reads it per call): what decides the default chunk.  Every pair is
also compared word for word.  Run by hand:
    python tools/profiling/render_paths.py [--runs 5] [--only A|texels|probes] [--chunks 262144,1048576]"""
import argparse, importlib, os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--only", choices=("A", "texels", "probes"))
ap.add_argument("--chunks", default="262144,1048576")
args = ap.parse_args()
W, H, DEPTH = 1920, 1080, 6

import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
scene = rt.Scene(sd)
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth}; one warm-up call each, then {args.runs} alternating repeats", flush=True)
words = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()


def line(name, st, paths):
    k, t = np.array([s.kernel_ms for s in st]), np.array([s.total_ms for s in st])
    print(f"  {name:34s} kernel_ms median {np.median(k):9.3f} (min {k.min():.3f}, max {k.max():.3f}) = {paths / np.median(k) / 1e3:7.1f} Mpaths/s   "
          f"total_ms median {np.median(t):9.3f} (min {t.min():.3f}, max {t.max():.3f})   launches {st[0].launches}, exact walks {getattr(st[0], 'exact_walks', None)}", flush=True)
    return float(np.median(k)), float(k.min()), float(k.max())


def alternate(calls):
    """calls: name -> call() returning a stats record; one warm-up each, then the repeats in turn."""
    for c in calls.values():
        c()
    st = {name: [] for name in calls}
    for _ in range(args.runs):
        for name, c in calls.items():
            st[name].append(c())
    return st


def with_chunks(name, call, paths):
    for chunk in [int(v) for v in args.chunks.split(",") if v]:
        os.environ["RTAMD_QUERY_CHUNK"] = str(chunk)
        call()
        line(f"{name}, chunk {chunk}", [call() for _ in range(args.runs)], paths)
    os.environ.pop("RTAMD_QUERY_CHUNK", None)


if args.only in (None, "A"):
    n = W * H
    M = 2147483647
    x = (np.arange(n, dtype=np.uint64) % M).astype(np.uint64)
    x[x == 0] = 1
    xy = np.zeros((n, 2), np.float32)
    for c, base in ((0, np.tile(np.arange(W, dtype=np.float32), H)), (1, np.repeat(np.arange(H, dtype=np.float32), W))):
        x = x * np.uint64(48271) % np.uint64(M)
        xy[:, c] = base + np.minimum((x - 1).astype(np.float32) * np.float32(2.0 ** -31), np.float32(0.99999994))
    engines = np.zeros(n, rt.RNG_DTYPE)
    engines["x"] = x
    o, d = scene.camera_rays(W, H, xy)
    d_rays, d_engines = words(rt.pack_rays(o, d), 6), words(engines, 4)
    out = {k: torch.full((n, 3), -1, dtype=torch.int32, device="cuda") for k in ("trace", "render")}
    rng = {k: torch.empty_like(d_engines) for k in out}

    def trace():
        rng["trace"].copy_(d_engines); torch.cuda.synchronize()
        return scene.trace_paths_device(d_rays.data_ptr(), rng["trace"].data_ptr(), n, out["trace"].data_ptr(), ray_depth=DEPTH)

    def render_paths():
        rng["render"].copy_(d_engines); torch.cuda.synchronize()
        return scene.render_paths_device(d_rays.data_ptr(), rng["render"].data_ptr(), n, out["render"].data_ptr(), ray_depth=DEPTH)
    print(f"A: {n} camera-ray records, depth {DEPTH}, device pointers")
    st = alternate({"rt_trace_paths": trace, "rt_render_paths": render_paths,
                    "rt_render(samples = 1)": lambda: scene.render(W, H, 1, want_float=True, want_rgb8=False, ray_depth=DEPTH)[2]})
    a = line("rt_trace_paths", st["rt_trace_paths"], n)
    b = line("rt_render_paths", st["rt_render_paths"], n)
    line("rt_render(samples = 1), the floor", st["rt_render(samples = 1)"], n)
    frame, _, _ = scene.render(W, H, 1, want_rgb8=False, ray_depth=DEPTH)
    same = torch.equal(out["trace"], out["render"]) and torch.equal(rng["trace"], rng["render"])
    print(f"  outputs and engines equal, word for word: {same}; == rt_render(samples 1): {np.array_equal(out['render'].cpu().numpy().view(np.uint32), frame.reshape(-1, 3).view(np.uint32))}")
    print(f"  rt_render_paths = {b[0] / a[0]:.3f} x rt_trace_paths by kernel time; slowest new {b[2]:.3f} ms against fastest referee {a[1]:.3f} ms")
    with_chunks("rt_render_paths", render_paths, n)


def bake_workload(name, points, samples, K):
    n = len(points)
    slots = n * K
    engines = rt.rng_seed(1 + 7919 * np.arange(slots))
    d_points, d_engines = words(points, 6), words(engines, 4)
    out = {k: torch.full((n, 3), -1, dtype=torch.int32, device="cuda") for k in ("bake", "render")}
    rng = {k: torch.empty_like(d_engines) for k in out}

    def bake():
        rng["bake"].copy_(d_engines); torch.cuda.synchronize()
        return scene.bake_device(d_points.data_ptr(), rng["bake"].data_ptr(), n, out["bake"].data_ptr(), samples, K, rt.RT_BAKE_IRRADIANCE, DEPTH)

    def render_bake():
        rng["render"].copy_(d_engines); torch.cuda.synchronize()
        return scene.render_bake_device(d_points.data_ptr(), rng["render"].data_ptr(), n, out["render"].data_ptr(), samples, K, ray_depth=DEPTH)
    paths = n * samples
    print(f"{name}: {n} points, irradiance, {samples} samples, K = {K} ({slots} slots of {samples // K} paths), depth {DEPTH}", flush=True)
    st = alternate({"rt_bake": bake, "rt_render_bake": render_bake})
    a = line("rt_bake", st["rt_bake"], paths)
    b = line("rt_render_bake", st["rt_render_bake"], paths)
    same = torch.equal(out["bake"], out["render"]) and torch.equal(rng["bake"], rng["render"])
    print(f"  outputs and engines equal, word for word: {same}; invalid points {st['rt_bake'][0].invalid_points} and {st['rt_render_bake'][0].invalid_points}")
    print(f"  rt_render_bake = {b[0] / a[0]:.3f} x rt_bake by kernel time; slowest new {b[2]:.3f} ms against fastest referee {a[1]:.3f} ms")
    with_chunks("rt_render_bake", render_bake, paths)


if args.only in (None, "texels"):
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    xy = np.stack([x.reshape(-1) + np.float32(0.5), y.reshape(-1) + np.float32(0.5)], axis=1)
    o, d = scene.camera_rays(W, H, xy)
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != rt.RT_HIT_MISS
    p = (o[on] + hits["t"][on, None] * d[on]).astype(np.float32)
    print(f"texels: {int(on.sum())} of {W * H} pixel centres hit")
    bake_workload("texels", rt.pack_bake_points(p, hits["ng"][on]), 16, 1)
if args.only in (None, "probes"):
    xyz = np.asarray(sd.positions, np.float32).reshape(-1, 3)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    g = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = (lo + (0.1 + 0.8 * grid) * (hi - lo)).astype(np.float32)
    bake_workload("probes", rt.pack_bake_points(pts, np.tile(np.array([0, 1, 0], np.float32), (len(pts), 1))), 4096, 64)
scene.close()

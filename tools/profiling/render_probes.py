"""rt_render_probes next to its referee rt_bake (RT_BAKE_SH9) on synth_room_v1, device pointers, depth 6 (profiles/r34_render_probes.txt):
  probes   4,096 points on a 16^3 grid inside the room, 4,096 samples, K = 64 (profiles/r29_bake.txt's, r30's points)
  texels   the first hits of the 1920x1080 frame's pixel centres as points, 16 samples, K = 1: one full chunk of 2,073,600 slots
One warm-up call each, then the repeats alternate referee and new call in one process; kernel time is the calls' own (HIP events around
their launches).  Outputs and engines are compared word for word in the same run, and rt_render_bake (irradiance) runs on the same
points in the same alternation: what the SH mode costs over it.  Run by hand:
    python tools/profiling/render_probes.py [--runs 5] [--only probes|texels]"""
import argparse, importlib, os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--only", choices=("probes", "texels"))
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
          f"total_ms median {np.median(t):9.3f} (min {t.min():.3f}, max {t.max():.3f})   launches {st[0].launches}, exact walks {st[0].exact_walks}, "
          f"reference_exact {st[0].reference_exact}", flush=True)
    return float(np.median(k)), float(k.min()), float(k.max())


def workload(name, points, samples, K):
    n = len(points)
    slots, paths = n * K, n * samples
    engines = rt.rng_seed(1 + 7919 * np.arange(slots))
    d_points, d_engines = words(points, 6), words(engines, 4)
    out = {k: torch.full((n, 27), -1, dtype=torch.int32, device="cuda") for k in ("bake", "probes")}
    out["irradiance"] = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
    rng = {k: torch.empty_like(d_engines) for k in out}

    def fresh(k):
        rng[k].copy_(d_engines); torch.cuda.synchronize()
        return d_points.data_ptr(), rng[k].data_ptr(), n, out[k].data_ptr()
    calls = {"rt_bake(RT_BAKE_SH9)": lambda: scene.bake_device(*fresh("bake"), samples, K, rt.RT_BAKE_SH9, DEPTH),
             "rt_render_probes": lambda: scene.render_probes_device(*fresh("probes"), samples, K, ray_depth=DEPTH),
             "rt_render_bake (irradiance)": lambda: scene.render_bake_device(*fresh("irradiance"), samples, K, ray_depth=DEPTH)}
    print(f"{name}: {n} points, {samples} samples, K = {K} ({slots} slots of {samples // K} paths), depth {DEPTH}; "
          f"slot state {slots * 144 / 1e6:.1f} MB (24 + 120 bytes a slot), answer {n * 108 / 1e6:.1f} MB", flush=True)
    for c in calls.values():
        c()
    st = {k: [] for k in calls}
    for _ in range(args.runs):
        for k, c in calls.items():
            st[k].append(c())
    a, b, i = (line(k, st[k], paths) for k in calls)
    same = torch.equal(out["bake"], out["probes"]) and torch.equal(rng["bake"], rng["probes"])
    first = st["rt_render_probes"][0]
    print(f"  outputs and engines equal, word for word: {same}; invalid points {st['rt_bake(RT_BAKE_SH9)'][0].invalid_points} and {first.invalid_points}; "
          f"coefficients non-zero: {int((out['probes'] != 0).sum())} of {n * 27}")
    print(f"  rt_render_probes = {b[0] / a[0]:.3f} x rt_bake by kernel time ({a[0] / b[0]:.2f} x faster); slowest new {b[2]:.3f} ms against fastest referee {a[1]:.3f} ms: "
          f"every repeat faster than every repeat of the referee: {b[2] < a[1]}")
    print(f"  the SH mode over rt_render_bake irradiance on the same points: {b[0] / i[0]:.3f} x ({b[0] - i[0]:+.3f} ms)", flush=True)


if args.only in (None, "probes"):
    xyz = np.asarray(sd.positions, np.float32).reshape(-1, 3)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    g = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = (lo + (0.1 + 0.8 * grid) * (hi - lo)).astype(np.float32)
    workload("probes", rt.pack_bake_points(pts, np.tile(np.array([0, 1, 0], np.float32), (len(pts), 1))), 4096, 64)
if args.only in (None, "texels"):
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    xy = np.stack([x.reshape(-1) + np.float32(0.5), y.reshape(-1) + np.float32(0.5)], axis=1)
    o, d = scene.camera_rays(W, H, xy)
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != rt.RT_HIT_MISS
    p = (o[on] + hits["t"][on, None] * d[on]).astype(np.float32)
    print(f"texels: {int(on.sum())} of {W * H} pixel centres hit")
    workload("texels", rt.pack_bake_points(p, hits["ng"][on]), 16, 1)
scene.close()

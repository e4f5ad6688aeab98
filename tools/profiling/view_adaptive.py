"""Adaptive view sets next to the view set and the single-camera adaptive render (profiles/r38_view_adaptive.txt): synth_room_v1,
64 views of 128x128 on an orbit inside the room, depth 6, slices of 16, one MI355X.  The referees are rt_views and rt_adaptive, whose
kernels this feature leaves as they were.
  1  one all-active rt_view_adaptive_render_tiles slice against rt_views_render's slice on the same set, alternating repeats in one
     process: the cost of the update and estimate launches and of the per-sub-tile list
  2  a uniform run to 64 samples a pixel (every sub-tile drawn in each of the 4 slices); per view the worst sub-tile's noise over that
     view's mean luminance.  The largest of them over the views is the target T that the uniform set's worst sub-tile meets, their
     median the target M that the worst sub-tile of a typical view meets.  Then the policy with target_noise = T, and again with M,
     max_samples = 64 and min_batches = 2 (a sub-tile is judged from 32 samples on): camera samples drawn and wall time against the
     uniform rt_views run
  3  the same work (target M) as 64 rt_adaptive objects on 64 scenes, each created with one view's camera: kernel time only,
     rt_scene_create stated apart (every --stride-th camera per run, the sums scaled to 64)
  4  gather_ms, scatter_ms and noise_ms per slice of the runs of 2, as the active fraction falls
Run by hand:
    python tools/profiling/view_adaptive.py [--runs 5] [--stride 8]"""
import argparse, importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--stride", type=int, default=8)
args = ap.parse_args()
N, W, H, DEPTH, SLICE, SPP, MIN_BATCHES = 64, 128, 128, 6, 16, 64, 2

import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
scene = rt.Scene(sd)
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth}; {N} views of {W}x{H}, depth {DEPTH}, slices of {SLICE}", flush=True)
med = lambda v: f"median {np.median(v):9.3f} (min {np.min(v):.3f}, max {np.max(v):.3f})"


def orbit(n, radius, height=3.0, fov_y=0.9):
    """n cameras on a circle of `radius` about the room's axis at `height`, each looking at (0, height, 0): tools/profiling/views.py's."""
    cams = []
    for i in range(n):
        a = 2 * np.pi * i / n
        pos = np.array([radius * np.sin(a), height, radius * np.cos(a)])
        fwd = np.array([-np.sin(a), 0.0, -np.cos(a)])
        up = np.array([0.0, 1.0, 0.0])
        right = np.cross(fwd, up)
        c = rt.rt_camera()
        for k in range(3):
            c.position[k], c.right[k], c.up[k], c.forward[k] = pos[k], right[k], up[k], fwd[k]
        c.fov_y = fov_y
        cams.append(c)
    return cams


def swapped(cam):
    return rt.SceneData(sd.positions, sd.texcoords, sd.normals, sd.tangents, sd.material_index, list(sd.materials)[:sd.n_materials],
                        sd.texture_source, sd.images, rt.rt_camera.from_buffer_copy(cam), sd.bg, sd.environment)


cams = orbit(N, 5.0)

# ---- 1: one all-active slice against rt_views_render ---------------------------------------------------------------------------------------
plain = scene.views(W, H, cams, ray_depth=DEPTH)
views = scene.adaptive_views(W, H, cams, 1.0, ray_depth=DEPTH)
ones = np.ones((N,) + views.grid, np.uint8)
plain.render(SLICE); views.render_tiles(SLICE, ones)      # one warm-up slice each
ref, new = [], []
for _ in range(args.runs):
    st = plain.render(SLICE); ref.append((st.kernel_ms, st.total_ms, st.gather_ms, st.scatter_ms, st.launches))
    st = views.render_tiles(SLICE, ones); new.append((st.kernel_ms, st.total_ms, st.gather_ms, st.scatter_ms, st.noise_ms, st.launches))
ref, new = np.array(ref), np.array(new)
same = all(np.array_equal(plain.resolve(v)[1], views.resolve(v)[1]) for v in range(N))
print(f"1. one slice of {SLICE} samples, every sub-tile of every view active ({ones.size} sub-tiles), {args.runs} alternating repeats after one warm-up slice each")
print(f"  rt_views_render (referee)        kernel_ms {med(ref[:, 0])}   total_ms {med(ref[:, 1])}   gather_ms {med(ref[:, 2])}   scatter_ms {med(ref[:, 3])}   launches {int(ref[0, 4])}")
print(f"  rt_view_adaptive_render_tiles    kernel_ms {med(new[:, 0])}   total_ms {med(new[:, 1])}   gather_ms {med(new[:, 2])}   scatter_ms {med(new[:, 3])}   launches {int(new[0, 5])}")
print(f"    noise_ms (update + estimate) {med(new[:, 4])}")
print(f"  whole call: {np.median(new[:, 1]) / np.median(ref[:, 1]):.3f} x ({np.median(new[:, 1]) - np.median(ref[:, 1]):+.3f} ms); pictures after {(args.runs + 1) * SLICE} samples equal: {same}", flush=True)
plain.close(); views.close()

# ---- 2 and 4: uniform to SPP, then the policy at the uniform set's worst sub-tile noise -----------------------------------------------------
uniform = []
for _ in range(args.runs):
    plain = scene.views(W, H, cams, ray_depth=DEPTH)
    t0 = time.perf_counter()
    kernel = sum(plain.render(SLICE).kernel_ms for _ in range(SPP // SLICE))
    uniform.append(((time.perf_counter() - t0) * 1e3, kernel))
    plain.close()
uniform = np.array(uniform)
views = scene.adaptive_views(W, H, cams, 1.0, ray_depth=DEPTH)
for _ in range(SPP // SLICE):
    views.render_tiles(SLICE, ones)
worst = [views.noise(v, want_map=False)[1].worst_tile_noise for v in range(N)]
views.close()
T, M = float(np.float32(max(worst))), float(np.float32(np.median(worst)))
print(f"2. uniform rt_views, {SPP // SLICE} slices of {SLICE}: {N * W * H * SPP} camera samples, wall ms {med(uniform[:, 0])} (kernels {med(uniform[:, 1])}); "
      f"worst sub-tile noise over its view's mean luminance: {min(worst):.6g} .. {max(worst):.6g} over the views (median {np.median(worst):.6g}), T = {T:.9g}, M = {M:.9g}", flush=True)


def policy(T, name):
    runs, per_slice = [], None
    for _ in range(args.runs):
        views = scene.adaptive_views(W, H, cams, T, min_batches=MIN_BATCHES, max_samples=SPP, ray_depth=DEPTH)
        t0 = time.perf_counter()
        stats = []
        while True:
            st = views.render(SLICE)
            if st.samples == 0:
                break
            stats.append((st.active_views, st.active_tiles, st.samples, st.kernel_ms, st.gather_ms, st.scatter_ms, st.noise_ms, st.total_ms, st.launches))
        wall = (time.perf_counter() - t0) * 1e3
        stats = np.array(stats)
        runs.append((wall, stats[:, 2].sum(), stats[:, 3].sum(), stats[:, 4].sum() + stats[:, 5].sum(), stats[:, 6].sum(), len(stats)))
        if per_slice is None:
            per_slice = stats
            tiles = np.stack([views.tiles(v) for v in range(N)])
            left = [views.noise(v, want_map=False)[1].worst_tile_noise for v in range(N)]
        views.close()
    runs = np.array(runs)
    drawn = int(runs[0, 1])
    print(f"  policy, target_noise = {name} = {T:.6g}, min_batches {MIN_BATCHES}, max_samples {SPP}: {int(runs[0, 5])} slices, {drawn} camera samples ({drawn / (N * W * H * SPP):.3f} of the uniform run's)")
    print(f"    wall ms {med(runs[:, 0])} ({np.median(runs[:, 0]) / np.median(uniform[:, 0]):.3f} x the uniform rt_views run); kernels {med(runs[:, 2])}; gather + scatter {med(runs[:, 3])}; noise {med(runs[:, 4])}")
    counts, k = np.unique(tiles["samples"], return_counts=True)
    print(f"    sub-tiles converged {int(((tiles['flags'] & rt.RT_ADAPTIVE_CONVERGED) != 0).sum())}, capped {int(((tiles['flags'] & rt.RT_ADAPTIVE_CAPPED) != 0).sum())} of {tiles.size}; "
          f"by sample count: " + ", ".join(f"{int(c)}: {int(n)}" for c, n in zip(counts, k)) + f"; worst sub-tile noise at the end {max(left):.6g} ({max(left) / T:.3f} {name})")
    per_view = tiles["samples"].reshape(N, -1).mean(axis=1)
    print(f"    mean samples per pixel slot by view: min {per_view.min():.1f}, median {np.median(per_view):.1f}, max {per_view.max():.1f}")
    print(f"4. per slice of the first such run, target {name} (active views, active sub-tiles of {ones.size}, kernel_ms, gather_ms, scatter_ms, noise_ms, total_ms, launches):")
    for s in per_slice:
        print(f"    {int(s[0]):3d} {int(s[1]):6d} ({s[1] / ones.size:.3f})  kernel {s[3]:8.3f}  gather {s[4]:.3f}  scatter {s[5]:.3f}  noise {s[6]:.3f}  total {s[7]:8.3f}  launches {int(s[8])}")
    sys.stdout.flush()
    return runs


policy(T, "T")
runs = policy(M, "M")
T = M   # section 3 repeats the second run


# ---- 3: the same work as one rt_adaptive per camera, each on a scene of its own ----------------------------------------------------------------
subset = list(range(0, N, args.stride))
create_ms = kernel_ms = wall_ms = 0.0
drawn_own, equal = 0, 0
check = scene.adaptive_views(W, H, cams, T, min_batches=MIN_BATCHES, max_samples=SPP, ray_depth=DEPTH)
while check.render(SLICE).samples:
    pass
for i in subset:
    data = swapped(cams[i])
    t0 = time.perf_counter(); own = rt.Scene(data); create_ms += (time.perf_counter() - t0) * 1e3
    a = own.adaptive(W, H, T, min_batches=MIN_BATCHES, max_samples=SPP, ray_depth=DEPTH)
    t0 = time.perf_counter()
    while True:
        st = a.render(SLICE)
        if st.samples == 0:
            break
        kernel_ms += st.kernel_ms; drawn_own += st.samples
    wall_ms += (time.perf_counter() - t0) * 1e3
    equal += int(np.array_equal(a.resolve()[1], check.resolve(i)[1]) and np.array_equal(a.sample_map(), check.sample_map(i)))
    a.close(); own.close()
check.close()
scale = N / len(subset)
print(f"3. target M; one rt_adaptive per camera on a scene created with it, {len(subset)} of the {N} cameras, sums scaled by {scale:g}: rt_scene_create {create_ms * scale:.1f} ms; "
      f"render kernels {kernel_ms * scale:.1f} ms, the loops' wall {wall_ms * scale:.1f} ms; camera samples {int(drawn_own * scale)}; "
      f"pictures and sample maps equal to the set's views: {equal} of {len(subset)}")
print(f"  the set's kernels / these kernels: {np.median(runs[:, 2]) / (kernel_ms * scale):.3f} x; the set's wall / these loops' wall: {np.median(runs[:, 0]) / (wall_ms * scale):.3f} x", flush=True)
scene.close()

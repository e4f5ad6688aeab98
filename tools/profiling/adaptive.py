"""Adaptive sampling next to the uniform resumable render on the headline frame (profiles/r35_adaptive.txt, sections a and b):
synth_room_v1, 1920x1080, depth 6, slices of 16, one MI355X.
  a  the price of the detour: one all-active rt_adaptive_render_tiles slice (gather, the persistent kernel over the strip, scatter,
     update, estimate) against one rt_accum_render slice of the same samples, the referee; alternating repeats in one process
  b  the point of it: a uniform rt_accum + rt_noise loop to 256 spp, whose final worst_tile_noise is the target T; then the adaptive loop
     with target_noise = T, min_batches = 4, max_samples = 256, without and with RT_ADAPTIVE_DILATE: camera samples drawn, wall time,
     the histogram of the sub-tiles' sample counts, and the worst sub-tile's noise at the end
Run by hand:
    python tools/profiling/adaptive.py [--runs 5] [--spp 256] [--slice 16]"""
import argparse, importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--slice", type=int, default=16)
args = ap.parse_args()
W, H, DEPTH, SLICE, SPP = 1920, 1080, 6, args.slice, args.spp

import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
scene = rt.Scene(sd)
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth}; {W}x{H}, depth {DEPTH}, slices of {SLICE}", flush=True)
med = lambda v: f"median {np.median(v):9.3f} (min {np.min(v):.3f}, max {np.max(v):.3f})"

# ---- a: one slice, all sub-tiles active, against rt_accum_render ---------------------------------------------------------------------------
acc = scene.accumulator(W, H, ray_depth=DEPTH)
ad = scene.adaptive(W, H, 1.0, ray_depth=DEPTH)
ones = np.ones(ad.grid, np.uint8)
acc.render(SLICE); ad.render_tiles(SLICE, ones)     # one warm-up slice each
ref, new = [], []
for _ in range(args.runs):
    t0 = time.perf_counter(); st = acc.render(SLICE); ref.append((st.kernel_ms, (time.perf_counter() - t0) * 1e3))
    st = ad.render_tiles(SLICE, ones); new.append((st.kernel_ms, st.total_ms, st.gather_ms, st.scatter_ms, st.launches))
ref, new = np.array(ref), np.array(new)
same = np.array_equal(acc.resolve()[1], ad.resolve()[1])
print(f"a. one slice of {SLICE} samples, every sub-tile active ({ones.size} sub-tiles), {args.runs} alternating repeats after one warm-up slice each")
print(f"  rt_accum_render (referee)      kernel_ms {med(ref[:, 0])}   total_ms {med(ref[:, 1])}")
print(f"  rt_adaptive_render_tiles       kernel_ms {med(new[:, 0])}   total_ms {med(new[:, 1])}   launches {int(new[0, 4])}")
print(f"    of which gather_ms {med(new[:, 2])}   scatter_ms {med(new[:, 3])}")
print(f"  persistent kernel over the strip / over the frame: {np.median(new[:, 0]) / np.median(ref[:, 0]):.3f} x; whole call: {np.median(new[:, 1]) / np.median(ref[:, 1]):.3f} x "
      f"({np.median(new[:, 1]) - np.median(ref[:, 1]):+.3f} ms); pictures after {(args.runs + 1) * SLICE} samples equal: {same}", flush=True)
acc.close(); ad.close()

# ---- b: uniform to SPP, then adaptive at the uniform run's worst sub-tile noise -------------------------------------------------------------
acc = scene.accumulator(W, H, ray_depth=DEPTH)
mon = acc.noise_monitor()
t0 = time.perf_counter()
kernel = 0.0
for k in range(SPP // SLICE):
    kernel += acc.render(SLICE).kernel_ms
    mon.update()
    if k >= 1:
        _, s = mon.estimate(want_map=False)
uniform_ms = (time.perf_counter() - t0) * 1e3
T = s.worst_tile_noise
print(f"b. uniform rt_accum + rt_noise, {SPP // SLICE} slices of {SLICE}: {W * H * SPP} camera samples, wall {uniform_ms:.1f} ms (render kernels {kernel:.1f} ms); "
      f"noise {s.noise:.6g}, worst_tile_noise T = {T:.9g}", flush=True)
acc.close()
for dilate in (False, True):
    ad = scene.adaptive(W, H, T, min_batches=4, max_samples=SPP, dilate=dilate, ray_depth=DEPTH)
    t0 = time.perf_counter()
    drawn, kernel, detour, slices, active = 0, 0.0, 0.0, 0, []
    while True:
        st = ad.render(SLICE)
        if st.samples == 0:
            break
        drawn += st.samples; kernel += st.kernel_ms; detour += st.gather_ms + st.scatter_ms; slices += 1; active.append(st.active_tiles)
    wall = (time.perf_counter() - t0) * 1e3
    tiles = ad.tiles()
    _, s = ad.noise(want_map=False)
    worst = float(np.nanmax(np.sqrt(tiles["sum_se2"].astype(np.float64) / np.maximum(tiles["pixels"], 1)))) / s.mean_luminance
    counts, n = np.unique(tiles["samples"], return_counts=True)
    print(f"  adaptive, target_noise = T, min_batches 4, max_samples {SPP}, dilate {int(dilate)}: {slices} slices, {drawn} camera samples "
          f"({drawn / (W * H * SPP):.3f} of the uniform run's), wall {wall:.1f} ms ({wall / uniform_ms:.3f} x the uniform loop; render kernels {kernel:.1f} ms, gather + scatter {detour:.1f} ms)")
    print(f"    sub-tiles converged {int(((tiles['flags'] & rt.RT_ADAPTIVE_CONVERGED) != 0).sum())}, capped {int(((tiles['flags'] & rt.RT_ADAPTIVE_CAPPED) != 0).sum())} of {tiles.size}; "
          f"worst sub-tile noise at the end {worst:.9g} ({worst / T:.3f} T); frame noise {s.noise:.6g}")
    print(f"    active sub-tiles per slice: {active}")
    print(f"    sub-tiles by sample count: " + ", ".join(f"{int(c)}: {int(k)}" for c, k in zip(counts, n)), flush=True)
    ad.close()
scene.close()

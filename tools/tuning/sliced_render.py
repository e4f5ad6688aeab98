#!/usr/bin/env python3
"""Cost of rendering the headline frame (synth_room_v1, 1920x1080x256) in slices: wall time of the whole sequence, one resolve to the
host per slice included, against the one-shot render of the same frame.

usage: sliced_render.py [--workload NAME] [--repeats R] [--oneshot] [--slices N ...] [--monitor]
  --oneshot    time Scene.render (works with a library that has no rt_accum_*: point RTAMD_LIB at it, or run a copy of this script
               inside a checkout of the commit to compare with)
  --slices N   time an Accumulator advanced in slices of N samples (several N: one after the other)
  --monitor    with a NoiseMonitor updated and estimated (summary only) after every slice; its share of the wall time is printed
Every configuration is rendered once untimed first (allocations, code objects), then R times; all R times are printed."""
import argparse
import importlib
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
WORKLOADS = {"synth_room_v1_1920x1080x256": dict(width=1920, height=1080, spp=256, spheres=64, segs=50, rings=43),   # bench.py's
             "synth_room_small_320x180x16": dict(width=320, height=180, spp=16, spheres=8, segs=12, rings=9)}
ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="synth_room_v1_1920x1080x256", choices=sorted(WORKLOADS))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--oneshot", action="store_true")
ap.add_argument("--slices", type=int, nargs="*", default=[])
ap.add_argument("--monitor", action="store_true")
a = ap.parse_args()
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room

wl = WORKLOADS[a.workload]
W, H, SPP = wl["width"], wl["height"], wl["spp"]
gltf, _ = gen_synth_room.generate(tempfile.mkdtemp(prefix="synth_room_"), wl["spheres"], wl["segs"], wl["rings"])
scene = rt.Scene(rt.load_gltf(gltf))
print(f"# {a.workload}, library {rt.LIB_PATH}", flush=True)
if a.oneshot:
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        _, _, st = scene.render(W, H, SPP)
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            print(f"one-shot run {rep}: wall {wall:.1f} ms, kernel {st.kernel_ms:.1f} ms, {st.launches} launches", flush=True)
for n in a.slices:
    for rep in range(a.repeats + 1):
        acc = scene.accumulator(W, H)
        mon = acc.noise_monitor() if a.monitor else None
        per_slice, resolve_ms, monitor_ms, noise = [], 0.0, 0.0, None
        t0 = time.perf_counter()
        while acc.samples < SPP:
            st = acc.render(min(n, SPP - acc.samples))
            per_slice.append(st.kernel_ms)
            t1 = time.perf_counter()
            if mon:
                mon.update()
                if mon.batches >= 2:
                    noise = mon.estimate(want_map=False)[1].noise
                monitor_ms += (time.perf_counter() - t1) * 1e3
                t1 = time.perf_counter()
            acc.resolve()
            resolve_ms += (time.perf_counter() - t1) * 1e3
        wall = (time.perf_counter() - t0) * 1e3
        acc.close()
        if rep:
            if mon:
                print(f"slices of {n} run {rep}: monitor {monitor_ms:.2f} ms of the wall time ({monitor_ms / len(per_slice):.3f} ms per slice: one update, one estimate), last noise {noise!r}", flush=True)
            print(f"slices of {n}{' monitored' if mon else ''} run {rep}: wall {wall:.1f} ms ({len(per_slice)} slices, resolves {resolve_ms:.1f} ms of it), kernel_ms per slice: "
                  + " ".join(f"{k:.1f}" for k in per_slice) + f" (sum {sum(per_slice):.1f}), {st.launches} launches per slice", flush=True)
    p = rt.make_params(W, H, 0)
    state = rt.lib.rt_accum_state_bytes(p)
    print(f"slices of {n}: state {state / 1e6:.1f} MB, read and written once per slice = {2 * state / 1e6:.1f} MB per slice", flush=True)
scene.close()

#!/usr/bin/env python3
"""Cost of the resumable render on several device entries (rt_multi_accum_*) on the headline frame (synth_room_v1, 1920x1080x256):
the frame in slices with one resolve to the host per slice, through a plain Accumulator and through a MultiAccumulator on each device
list, against MultiScene.render one-shot on the same lists; then the time of save and of load (a ~50 MB checkpoint).

usage: multi_sliced_render.py [--workload NAME] [--rounds R] [--slice N] [--lists 0 0,0 ...] [--single-only]
  --single-only   the plain Accumulator alone (works with a library that has no rt_multi_accum_*: point RTAMD_LIB at it)
Everything is rendered once untimed first; then R rounds, each configuration once per round in turn, every time printed.
The lists repeat device indices as given: "0,0" is two shards on ONE physical GPU, not two GPUs."""
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--slice", type=int, default=64)
ap.add_argument("--lists", nargs="*", default=["0", "0,0"])
ap.add_argument("--single-only", action="store_true")
a = ap.parse_args()
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room

wl = WORKLOADS[a.workload]
W, H, SPP = wl["width"], wl["height"], wl["spp"]
gltf, _ = gen_synth_room.generate(tempfile.mkdtemp(prefix="synth_room_"), wl["spheres"], wl["segs"], wl["rings"])
sd = rt.load_gltf(gltf)
print(f"# {a.workload}, library {rt.LIB_PATH}, slices of {a.slice}", flush=True)


def sliced(make, label, timed):
    acc = make()
    per_slice = []
    t0 = time.perf_counter()
    while acc.samples < SPP:
        per_slice.append(acc.render(min(a.slice, SPP - acc.samples)).kernel_ms)
        acc.resolve()
    wall = (time.perf_counter() - t0) * 1e3
    if timed:
        print(f"{label}: wall {wall:.1f} ms ({len(per_slice)} slices, a resolve to the host after each), kernel_ms per slice: "
              + " ".join(f"{k:.1f}" for k in per_slice), flush=True)
    return acc


def save_load(acc, label):
    for rep in range(4):
        t0 = time.perf_counter()
        blob = acc.save()
        t1 = time.perf_counter()
        acc.load(blob)
        t2 = time.perf_counter()
        if rep:
            print(f"{label}: save {(t1 - t0) * 1e3:.1f} ms, load {(t2 - t1) * 1e3:.1f} ms, {len(blob) / 1e6:.1f} MB", flush=True)


scene = rt.Scene(sd)
multis = {} if a.single_only else {names: rt.MultiScene(sd, [int(x) for x in names.split(",")]) for names in a.lists}
for rnd in range(a.rounds + 1):
    acc = sliced(lambda: scene.accumulator(W, H), f"rt_accum round {rnd}", rnd)
    if rnd == a.rounds:
        save_load(acc, "rt_accum")
    acc.close()
    for names, m in multis.items():
        acc = sliced(lambda: m.accumulator(W, H), f"rt_multi_accum [{names}] round {rnd}", rnd)
        if rnd == a.rounds:
            save_load(acc, f"rt_multi_accum [{names}]")
        acc.close()
        t0 = time.perf_counter()
        _, _, st = m.render(W, H, SPP)
        if rnd:
            print(f"rt_multi_render [{names}] round {rnd}: wall {(time.perf_counter() - t0) * 1e3:.1f} ms, slowest device's kernels {st.kernel_ms:.1f} ms", flush=True)
for m in multis.values():
    m.close()
scene.close()

#!/usr/bin/env python3
"""The headline frame (synth_room_v1, 1920x1080x256) rendered in four slices of 64 samples against the one-shot frame that
`python bench.py --dump-outputs DIR` wrote: every dumped float and byte must be equal.

usage: validate_sliced_headline.py DIR [--slice 64]"""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("dump_dir")
ap.add_argument("--slice", type=int, default=64)
a = ap.parse_args()
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room

W, H, SPP = 1920, 1080, 256
gltf, _ = gen_synth_room.generate(tempfile.mkdtemp(prefix="synth_room_"), 64, 50, 43)   # bench.py's synth_room_v1
scene = rt.Scene(rt.load_gltf(gltf))
acc = scene.accumulator(W, H)
while acc.samples < SPP:
    st = acc.render(min(a.slice, SPP - acc.samples))
    print(f"{acc.samples} of {SPP} samples, slice kernel {st.kernel_ms:.1f} ms", flush=True)
rgb, rgb8 = acc.resolve()
acc.close()
scene.close()
import bench  # dump_sample: a dump larger than bench.py's budget keeps a fixed, seeded sample of the flat elements
bad = {}
for name, mine in (("rgb", rgb), ("rgb8", rgb8)):
    ref = np.load(os.path.join(a.dump_dir, name + ".npy")).reshape(-1)
    mine = np.asarray(mine, dtype=np.float32).reshape(-1)
    if ref.size != mine.size:
        mine = mine[bench.dump_sample(mine.size, ref.size)]
    bad[name] = int((~((mine == ref) | (np.isnan(mine) & np.isnan(ref)))).sum())
    print(f"sliced headline frame ({SPP} = {-(-SPP // a.slice)} slices of {a.slice}) against the one-shot dump, {name}: {bad[name]} of {ref.size} dumped elements differ")
sys.exit(1 if any(bad.values()) else 0)

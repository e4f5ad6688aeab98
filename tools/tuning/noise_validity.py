#!/usr/bin/env python3
"""How close the noise monitor's estimate comes to the error it estimates: the sphere scene at 96x64, d samples in slices, against a
frame of many more samples of the same scene.  The picture's actual luminance RMS error (against the reference frame) is compared with
rms_error * sqrt(1 + d / REF): the factor accounts for the reference frame's own variance.  Under replay mode all samples of a pixel
share one stream (the reference frame CONTINUES the picture's streams), so this is one realisation, not an average.

usage: noise_validity.py [--ref 4096]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--ref", type=int, default=4096)
a = ap.parse_args()
rt = importlib.import_module("raytracing-course-hw_amd")
W, H = 96, 64
scene = rt.Scene(rt.load_gltf(os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")))
luma = lambda rgb: rgb.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
ref = luma(scene.render(W, H, a.ref, want_rgb8=False)[0])
for d, slices in ((64, 8), (256, 16)):
    acc = scene.accumulator(W, H)
    mon = acc.noise_monitor()
    for _ in range(slices):
        acc.render(d // slices)
        mon.update()
    se, s = mon.estimate()
    pic = luma(acc.resolve(want_rgb8=False)[0])
    acc.close()
    actual = float(np.sqrt(np.mean((pic - ref) ** 2)))
    # the reference frame holds the picture's own d samples: picture - reference = (1 - d/REF) * (mean of d - mean of the other REF - d),
    # whose variance is sigma^2 / d * (1 - d/REF); the plain factor sqrt(1 + d/REF) would fit a reference of independent samples
    predicted_indep = s.rms_error * np.sqrt(1 + d / a.ref)
    predicted_shared = s.rms_error * np.sqrt(1 - d / a.ref)
    print(f"d = {d} in {slices} slices of {d // slices}: estimated rms_error {s.rms_error:.6g}, noise {s.noise:.6g}, worst tile {s.worst_tile_noise:.6g}; "
          f"actual RMS luminance error against {a.ref} samples {actual:.6g}; ratio actual / (rms_error * sqrt(1 + d/{a.ref})) = {actual / predicted_indep:.4f}, "
          f"actual / (rms_error * sqrt(1 - d/{a.ref})) = {actual / predicted_shared:.4f}", flush=True)
scene.close()

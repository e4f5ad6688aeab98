"""Batched ray queries (rt_query_closest / rt_query_light_pdf / rt_query_occluded) on synth_room_v1: the camera rays of the 1920x1080 frame (coherent) and one
bounce ray from each of their hit points (incoherent), each set on the fast path and with RT_QUERY_REFERENCE_WALK.  Per run: Mrays/s by
kernel time (HIP events around the chunk's kernels) and by wall time of the call (host arrays: staging copies included), and the share of
rays answered by the reference-order walk.  Fast and forced answers are compared bit for bit.  For scale: the closest-hit rate of the
round pipeline's own render (RTAMD_KERNEL=wavefront, RT_FLAG_COUNTERS): closest_hit_queries / dominant_kernel_ms -- its traverse launches
walk the light queries of the same rounds too, so that figure is a floor.  Then rt_query_occluded against rt_query_closest on the same rays,
alternating in this process, for tmax = none, 0.5 T (nothing occluded: a full walk cut at the bound) and 2 T (everything occluded: an early
exit), T being the ray's closest t; per set the exact-walk share and the fast path compared with its reference walk bit for bit.  Run by hand:
    python tools/profiling/ray_queries.py [--runs 3] [--no-resources | --resources-only]
--resources-only needs no GPU: it compiles rtamd_api.hip for the device with -Rpass-analysis=kernel-resource-usage and prints VGPRs,
scratch, LDS and occupancy of the rq_* kernels."""
import argparse, importlib, os, re, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--resources-only", action="store_true")
args = ap.parse_args()


def resources():
    import test_kernel_resources as tk  # the Makefile's flags, as the budget test reads them
    csrc = os.path.join(ROOT, "raytracing-course-hw_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([tk.HIPCC] + tk._makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "rtamd_api.hip",
                            "-o", os.path.join(tmp, "api.o")], cwd=csrc, stderr=subprocess.PIPE, text=True, check=True)
    name, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?\d+(rq_\w+?kernel)(ILb([01])E)?", line)
        if "Function Name" in line:
            name = (m.group(1) + ("<SPILL>" if m.group(3) == "1" and m.group(1) in ("rq_closest_kernel", "rq_any_kernel") else "<light>" if m.group(3) == "1" else "")) if m else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            rows.setdefault(name, {})[m.group(1).split(" [")[0]] = int(m.group(2))
    print("kernel resources (gfx950, the Makefile's flags):")
    for k in sorted(rows):
        u = rows[k]
        print(f"  {k:32s} VGPRs {u['VGPRs']:3d}  scratch {u['ScratchSize']:4d} B/lane  LDS {u['LDS Size']:6d} B/block  occupancy {u['Occupancy']} waves/SIMD")


if not args.no_resources:
    resources()
if args.resources_only:
    sys.exit(0)

rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
import test_gpu_query as tq  # the tests' camera-ray generator
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
scene = rt.Scene(sd)
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth} / light tree {info.light_bvh_depth}")
W, H = 1920, 1080
o1, d1 = tq._camera_rays(sd, W, H, seed=1)


def run(label, fn, o, d, flags):
    best = None
    for _ in range(args.runs):
        out, st = fn(o, d, flags=flags)
        if best is None or st.kernel_ms < best[1].kernel_ms:
            best = (out, st)
    out, st = best
    mode = "reference walk" if flags & rt.RT_QUERY_REFERENCE_WALK else "fast path     "
    print(f"  {label:28s} {mode} {st.rays:8d} rays  kernels {st.kernel_ms:9.3f} ms = {st.rays / st.kernel_ms / 1e3:8.1f} Mrays/s   call {st.total_ms:8.1f} ms = "
          f"{st.rays / st.total_ms / 1e3:6.1f} Mrays/s   exact walks {st.exact_walks} ({100.0 * st.exact_walks / max(1, st.rays):.4f} %)  launches {st.launches}", flush=True)
    return out


def both(label, fn, o, d):
    fast = run(label, fn, o, d, 0)
    slow = run(label, fn, o, d, rt.RT_QUERY_REFERENCE_WALK)
    a, b = fast.view(np.uint32).reshape(len(o), -1).copy(), slow.view(np.uint32).reshape(len(o), -1).copy()
    if a.shape[1] == 16:
        a[:, 14] &= ~np.uint32(rt.RT_HIT_EXACT_WALK); b[:, 14] &= ~np.uint32(rt.RT_HIT_EXACT_WALK)
    print(f"  {label:28s} fast path == reference walk, bit for bit: {bool(np.array_equal(a, b))} ({int(np.any(a != b, axis=1).sum())} rays differ)", flush=True)
    return fast


print(f"best of {args.runs} by kernel time; host arrays in, host arrays out")
hits = both("closest, camera (coherent)", scene.query_closest, o1, d1)
on = hits["triangle"] != rt.RT_HIT_MISS
x = (o1[on] + hits["t"][on, None] * d1[on] + np.float32(1e-4) * hits["ng"][on]).astype(np.float32)
rng = np.random.default_rng(2)
d2 = rng.normal(0, 1, x.shape)
d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True) + hits["ng"][on]).astype(np.float32)          # cosine-weighted about the geometric normal
d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(np.float32)
hits2 = both("closest, bounce (incoherent)", scene.query_closest, x, d2)
both("light pdf, camera", scene.query_light_pdf, o1, d1)
both("light pdf, bounce", scene.query_light_pdf, x, d2)



def occlusion(label, o, d, t):
    """rt_query_occluded against rt_query_closest on the rays (o, d) whose closest t is t, alternating, best of --runs by kernel time."""
    for name, tmax in (("none ", None), ("0.5 T", (np.float32(0.5) * t).astype(np.float32)), ("2 T  ", (np.float32(2) * t).astype(np.float32))):
        closest, occluded = [], []
        for _ in range(args.runs):
            closest.append(scene.query_closest(o, d)[1])
            occ, st = scene.query_occluded(o, d, tmax)
            occluded.append(st)
        c_ms = sorted(s.kernel_ms for s in closest)
        st = min(occluded, key=lambda s: s.kernel_ms)
        sc = min(closest, key=lambda s: s.kernel_ms)
        print(f"  {label} tmax {name} closest  kernels {c_ms[0]:8.3f} ms = {sc.rays / c_ms[0] / 1e3:8.1f} Mrays/s (runs {', '.join('%.3f' % v for v in c_ms)}: spread {c_ms[-1] - c_ms[0]:.3f} ms)"
              f"   call {sc.total_ms:7.1f} ms   exact walks {sc.exact_walks}", flush=True)
        print(f"  {label} tmax {name} occluded kernels {st.kernel_ms:8.3f} ms = {st.rays / st.kernel_ms / 1e3:8.1f} Mrays/s (runs {', '.join('%.3f' % v for v in sorted(s.kernel_ms for s in occluded))})"
              f"   call {st.total_ms:7.1f} ms   exact walks {st.exact_walks} ({100.0 * st.exact_walks / max(1, st.rays):.4f} %, {st.exact_walks / max(1, sc.exact_walks):.1f}x closest's)"
              f"   occluded {int((occ & 1).sum())}   no longer than closest beyond its spread: {bool(st.kernel_ms <= c_ms[0] + (c_ms[-1] - c_ms[0]))}", flush=True)
        ref, st_r = scene.query_occluded(o, d, tmax, flags=rt.RT_QUERY_REFERENCE_WALK)
        mask = np.uint8(0xFF ^ rt.RT_OCCLUSION_EXACT_WALK)
        print(f"  {label} tmax {name} occluded reference walk kernels {st_r.kernel_ms:8.3f} ms; fast path == reference walk, bit for bit: "
              f"{bool(np.array_equal(occ & mask, ref & mask))} ({int(((occ & mask) != (ref & mask)).sum())} rays differ)", flush=True)


print(f"occlusion against closest hit, alternating, best of {args.runs} by kernel time; host arrays in, host arrays out")
occlusion("camera", o1, d1, np.where(on, hits["t"], np.float32(1)).astype(np.float32))
occlusion("bounce", x, d2, np.where(hits2["triangle"] != rt.RT_HIT_MISS, hits2["t"], np.float32(1)).astype(np.float32))

os.environ["RTAMD_KERNEL"] = "wavefront"
_, _, st = scene.render(W, H, 4, want_float=False, counters=True)
assert st.pipeline == rt.RT_PIPELINE_ROUNDS
print(f"for scale, the round pipeline's render {W}x{H}x4 with counters: {st.closest_hit_queries} closest-hit and {st.light_pdf_queries} light queries in "
      f"{st.dominant_kernel_ms:.1f} ms of traverse launches = {st.closest_hit_queries / st.dominant_kernel_ms / 1e3:.1f} M closest hits/s (light walks share those launches)")
scene.close()

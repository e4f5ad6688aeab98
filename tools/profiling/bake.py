"""The baker (rt_bake_rays, rt_bake) on synth_room_v1, device pointers (torch tensors), two workloads:
  texels  the first hits of the 1920x1080 frame (pixel centres) as points, irradiance, 16 samples, K = 1, depth 6
  probes  4,096 points on a 16^3 grid inside the room, SH9, 4,096 samples, K = 64, depth 6
For each: rt_bake as it is (paths restarted in place), rt_bake under RT_BAKE_LOCKSTEP, and the outside loop a caller without rt_bake
would write (per sample rt_bake_rays + rt_trace_paths on the slots' engines; its float sums are not timed) -- kernel time (HIP events),
call time, rounds, ray slots and live ray slots of each, and whether the three agree bit for bit.  The yardsticks are the lockstep run
and the outside loop of the same session.  Run by hand:
    python tools/profiling/bake.py [--runs 7] [--no-resources | --resources-only] [--only texels|probes]
--resources-only needs no GPU: VGPRs, scratch, LDS and occupancy of the three kernels of device/rt_bake.h."""
import argparse, importlib, os, re, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--only", choices=("texels", "probes"))
args = ap.parse_args()
KERNELS = ("rq_bake_rays_kernel", "rq_bake_advance_kernel", "rq_bake_resolve_kernel", "rq_path_advance_kernel")
W, H, DEPTH = 1920, 1080, 6


def resources():
    import test_kernel_resources as tk  # the Makefile's flags, as the budget test reads them
    csrc = os.path.join(ROOT, "raytracing-course-hw_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([tk.HIPCC] + tk._makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "rtamd_api.hip",
                            "-o", os.path.join(tmp, "api.o")], cwd=csrc, stderr=subprocess.PIPE, text=True, check=True)
    name, rows = None, {}
    for line in r.stderr.splitlines():
        if "Function Name" in line:
            name = next((k for k in KERNELS if k in line), None)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            rows.setdefault(name, {})[m.group(1).split(" [")[0]] = int(m.group(2))
    print("kernel resources (gfx950, the Makefile's flags):")
    for k in KERNELS:
        u = rows[k]
        print(f"  {k:28s} VGPRs {u['VGPRs']:3d}  scratch {u['ScratchSize']:4d} B/lane  LDS {u['LDS Size']:6d} B/block  occupancy {u['Occupancy']} waves/SIMD")


if not args.no_resources:
    resources()
if args.resources_only:
    sys.exit(0)

import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
scene = rt.Scene(sd)
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth}; 2 warm-up calls, then median (min) of {args.runs}")
words = lambda a, cols: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, cols).copy()).cuda()
host = lambda t: t.cpu().numpy().view(np.uint32)


def timed(call):
    """call() -> a record with kernel_ms and total_ms; (median, min) of each over the runs, after two warm-up calls."""
    for _ in range(2):
        call()
    st = [call() for _ in range(args.runs)]
    k, t = np.array([s.kernel_ms for s in st]), np.array([s.total_ms for s in st])
    return (float(np.median(k)), float(k.min())), (float(np.median(t)), float(t.min())), st[0]


class Sum:
    """The statistics of the outside loop's calls, added up."""
    def __init__(self):
        self.kernel_ms = self.total_ms = 0.0
        self.launches = self.exact_walks = 0

    def add(self, st):
        self.kernel_ms += st.kernel_ms; self.total_ms += st.total_ms; self.launches += st.launches; self.exact_walks += st.exact_walks


def workload(name, points, mode, samples, K):
    n, floats, q = len(points), rt.BAKE_FLOATS[mode], samples // K
    slots = n * K
    engines = np.zeros(slots, rt.RNG_DTYPE)
    engines["x"] = 1 + np.arange(slots, dtype=np.uint64) * 7919 % 2147483646
    d_points, d_rng = words(points, 6), words(engines, 4)
    d_slot_points = words(np.repeat(points, K), 6) if K > 1 else d_points
    d_out = torch.zeros((n, floats), dtype=torch.int32, device="cuda")
    d_rays, d_L = torch.zeros((slots, 6), dtype=torch.int32, device="cuda"), torch.zeros((slots, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    print(f"{name}: {n} points, mode {mode}, {samples} samples, K = {K} ({slots} slots of {q} paths), depth {DEPTH}", flush=True)
    kept = {}

    def bake(flags):
        def call():
            d_rng.copy_(words(engines, 4))       # the same engines every run
            torch.cuda.synchronize()
            return scene.bake_device(d_points.data_ptr(), d_rng.data_ptr(), n, d_out.data_ptr(), samples, K, mode, DEPTH, flags=flags)
        return call

    def outside():
        d_rng.copy_(words(engines, 4))
        torch.cuda.synchronize()
        total = Sum()
        for _ in range(q):
            total.add(scene.bake_rays_device(d_slot_points.data_ptr(), d_rng.data_ptr(), slots, d_rays.data_ptr(), mode))
            total.add(scene.trace_paths_device(d_rays.data_ptr(), d_rng.data_ptr(), slots, d_L.data_ptr(), ray_depth=DEPTH))
        return total

    for label, call in (("restart in place", bake(0)), ("RT_BAKE_LOCKSTEP", bake(rt.RT_BAKE_LOCKSTEP)), ("outside loop", outside)):
        (k, kmin), (t, tmin), st = timed(call)
        kept[label] = (host(d_out).copy(), host(d_rng).copy(), k)
        line = f"  {label:17s} kernel {k:9.3f} ms ({kmin:.3f}) = {slots * q / k / 1e3:6.1f} Mpaths/s   call {t:9.3f} ms ({tmin:.3f})   call - kernel {t - k:7.3f} ms   {st.launches} launches"
        if label != "outside loop":
            line += f"\n  {'':17s} rounds {st.rounds}, ray slots {st.ray_slots}, live {st.live_ray_slots} ({st.live_ray_slots / st.ray_slots:.1%}), {st.exact_walks} exact walks, {st.invalid_points} invalid points"
        print(line, flush=True)
    a, b, c = kept["restart in place"], kept["RT_BAKE_LOCKSTEP"], kept["outside loop"]
    print(f"  restart in place == lockstep, bit for bit: outputs {np.array_equal(a[0], b[0])}, engines {np.array_equal(a[1], b[1])}; engines == the outside loop's: {np.array_equal(a[1], c[1])}")
    print(f"  kernel time: restart in place = {a[2] / b[2]:.3f} x lockstep = {a[2] / c[2]:.3f} x the outside loop")


if args.only != "probes":
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    xy = np.stack([x.reshape(-1) + np.float32(0.5), y.reshape(-1) + np.float32(0.5)], axis=1)
    o, d = scene.camera_rays(W, H, xy)
    hits, _ = scene.query_closest(o, d)
    on = hits["triangle"] != rt.RT_HIT_MISS
    p = (o[on] + hits["t"][on, None] * d[on]).astype(np.float32)
    print(f"texels: {int(on.sum())} of {W * H} pixel centres hit")
    workload("texels", rt.pack_bake_points(p, hits["ng"][on]), rt.RT_BAKE_IRRADIANCE, 16, 1)
if args.only != "texels":
    xyz = np.asarray(sd.positions, np.float32).reshape(-1, 3)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    g = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    workload("probes", rt.pack_bake_points(lo + (0.1 + 0.8 * grid) * (hi - lo)), rt.RT_BAKE_SH9, 4096, 64)
scene.close()

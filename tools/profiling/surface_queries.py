"""The first-hit layer (rt_query_surface, rt_render_guides) on synth_room_v1: surface query rates on the hits of the camera rays of the
1920x1080 frame (coherent) and of one bounce ray from each of their hit points (incoherent) -- profiles/r20_ray_queries.txt's two sets --,
with host arrays and with device pointers (torch tensors), by kernel time (HIP events around the chunk's kernel) and by wall time of the
call; each rate next to the traffic floor of the gather, 128 bytes per hit (64 in, 64 out; texel traffic not counted) at the HBM rate
MI355X_MICROARCH.md measured (6.29 TB/s, float4 copy).  Then rt_render_guides at 1920x1080 next to its yardstick, rt_render(samples = 1,
ray_depth = 1) of the same scene: one closest hit and one material fetch per pixel in the render's own organisation.  Run by hand:
    python tools/profiling/surface_queries.py [--runs 7] [--no-resources | --resources-only] [--render-only]
--resources-only needs no GPU: it compiles rtamd_api.hip for the device with -Rpass-analysis=kernel-resource-usage and prints VGPRs,
scratch, LDS and occupancy of the layer's kernels.  --render-only prints the yardstick alone (it runs on a tree without the layer too)."""
import argparse, importlib, os, re, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--render-only", action="store_true")
args = ap.parse_args()
KERNELS = ("rq_material_table_kernel", "rq_surface_kernel", "rq_environment_kernel", "rq_camera_rays_kernel", "rq_guides_kernel")
HBM_BYTES_PER_S = 6.29e12
W, H = 1920, 1080


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


if not (args.no_resources or args.render_only):
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


def timed(call):
    """call() -> a stats record with kernel_ms and total_ms; (median, min) of each over the runs, after two warm-up calls."""
    for _ in range(2):
        call()
    st = [call() for _ in range(args.runs)]
    k, t = np.array([s.kernel_ms for s in st]), np.array([s.total_ms for s in st])
    return (float(np.median(k)), float(k.min())), (float(np.median(t)), float(t.min())), st[0]


def yardstick():
    os.environ.pop("RTAMD_KERNEL", None)
    (k, kmin), (t, tmin), st = timed(lambda: scene.render(W, H, 1, want_float=True, want_rgb8=False, ray_depth=1)[2])
    print(f"  rt_render {W}x{H}, samples 1, ray_depth 1 (pipeline {st.pipeline}): kernel_ms {k:.3f} ({kmin:.3f})  total_ms {t:.3f} ({tmin:.3f})", flush=True)
    return k


if args.render_only:
    yardstick()
    scene.close()
    sys.exit(0)

import test_gpu_query as tq  # the tests' camera-ray generator
o1, d1 = tq._camera_rays(sd, W, H, seed=1)
cam, _ = scene.query_closest(o1, d1)
on = cam["triangle"] != rt.RT_HIT_MISS
x = (o1[on] + cam["t"][on, None] * d1[on] + np.float32(1e-4) * cam["ng"][on]).astype(np.float32)
rng = np.random.default_rng(2)
d2 = rng.normal(0, 1, x.shape)
d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True) + cam["ng"][on]).astype(np.float32)          # cosine-weighted about the geometric normal
d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(np.float32)
bounce, _ = scene.query_closest(x, d2)


def report(label, hits):
    n = len(hits)
    floor_ms = n * 128 / HBM_BYTES_PER_S * 1e3
    out = {}
    (k, kmin), (t, tmin), _ = timed(lambda: out.__setitem__("host", scene.query_surface(hits)) or out["host"][1])
    print(f"  {label:18s} host arrays     {n:8d} records ({int((hits['triangle'] != rt.RT_HIT_MISS).sum())} hits)  kernel {k:7.3f} ms ({kmin:.3f}) = {n / k / 1e3:8.1f} M/s, "
          f"traffic floor {floor_ms:.3f} ms = {floor_ms / k:.2f} of it   call {t:7.2f} ms ({tmin:.2f}) = {n / t / 1e3:7.1f} M/s", flush=True)
    d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 16).copy()).cuda()
    d_out = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    (k, kmin), (t, tmin), _ = timed(lambda: scene.query_surface_device(d_hits.data_ptr(), n, d_out.data_ptr()))
    print(f"  {label:18s} device pointers {n:8d} records  kernel {k:7.3f} ms ({kmin:.3f}) = {n / k / 1e3:8.1f} M/s, traffic floor {floor_ms / k:.2f} of it   "
          f"call {t:7.2f} ms ({tmin:.2f}) = {n / t / 1e3:7.1f} M/s", flush=True)
    same = np.array_equal(d_out.cpu().numpy().view(np.uint32), out["host"][0].view(np.uint32).reshape(-1, 16))
    print(f"  {label:18s} device pointers == host arrays, bit for bit: {same}", flush=True)


print("rt_query_surface:")
report("camera (coherent)", cam)
report("bounce (incoherent)", bounce)
print("rt_render_guides against its yardstick:")
render_ms = yardstick()
(k, kmin), (t, tmin), st = timed(lambda: scene.render_guides(W, H)[1])
print(f"  rt_render_guides {W}x{H}, host planes:   kernel_ms {k:.3f} ({kmin:.3f}) = {k / render_ms:.2f} x the yardstick   total_ms {t:.3f} ({tmin:.3f})   "
      f"{st.launches} launches, {st.exact_walks} exact walks", flush=True)
planes = [torch.zeros((H, W, c), dtype=torch.float32, device="cuda") for c in (3, 3, 1, 3)]
torch.cuda.synchronize()
(k, kmin), (t, tmin), st = timed(lambda: scene.render_guides_device(W, H, *[p.data_ptr() for p in planes]))
print(f"  rt_render_guides {W}x{H}, device planes: kernel_ms {k:.3f} ({kmin:.3f}) = {k / render_ms:.2f} x the yardstick   total_ms {t:.3f} ({tmin:.3f})", flush=True)
guides_ms = k
# where a guide pass spends its kernel time: the same pixel-centre rays through the public calls it is composed of, device pointers
n = W * H
px, py = np.meshgrid(np.arange(W, dtype=np.float32) + np.float32(0.5), np.arange(H, dtype=np.float32) + np.float32(0.5))
d_xy = torch.from_numpy(np.stack([px.reshape(-1), py.reshape(-1)], axis=1).copy()).cuda()
d_rays, d_hits, d_surf = (torch.zeros((n, c), dtype=torch.float32, device="cuda") for c in (6, 16, 16))
d_env = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
scene.camera_rays_device(W, H, d_xy.data_ptr(), n, d_rays.data_ptr())
parts = 0.0
for label, call in (("rt_query_closest", lambda: scene.query_closest_device(d_rays.data_ptr(), n, d_hits.data_ptr())),
                    ("rt_query_surface", lambda: scene.query_surface_device(d_hits.data_ptr(), n, d_surf.data_ptr())),
                    ("rt_query_environment", lambda: scene.query_environment_device(d_rays.data_ptr(), n, d_env.data_ptr()))):
    (k, kmin), _, st = timed(call)
    parts += k if label != "rt_query_environment" else 0.0
    print(f"  {label:22s} on the pixel-centre rays: kernel_ms {k:.3f} ({kmin:.3f}) = {k / guides_ms:.2f} of the guide pass   {st.launches} launches", flush=True)
print(f"  left for the camera-ray and plane kernels of the 8 chunks: {guides_ms - parts:.3f} ms", flush=True)
scene.close()

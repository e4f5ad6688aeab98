"""The preview filter (rt_denoise) on a 1920x1080 frame of seeded synthetic planes in device memory: kernel time (HIP events from the pack
kernel to the last level) and wall time of the call (launches and the synchronisation included) for 1 .. 8 levels, with and without an
error map; the time of level k is the difference between k + 1 and k levels.  Medians over --runs calls after a warm-up, and the
spread (min .. max) next to them.  A checksum of the filtered floats is printed per configuration, so that two builds of the library
(RTAMD_LIB=other.so) can be compared on the same planes.  Run by hand:
    python tools/profiling/denoise_levels.py [--runs 20] [--width 1920 --height 1080]"""
import argparse, importlib, os, sys, zlib
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--levels", type=int, nargs="*", default=list(range(1, 9)))
args = ap.parse_args()
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import pin_cases

W, H = args.width, args.height
rng = np.random.default_rng(22)
# a picture-like frame: smooth shading plus noise, 40 x 40 pixel facets with normals of their own, a depth ramp with steps, a fifth of misses
yy, xx = np.mgrid[0:H, 0:W]
facet = (yy // 40) * ((W + 39) // 40) + xx // 40
fn = rng.normal(0, 1, (facet.max() + 1, 3))
fn /= np.linalg.norm(fn, axis=1, keepdims=True)
normal = fn[facet].astype(np.float32)
depth = (2 + 0.002 * xx + 0.001 * yy + 0.5 * (facet % 3)).astype(np.float32)
depth[rng.uniform(size=(facet.max() + 1))[facet] < 0.2] = 0
shade = (0.5 + 0.4 * np.sin(xx / 97.0) * np.cos(yy / 61.0))[..., None] * np.array([1.0, 0.8, 0.6])
rgb = (shade * rng.gamma(4.0, 0.25, (H, W, 1))).astype(np.float32)
se = (0.5 * shade[..., 0] * (0.2 + rng.uniform(size=(H, W)))).astype(np.float32)
albedo = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(rgb=rgb, normal=normal, depth=depth, se=se, albedo=albedo).items()}
out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
out8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
scene = rt.Scene(pin_cases.load_sphere())
print(f"library {rt.LIB_PATH}\nframe {W}x{H}, {int((depth == 0).sum())} fixed pixels, {args.runs} runs per row; times in ms: median (min .. max)")


def measure(levels, with_se):
    def call():
        return scene.denoise_device(W, H, dev["rgb"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr(), None, None,
                                    dev["se"].data_ptr() if with_se else None, out_rgb_ptr=out.data_ptr(), out_rgb8_ptr=out8.data_ptr(), iterations=levels)
    for _ in range(3):
        call()
    k, t = [], []
    for _ in range(args.runs):
        st = call()
        k.append(st.kernel_ms); t.append(st.total_ms)
    return np.array(k), np.array(t), zlib.crc32(out.cpu().numpy().tobytes())


fmt = lambda a: f"{np.median(a):7.3f} ({a.min():6.3f} .. {a.max():6.3f})"
for with_se in (True, False):
    print(f"\n{'with' if with_se else 'without'} an error map\nlevels  kernels (pack + levels)        wall time of the call          last level  crc32 of the floats")
    prev = None
    for levels in args.levels:
        k, t, crc = measure(levels, with_se)
        step = "" if prev is None else f"{np.median(k) - prev:7.3f}"
        print(f"{levels:6d}  {fmt(k)}  {fmt(t)}  {step:>10s}  {crc:08x}")
        prev = float(np.median(k))
scene.close()

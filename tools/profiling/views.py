"""View sets next to what the library offered before them (profiles/r36_views.txt): synth_room_v1, depth 6, one MI355X.  Every figure is
the median of --runs repeats, a repeat of the view set alternating with a repeat of its referee in one process.
  a  one view at the scene's own camera, 1920x1080, slices of 16: rt_views_render against rt_accum_render -- the price of the detour
     (gather, scatter) and of pt_source_exact on every first ray
  b  64 views of 128x128 on an orbit inside the room, 64 samples: one rt_views_render call against (1) what the parent offers, per camera
     rt_scene_create then rt_render, creation and kernel time apart (every --stride-th camera of the orbit is created per repeat and
     the sum is scaled to 64: a creation is a host replay of the scene), and (2) 64 x rt_render of that size on the one scene (its own
     camera: the same work per frame to within the view), which isolates the occupancy gain
  c  the same 64 views moved out of the room (outside the node grid: every first ray is the exact role's) against b's view set
Run by hand:
    python tools/profiling/views.py [--runs 5] [--stride 8]"""
import argparse, importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--stride", type=int, default=8)
args = ap.parse_args()
DEPTH = 6

import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    sd = rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0])
t0 = time.perf_counter()
scene = rt.Scene(sd)
create_ms = (time.perf_counter() - t0) * 1e3
info = scene.info()
print(f"synth_room_v1: {info.n_triangles} triangles, {info.n_lights} lights, tree depth {info.bvh_depth}; depth {DEPTH}; rt_scene_create {create_ms:.1f} ms", flush=True)
med = lambda v: f"median {np.median(v):9.3f} (min {np.min(v):.3f}, max {np.max(v):.3f})"
wall = lambda f: (lambda t0: (f(), (time.perf_counter() - t0) * 1e3))(time.perf_counter())


def orbit(n, radius, height=3.0, fov_y=0.9):
    """n cameras on a circle of `radius` about the room's axis at `height`, each looking at (0, height, 0)."""
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


# ---- a: one view at the scene's own camera against rt_accum_render ------------------------------------------------------------------------
W, H, SLICE = 1920, 1080, 16
acc = scene.accumulator(W, H, ray_depth=DEPTH)
views = scene.views(W, H, [sd.camera], ray_depth=DEPTH)
acc.render(SLICE); views.render(SLICE)      # one warm-up slice each
ref, new = [], []
for _ in range(args.runs):
    st, ms = wall(lambda: acc.render(SLICE)); ref.append((st.kernel_ms, ms, st.exact_closest_hits + st.exact_light_sums))
    st = views.render(SLICE); new.append((st.kernel_ms, st.total_ms, st.gather_ms, st.scatter_ms, st.launches, st.exact_walks))
ref, new = np.array(ref), np.array(new)
same = np.array_equal(acc.resolve()[1], views.resolve(0)[1])
print(f"a. one view at the scene's own camera, {W}x{H}, one slice of {SLICE} samples, {args.runs} alternating repeats after one warm-up slice each")
print(f"  rt_accum_render (referee)   kernel_ms {med(ref[:, 0])}   call ms {med(ref[:, 1])}   exact walks {int(np.median(ref[:, 2]))}")
print(f"  rt_views_render             kernel_ms {med(new[:, 0])}   call ms {med(new[:, 1])}   exact walks {int(np.median(new[:, 5]))}   launches {int(new[0, 4])}")
print(f"    of which gather_ms {med(new[:, 2])}   scatter_ms {med(new[:, 3])}")
print(f"  kernel over the strip / over the frame: {np.median(new[:, 0]) / np.median(ref[:, 0]):.3f} x ({np.median(new[:, 0]) - np.median(ref[:, 0]):+.3f} ms); "
      f"whole call: {np.median(new[:, 1]) / np.median(ref[:, 1]):.3f} x ({np.median(new[:, 1]) - np.median(ref[:, 1]):+.3f} ms); bytes after {(args.runs + 1) * SLICE} samples equal: {same}", flush=True)
acc.close(); views.close()

# ---- b: 64 small views in one call against 64 scenes, and against 64 renders on the one scene -----------------------------------------------
N, W, H, SPP = 64, 128, 128, 64
inside = orbit(N, 5.0)
subset = list(range(0, N, args.stride))
one, parent, plain = [], [], []
scene.render(W, H, SPP, ray_depth=DEPTH)
views = scene.views(W, H, inside, ray_depth=DEPTH); views.render(SPP); views.close()     # warm-up
check, equal, checked = None, 0, 0
for _ in range(args.runs):
    def set_call():
        v = scene.views(W, H, inside, ray_depth=DEPTH)
        st = v.render(SPP)
        return v, st
    (v, st), ms = wall(set_call)
    one.append((st.kernel_ms, st.total_ms, ms, st.gather_ms + st.scatter_ms, st.exact_walks, st.launches))
    if check is None:
        check = [v.resolve(i)[1] for i in subset]
    v.close()
    c_ms = k_ms = r_ms = 0.0
    for j, i in enumerate(subset):
        data = swapped(inside[i])
        s, ms = wall(lambda: rt.Scene(data)); c_ms += ms
        (_, rgb8, st), ms = wall(lambda: s.render(W, H, SPP, ray_depth=DEPTH)); k_ms += st.kernel_ms; r_ms += ms
        equal += int(st.reference_exact == 1 and np.array_equal(rgb8, check[j])); checked += 1   # the contract, on the headline scene
        s.close()
    parent.append((c_ms * N / len(subset), k_ms * N / len(subset), r_ms * N / len(subset)))
    k_ms = r_ms = 0.0
    for i in range(N):
        (_, _, st), ms = wall(lambda: scene.render(W, H, SPP, ray_depth=DEPTH)); k_ms += st.kernel_ms; r_ms += ms
    plain.append((k_ms, r_ms))
one, parent, plain = np.array(one), np.array(parent), np.array(plain)
print(f"b. {N} views of {W}x{H} on an orbit of radius 5 inside the room, {SPP} samples, {args.runs} alternating repeats; views byte-equal to their fresh scenes' renders: {equal} of {checked} checked ({len(subset)} of the {N} per repeat)")
print(f"  one rt_views_render call      kernel_ms {med(one[:, 0])}   call ms {med(one[:, 1])}   with rt_views_create {med(one[:, 2])}")
print(f"    gather + scatter ms {med(one[:, 3])}   exact walks {int(np.median(one[:, 4]))} of {N * W * H * SPP} camera samples   launches {int(one[0, 5])}")
print(f"  {N} x (rt_scene_create, rt_render), from {len(subset)} cameras x {N // len(subset)}:  creation ms {med(parent[:, 0])}   kernel_ms {med(parent[:, 1])}   render call ms {med(parent[:, 2])}")
print(f"  {N} x rt_render on the one scene (its own camera):  kernel_ms {med(plain[:, 0])}   call ms {med(plain[:, 1])}")
print(f"  one call / sum of the {N} renders' kernel time (own scenes): {np.median(one[:, 1]) / np.median(parent[:, 1]):.3f} x; "
      f"kernel / kernel on the one scene: {np.median(one[:, 0]) / np.median(plain[:, 0]):.3f} x; one call / creation + render calls: "
      f"{np.median(one[:, 2]) / (np.median(parent[:, 0]) + np.median(parent[:, 2])):.5f} x", flush=True)

# ---- c: every first ray exact -----------------------------------------------------------------------------------------------------------------
outside = orbit(N, 30.0)
a, b = scene.views(W, H, inside, ray_depth=DEPTH), scene.views(W, H, outside, ray_depth=DEPTH)
a.render(SPP); b.render(SPP)
fast, exact = [], []
for _ in range(args.runs):
    st = a.render(SPP); fast.append((st.kernel_ms, st.exact_walks))
    st = b.render(SPP); exact.append((st.kernel_ms, st.exact_walks))
fast, exact = np.array(fast), np.array(exact)
print(f"c. the same {N} views on an orbit of radius 30, outside the room and its node grid (they see the room's outer walls: shorter paths), {SPP} samples")
print(f"  inside   kernel_ms {med(fast[:, 0])}   exact walks {int(np.median(fast[:, 1]))}")
print(f"  outside  kernel_ms {med(exact[:, 0])}   exact walks {int(np.median(exact[:, 1]))} (camera samples {N * W * H * SPP})")
print(f"  outside / inside: {np.median(exact[:, 0]) / np.median(fast[:, 0]):.3f} x", flush=True)
a.close(); b.close()
# the same rays on walkers derived for them: one outside camera on the big frame, the view set on the room's scene (every first ray exact)
# against rt_accum_render on a scene created WITH that camera (its grid and bound span the camera: the walkers take the rays)
W, H, SLICE = 1920, 1080, 16
far, beside = rt.rt_camera.from_buffer_copy(outside[0]), rt.rt_camera.from_buffer_copy(outside[N // 4])
far.position[2], beside.position[0] = 40.0, 12.0
for name, cam in (("far: (0, 3, 40) looking along -z", far), ("beside: (12, 3, 0) looking along -x", beside)):
    own = rt.Scene(swapped(cam))
    acc = own.accumulator(W, H, ray_depth=DEPTH)
    views = scene.views(W, H, [cam], ray_depth=DEPTH)
    acc.render(SLICE); views.render(SLICE)
    ref, new = [], []
    for _ in range(args.runs):
        st = acc.render(SLICE); ref.append((st.kernel_ms, st.exact_closest_hits + st.exact_light_sums))
        st = views.render(SLICE); new.append((st.kernel_ms, st.exact_walks))
    ref, new = np.array(ref), np.array(new)
    same = np.array_equal(acc.resolve()[1], views.resolve(0)[1])
    print(f"  {name}, {W}x{H}, one slice of {SLICE}: rt_accum_render on a scene created with it  kernel_ms {med(ref[:, 0])}  exact walks {int(np.median(ref[:, 1]))}")
    print(f"    rt_views_render on the room's scene  kernel_ms {med(new[:, 0])}  exact walks {int(np.median(new[:, 1]))} (camera samples {W * H * SLICE}); "
          f"{np.median(new[:, 0]) / np.median(ref[:, 0]):.3f} x; bytes equal: {same}", flush=True)
    acc.close(); views.close(); own.close()
scene.close()

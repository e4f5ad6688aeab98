"""What the thirteen launching calls of the query layer (csrc/rtamd_query.hip) answer and report, as digests: one line per case,
`name@host|device, sha256 of every array the call writes (the engines included; the first 16 hex digits), the deterministic fields
of its stats` -- never a time.

tests/golden/query_digests.txt is this module's output with the library as it was BEFORE the layer's host side was pulled together
(one chunk loop, one staging map, one stats shell); test_gpu_query_digests.py runs the module in a child process and compares line
by line, so the answers, the engines, the launch counts and the invalid-record counts stay as they were, through the staging (host
arrays) and without it (device pointers).  A case's @host and @device lines must be equal but for the tag.

The whole table runs under RTAMD_QUERY_CHUNK=64, on the sphere scene and on the textured soup_a of surface_cases.py:
  n = 0, 1 and 200 records (three full chunks and a ragged fourth): rays of this module's own making, the first through a pixel
    next to the frame's centre where both scenes are hit, so n = 1 is a record with a surface; two of the 200 rays are NaN, so the invalid counts are not zero;
  the bakers at 0, 1, 8 and 40 points of 4 streams, 8 samples, depth 4 (16 whole points per chunk: 8 points are one ragged chunk,
    40 two full ones and a ragged third), in both modes, with RT_BAKE_LOCKSTEP and without;
  rt_render_guides at 17 x 13 with the emission plane left out.
The staging sizes (rt_scene::query_stage_bytes, source_stage_bytes) are reported by no hook or rt_scene_info field and are not in
the lines.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_digests.txt")
CHUNK = "64"
SCENES = ("sphere_emissive", "soup_a")
SIZES = (0, 1, 200)
BAKE_POINTS, K, SAMPLES, DEPTH = (0, 1, 8, 40), 4, 8, 4
W, H = 17, 13
DEV, LOCKSTEP = 1, 4
F = np.float32
QUERY_FIELDS = ("rays", "launches", "exact_walks", "invalid_rays", "reference_exact")
BAKE_FIELDS = ("points", "launches", "exact_walks", "invalid_points", "reference_exact", "paths", "rounds", "ray_slots", "live_ray_slots")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).reshape(-1).tobytes()).hexdigest()[:16]


class Runner:
    def __init__(self, rt, torch):
        self.rt, self.torch, self.lines = rt, torch, []

    def both(self, name, fn, ins, outs, stats_cls, fields):
        """fn(p, flags, stats) makes the call; p maps each array's name to its pointer (None for a name in neither `ins` nor `outs`).
        ins: arrays the call reads (those it also writes are in `outs` too, by name only); outs: name -> zeros to write into."""
        for where in ("host", "device"):
            arrays = {k: np.ascontiguousarray(v).copy() for k, v in ins.items()}
            arrays.update({k: np.zeros_like(v) for k, v in outs.items() if k not in ins})
            if where == "device":
                held = {k: self.torch.from_numpy(v.view(np.uint8).reshape(-1)).cuda() for k, v in arrays.items()}
                p = {k: t.data_ptr() if t.numel() else None for k, t in held.items()}
            else:
                p = {k: v.ctypes.data if v.size else None for k, v in arrays.items()}
            st = stats_cls() if stats_cls else None
            if st is not None:
                st.struct_size = C.sizeof(st)
            code = fn(p, DEV if where == "device" else 0, C.byref(st) if st is not None else None)
            assert code == 0, (name, where, code, self.rt.lib.rt_last_error().decode())
            if where == "device":
                self.torch.cuda.synchronize()
                arrays = {k: held[k].cpu().numpy() for k in arrays}
            digests = " ".join(f"{k}={_sha(arrays[k])}" for k in outs)
            report = " ".join(f"{f}={getattr(st, f)}" for f in fields) if st is not None else "-"
            self.lines.append(f"{name}@{where}, {digests}, {report}")
        return arrays  # the device run's, as host arrays: the next call's input


def _camera_rays(sd, w=48, h=32):
    """One jittered ray through every pixel of a w x h frame of the scene's camera, in frame order: (o, d), float32."""
    cam = sd.camera
    gen = np.random.default_rng(31)
    px = (np.arange(w, dtype=F)[None, :] + gen.uniform(0, 1, (h, w)).astype(F)).reshape(-1)
    py = (np.arange(h, dtype=F)[:, None] + gen.uniform(0, 1, (h, w)).astype(F)).reshape(-1)
    tan_y = F(np.tan(np.float64(cam.fov_y) / 2))
    tan_x = F(tan_y * F(w) / F(h))
    cx, cy = tan_x * (F(2) * px / F(w) - F(1)), tan_y * (F(2) * py / F(h) - F(1))
    right, up, fwd = (np.array(v, F) for v in (cam.right, cam.up, cam.forward))
    d = cx[:, None] * right - cy[:, None] * up + fwd
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return np.broadcast_to(np.array(cam.position, F), d.shape).copy(), d


def _rays(rt, sd, n, w=48, h=32):
    """n rays: first the one through pixel (23, 16), next to the frame's centre, which hits in both scenes (the oracle's closest_hit says
    so), so that n = 1 is a record with a surface; then every step-th pixel."""
    o, d = _camera_rays(sd, w, h)
    first, rest = 16 * w + 23, np.arange(0, w * h, max(1, w * h // max(n, 1)))
    pick = np.concatenate([[first], rest[rest != first]])[:n]
    rays = rt.pack_rays(o[pick], d[pick])
    assert len(rays) == n
    if n > 130:
        rays["d"][5] = np.nan
        rays["o"][130, 1] = np.nan
    return rays


def _scene_cases(r, scene, sd, tag, sc):
    rt, lib, h = r.rt, r.rt.lib, scene._h
    Q, B = rt.rt_query_stats, rt.rt_bake_stats
    for n in SIZES:
        t = f"{tag}.n{n}"
        rays = _rays(rt, sd, n)
        rng = rt.rng_seed(1 + 7919 * np.arange(n))
        hits = r.both(f"rt_query_closest.{t}", lambda p, fl, st: lib.rt_query_closest(h, p["rays"], n, fl, p["hits"], st),
                      {"rays": rays}, {"hits": np.zeros(n, rt.HIT_DTYPE)}, Q, QUERY_FIELDS)["hits"].view(rt.HIT_DTYPE)
        assert n == 0 or hits["triangle"][0] != 0xFFFFFFFF, (tag, "the first ray must hit: n = 1 is a record with a surface")
        r.both(f"rt_query_closest.reference_walk.{t}", lambda p, fl, st: lib.rt_query_closest(h, p["rays"], n, fl | 2, p["hits"], st),
               {"rays": rays}, {"hits": np.zeros(n, rt.HIT_DTYPE)}, Q, QUERY_FIELDS)
        r.both(f"rt_query_light_pdf.{t}", lambda p, fl, st: lib.rt_query_light_pdf(h, p["rays"], n, fl, p["pdf"], st),
               {"rays": rays}, {"pdf": np.zeros(n, F)}, Q, QUERY_FIELDS)
        tmax = (hits["t"] * np.where(np.arange(n) % 2 == 0, F(0.5), F(2))).astype(F)
        r.both(f"rt_query_occluded.{t}", lambda p, fl, st: lib.rt_query_occluded(h, p["rays"], p["tmax"], n, fl, p["occ"], st),
               {"rays": rays, "tmax": tmax}, {"occ": np.zeros(n, np.uint8)}, Q, QUERY_FIELDS)
        r.both(f"rt_query_occluded.no_tmax.{t}", lambda p, fl, st: lib.rt_query_occluded(h, p["rays"], None, n, fl, p["occ"], st),
               {"rays": rays}, {"occ": np.zeros(n, np.uint8)}, Q, QUERY_FIELDS)
        surfaces = r.both(f"rt_query_surface.{t}", lambda p, fl, st: lib.rt_query_surface(h, p["hits"], n, fl, p["surfaces"], st),
                          {"hits": hits}, {"surfaces": np.zeros(n, rt.SURFACE_DTYPE)}, Q, QUERY_FIELDS)["surfaces"].view(rt.SURFACE_DTYPE)
        r.both(f"rt_query_environment.{t}", lambda p, fl, st: lib.rt_query_environment(h, p["rays"], n, fl, p["rgb"], st),
               {"rays": rays}, {"rgb": np.zeros((n, 3), F)}, Q, QUERY_FIELDS)
        xy = (sc.centres(W, H) + F(0.25))[:n]
        r.both(f"rt_camera_rays.{t}", lambda p, fl, st: lib.rt_camera_rays(h, W, H, p["xy"], n, fl, p["out"]),
               {"xy": xy}, {"out": np.zeros(n, rt.RAY_DTYPE)}, None, ())
        scat = r.both(f"rt_query_scatter.{t}", lambda p, fl, st: lib.rt_query_scatter(h, p["rays"], p["hits"], p["surfaces"], p["rng"], n, fl, p["out"], st),
                      {"rays": rays, "hits": hits, "surfaces": surfaces, "rng": rng}, {"out": np.zeros(n, rt.SCATTER_DTYPE), "rng": None}, Q, QUERY_FIELDS)["out"].view(rt.SCATTER_DTYPE)
        dirs = np.where(np.isfinite(scat["d"]).all(axis=1, keepdims=True) & (np.abs(scat["d"]).sum(axis=1, keepdims=True) > 0), scat["d"], F([0, 1, 0])).astype(F)
        r.both(f"rt_query_bsdf.{t}", lambda p, fl, st: lib.rt_query_bsdf(h, p["rays"], p["hits"], p["surfaces"], p["dirs"], n, fl, p["brdf"], p["pdf"], st),
               {"rays": rays, "hits": hits, "surfaces": surfaces, "dirs": dirs}, {"brdf": np.zeros((n, 3), F), "pdf": np.zeros(n, F)}, Q, QUERY_FIELDS)
        for fn in ("rt_trace_paths", "rt_render_paths"):
            r.both(f"{fn}.{t}", lambda p, fl, st: getattr(lib, fn)(h, p["rays"], p["rng"], n, DEPTH, fl, p["rgb"], st),
                   {"rays": rays, "rng": rng}, {"rgb": np.zeros((n, 3), F), "rng": None}, Q, QUERY_FIELDS)
        on = hits["triangle"] != 0xFFFFFFFF
        points = rt.pack_bake_points((rays["o"][on] + hits["t"][on, None] * rays["d"][on]).astype(F), hits["ng"][on])
        m = len(points)
        for mode in (0, 1):
            r.both(f"rt_bake_rays.mode{mode}.{t}", lambda p, fl, st: lib.rt_bake_rays(h, p["points"], p["rng"], m, mode, fl, p["out"], st),
                   {"points": points, "rng": rng[:m]}, {"out": np.zeros(m, rt.RAY_DTYPE), "rng": None}, Q, QUERY_FIELDS)
    # the bakers: points at the hits of the 200 rays
    rays = _rays(rt, sd, 200)
    hits, _ = scene.query_closest(rays["o"], rays["d"])
    on = hits["triangle"] != 0xFFFFFFFF
    cand = rt.pack_bake_points((rays["o"][on] + hits["t"][on, None] * rays["d"][on]).astype(F), hits["ng"][on])
    assert len(cand) >= max(BAKE_POINTS), (tag, len(cand))
    for n in BAKE_POINTS:
        points, rng = np.ascontiguousarray(cand[:n]), rt.rng_seed(1 + 7919 * np.arange(n * K))
        for fn, mode, flags in (("rt_bake", 0, 0), ("rt_bake", 0, LOCKSTEP), ("rt_bake", 1, 0), ("rt_bake", 1, LOCKSTEP), ("rt_bake", 0, 2), ("rt_render_bake", 0, 0)):
            def call(p, fl, st, fn=fn, mode=mode, flags=flags):
                params = rt.make_bake_params(SAMPLES, K, mode, DEPTH, flags | fl)
                return getattr(lib, fn)(h, p["points"], n, C.byref(params), p["rng"], p["out"], st)
            r.both(f"{fn}.mode{mode}.flags{flags}.{tag}.p{n}", call, {"points": points, "rng": rng},
                   {"out": np.zeros((n, 27 if mode else 3), F), "rng": None}, B, BAKE_FIELDS)
    planes = {"albedo": np.zeros((H, W, 3), F), "normal": np.zeros((H, W, 3), F), "depth": np.zeros((H, W), F)}
    r.both(f"rt_render_guides.{tag}.{W}x{H}", lambda p, fl, st: lib.rt_render_guides(h, W, H, fl, p["albedo"], p["normal"], p["depth"], None, st),
           {}, planes, Q, QUERY_FIELDS)
    r.both(f"rt_render_guides.depth_only.{tag}.1x1", lambda p, fl, st: lib.rt_render_guides(h, 1, 1, fl, None, None, p["depth"], None, st),
           {}, {"depth": np.zeros((1, 1), F)}, Q, QUERY_FIELDS)


def run():
    """Every line, on device 0.  torch opens the GPU before the library does (the order bench.py keeps), and RTAMD_QUERY_CHUNK is
    read at every call: run this in a process of its own."""
    import torch
    torch.zeros(1).cuda()
    os.environ["RTAMD_QUERY_CHUNK"] = CHUNK
    import surface_cases as sc
    rt = sc.rt
    r = Runner(rt, torch)
    for name in SCENES:
        sd = sc.scene_data(name)
        scene = rt.Scene(sd)
        _scene_cases(r, scene, sd, name, sc)
        scene.close()
    return r.lines


def host_and_device_differ(lines):
    """The cases whose @host and @device lines are not equal but for the tag."""
    strip = lambda line, where: line.replace("@" + where + ",", ",", 1)
    return [h for h, d in zip(lines[0::2], lines[1::2]) if strip(h, "host") != strip(d, "device")]


if __name__ == "__main__":  # python tests/query_digest_cases.py FILE: writes the transcript ("-": to stdout)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    lines = run()
    if sys.argv[1] == "-":
        print("\n".join(lines))
    else:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{len(lines)} lines -> {sys.argv[1]}")

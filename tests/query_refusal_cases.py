"""The calls the query layer (csrc/rtamd_query.hip) must refuse, as a table, and run(): one line per case, `name, return code,
rt_last_error()`.

tests/golden/query_refusals_host.txt (HOST, no GPU) and tests/golden/query_refusals.txt (HOST + GPU, on a GPU) are this module's
output with the library as it was BEFORE the layer's host side was pulled together (one chunk loop, one staging map, one stats shell,
one set of argument predicates); test_query_refusals_host.py and test_gpu_query_refusals_transcript.py compare line by line, so
every return code, every message and the order of the refusals within a call stay byte for byte.

Covered: every fail( site of rtamd_query.hip for its thirteen entry points that refuse anything (rt_rng_seed and rt_rng_uniform
refuse nothing).  HOST: what each call decides before it looks at the scene, on a null scene, with four records or eight points of
four streams.  GPU: the rest, on the sphere scene as hw8 scene, as hw6 scene (the flavor refusal) and without its light (the light
pdf's refusal), with device arrays from torch whose pointers are offset by 4 bytes or 1 byte into the allocation (the alignment
refusals come before any launch), and the refusals of source_check under RTAMD_KERNEL=wavefront (its own) and =mega (check_frame's,
with the call's name in front).  Where two refusals of a call compete, a case gives both and the line shows which one the call
reaches first.

Left out, and why:
  behind a failing HIP call or a failed allocation -- the catch clauses of guarded(), grow(), ensure_materials.
  the launch-deadline and lost-path reports of collect_frame under source_render: the frame driver's, and met only on a fault.
  check_frame's other refusals under source_check: the limits on the strip frame cannot be met, the chunk and RT_MAX_DEPTH bound
    its height and depth before it is asked.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_DIR = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere")
GOLDEN_HOST = os.path.join(ROOT, "tests", "golden", "query_refusals_host.txt")
GOLDEN_GPU = os.path.join(ROOT, "tests", "golden", "query_refusals.txt")
DEV, REF, LOCKSTEP = 1, 2, 4   # RT_QUERY_DEVICE_POINTERS, RT_QUERY_REFERENCE_WALK, RT_BAKE_LOCKSTEP
N, POINTS, K = 4, 8, 4         # records of the ray calls; points and streams of the bakers (32 engines)


class Ctx:
    """The arrays every case draws on, by name: host arrays, and on a GPU device allocations of the same sizes."""

    def __init__(self, rt, torch=None):
        self.rt, self.lib = rt, rt.lib
        F = np.float32
        rng = rt.rng_seed(1 + 7919 * np.arange(POINTS * K))
        self.host = {"rays": rt.pack_rays(np.zeros((32, 3), F), np.tile(np.array([0, 0, -1], F), (32, 1))), "hits": np.zeros(32, rt.HIT_DTYPE),
                     "surfaces": np.zeros(32, rt.SURFACE_DTYPE), "rng": rng, "scatter": np.zeros(32, rt.SCATTER_DTYPE),
                     "dirs": np.ones((32, 3), F), "rgb": np.zeros((32, 3), F), "pdf": np.zeros(32, F), "tmax": np.ones(32, F),
                     "occ": np.zeros(32, np.uint8), "xy": np.full((32, 2), 0.5, F), "out": np.zeros((POINTS, 27), F),
                     "points": rt.pack_bake_points(np.zeros((POINTS, 3), F), np.tile(np.array([0, 1, 0], F), (POINTS, 1)))}
        self.dev = {k: torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).cuda() for k, v in self.host.items()} if torch else {}
        self.scenes = {}

    def ptr(self, name, flags, drop, off):
        if name in drop:
            return None
        base = self.dev[name].data_ptr() if (flags & DEV) and self.dev else self.host[name].ctypes.data
        return base + off.get(name, 0)

    def stats(self, size, cls=None):
        """None: no stats; "ok": the struct's own size; a number: that struct_size."""
        if size is None:
            return None
        st = (cls or self.rt.rt_query_stats)()
        st.struct_size = C.sizeof(st) if size == "ok" else size
        return C.byref(st)

    def scene(self, name):
        return None if name is None else self.scenes[name]._h


def _env(name, value, fn):
    def run(c):
        os.environ[name] = value  # putenv: the library reads its knobs at every call
        try:
            return fn(c)
        finally:
            del os.environ[name]
    return run


def _rng_x(at, x, fn):
    """fn with engine `at` of the host array in the state x."""
    def run(c):
        keep = int(c.host["rng"]["x"][at])
        c.host["rng"]["x"][at] = x
        try:
            return fn(c)
        finally:
            c.host["rng"]["x"][at] = keep
    return run


def _xy(value, fn):
    def run(c):
        c.host["xy"][N - 1, 1] = value
        try:
            return fn(c)
        finally:
            c.host["xy"][N - 1, 1] = 0.5
    return run


# One maker per signature: keywords name what differs from a call that is in order; `drop` the arrays passed as NULL, `off` byte
# offsets added to an array's pointer.
def _in_out(fn, a_in, a_out):
    def make(scene=None, n=N, flags=0, stats="ok", drop=(), off={}):
        return lambda c: getattr(c.lib, fn)(c.scene(scene), c.ptr(a_in, flags, drop, off), n, flags, c.ptr(a_out, flags, drop, off), c.stats(stats))
    return make


closest, light_pdf = _in_out("rt_query_closest", "rays", "hits"), _in_out("rt_query_light_pdf", "rays", "pdf")
surface, environment = _in_out("rt_query_surface", "hits", "surfaces"), _in_out("rt_query_environment", "rays", "rgb")


def occluded(scene=None, n=N, flags=0, stats="ok", drop=(), off={}):
    return lambda c: c.lib.rt_query_occluded(c.scene(scene), c.ptr("rays", flags, drop, off), c.ptr("tmax", flags, drop, off), n, flags,
                                             c.ptr("occ", flags, drop, off), c.stats(stats))


def camera_rays(scene=None, w=16, h=16, n=N, flags=0, drop=(), off={}):
    return lambda c: c.lib.rt_camera_rays(c.scene(scene), w, h, c.ptr("xy", flags, drop, off), n, flags, c.ptr("rays", flags, drop, off))


def guides(scene=None, w=4, h=4, flags=0, stats="ok"):
    return lambda c: c.lib.rt_render_guides(c.scene(scene), w, h, flags, None, None, c.ptr("pdf", flags, (), {}), None, c.stats(stats))


def scatter(scene=None, n=N, flags=0, stats="ok", drop=(), off={}):
    p = lambda c, k: c.ptr(k, flags, drop, off)
    return lambda c: c.lib.rt_query_scatter(c.scene(scene), p(c, "rays"), p(c, "hits"), p(c, "surfaces"), p(c, "rng"), n, flags, p(c, "scatter"), c.stats(stats))


def bsdf(scene=None, n=N, flags=0, stats="ok", drop=(), off={}):
    p = lambda c, k: c.ptr(k, flags, drop, off)
    return lambda c: c.lib.rt_query_bsdf(c.scene(scene), p(c, "rays"), p(c, "hits"), p(c, "surfaces"), p(c, "dirs"), n, flags, p(c, "rgb"), p(c, "pdf"), c.stats(stats))


def _paths(fn):
    def make(scene=None, n=N, depth=0, flags=0, stats="ok", drop=(), off={}):
        p = lambda c, k: c.ptr(k, flags, drop, off)
        return lambda c: getattr(c.lib, fn)(c.scene(scene), p(c, "rays"), p(c, "rng"), n, depth, flags, p(c, "rgb"), c.stats(stats))
    return make


trace_paths, render_paths = _paths("rt_trace_paths"), _paths("rt_render_paths")


def bake_rays(scene=None, n=N, mode=0, flags=0, stats="ok", drop=(), off={}):
    p = lambda c, k: c.ptr(k, flags, drop, off)
    return lambda c: c.lib.rt_bake_rays(c.scene(scene), p(c, "points"), p(c, "rng"), n, mode, flags, p(c, "rays"), c.stats(stats))


def _baker(fn, mode0):
    def make(scene=None, n=POINTS, stats="ok", drop=(), off={}, params="made", **fields):
        def run(c):
            made = c.rt.make_bake_params(8, K, mode0, 4)
            for k, v in fields.items():
                if k == "reserved":
                    made.reserved[v] = 1
                else:
                    setattr(made, k, v)
            flags = made.flags
            p = lambda k: c.ptr(k, flags, drop, off)
            return getattr(c.lib, fn)(c.scene(scene), p("points"), n, C.byref(made) if params == "made" else None, p("rng"), p("out"),
                                      c.stats(stats, c.rt.rt_bake_stats))
        return run
    return make


bake, render_bake = _baker("rt_bake", 1), _baker("rt_render_bake", 0)


def _walk_host(tag, make):
    """rt_query_closest and its like: check_walk_call comes first, so a null scene hides everything behind the stats."""
    return [(f"{tag}.struct_size", make(stats=8)), (f"{tag}.struct_size_over_flags", make(stats=80, flags=8)),
            (f"{tag}.null_scene", make()), (f"{tag}.null_scene_no_stats_n_0", make(stats=None, n=0, drop=("rays", "hits", "pdf", "surfaces", "rgb")))]


def _bounce_host(tag, make, arrays, engines):
    cases = [(f"{tag}.null_{a}", make(drop=(a,))) for a in arrays]
    cases += [(f"{tag}.null_over_struct_size", make(drop=arrays[:1], stats=8)), (f"{tag}.struct_size", make(stats=8)),
              (f"{tag}.struct_size_over_flags", make(stats=80, flags=8)), (f"{tag}.flags_4", make(flags=4)), (f"{tag}.flags_all", make(flags=0xFFFFFFFF))]
    if engines:
        cases += [(f"{tag}.flags_over_engine", _rng_x(0, 0, make(flags=4))), (f"{tag}.engine_0_at_0", _rng_x(0, 0, make())),
                  (f"{tag}.engine_2^31-1_at_3", _rng_x(N - 1, 2**31 - 1, make())), (f"{tag}.engine_beyond_n", _rng_x(N, 0, make())),
                  (f"{tag}.engine_device_array", _rng_x(0, 0, make(flags=DEV)))]
    return cases + [(f"{tag}.null_scene", make()), (f"{tag}.null_scene_n_0", make(n=0, drop=arrays))]


def _baker_host(tag, make, flag_names_bits, extra):
    cases = [(f"{tag}.null_params", make(params=None)), (f"{tag}.params_struct_size", make(struct_size=28)),
             (f"{tag}.params_over_stats", make(struct_size=36, stats=8)), (f"{tag}.stats_struct_size", make(stats=64)),
             (f"{tag}.stats_over_mode", make(stats=0, mode=2)), (f"{tag}.mode_2", make(mode=2)), (f"{tag}.mode_-1", make(mode=-1)),
             (f"{tag}.mode_over_flags", make(mode=2, flags=0x80)), (f"{tag}.flags", make(flags=flag_names_bits)), (f"{tag}.flags_all", make(flags=0xFFFFFFFF)),
             (f"{tag}.reserved_0", make(reserved=0)), (f"{tag}.reserved_1", make(reserved=1)), (f"{tag}.streams_-1", make(streams=-1)),
             (f"{tag}.streams_65", make(streams=65, samples=65)), (f"{tag}.samples_0", make(samples=0)), (f"{tag}.samples_-8", make(samples=-8)),
             (f"{tag}.samples_6_streams_4", make(samples=6)), (f"{tag}.samples_1_streams_2", make(samples=1, streams=2)),
             (f"{tag}.ray_depth_17", make(ray_depth=17)), (f"{tag}.multiple_over_depth", make(samples=6, ray_depth=17)),
             (f"{tag}.points_2^25_streams_64", make(n=2**25, streams=64, samples=64)), (f"{tag}.points_2^31", make(n=2**31, streams=1))]
    cases += extra
    cases += [(f"{tag}.null_{a}", make(drop=(a,))) for a in ("points", "rng", "out")]
    cases += [(f"{tag}.engine_0_at_0", _rng_x(0, 0, make())), (f"{tag}.engine_2^31-1_at_31", _rng_x(POINTS * K - 1, 2**31 - 1, make())),
              (f"{tag}.engine_beyond_streams", _rng_x(POINTS, 0, make(streams=1, samples=1))), (f"{tag}.engine_device_array", _rng_x(0, 0, make(flags=DEV))),
              (f"{tag}.null_scene", make()), (f"{tag}.null_scene_defaults", make(streams=0, ray_depth=0, mode=0, flags=DEV)),
              (f"{tag}.null_scene_n_0", make(n=0, drop=("points", "rng", "out"), stats=None))]
    return cases


HOST = (_walk_host("rt_query_closest", closest) + _walk_host("rt_query_light_pdf", light_pdf)
        + [("rt_query_occluded.struct_size", occluded(stats=8)), ("rt_query_occluded.struct_size_over_flags", occluded(stats=80, flags=4)),
           ("rt_query_occluded.flags_4", occluded(flags=4)), ("rt_query_occluded.flags_over_rays", occluded(flags=0x80000000, drop=("rays",))),
           ("rt_query_occluded.null_rays", occluded(drop=("rays", "occ"))), ("rt_query_occluded.null_out", occluded(drop=("occ",))),
           ("rt_query_occluded.null_tmax_null_scene", occluded(drop=("tmax",))), ("rt_query_occluded.null_scene", occluded()),
           ("rt_query_occluded.null_scene_n_0", occluded(n=0, drop=("rays", "occ"), stats=None))]
        + _walk_host("rt_query_surface", surface) + _walk_host("rt_query_environment", environment)
        + [("rt_camera_rays.null_scene", camera_rays()), ("rt_camera_rays.null_scene_over_width", camera_rays(w=0, flags=8)),
           ("rt_render_guides.struct_size", guides(stats=8)), ("rt_render_guides.null_scene", guides()), ("rt_render_guides.null_scene_over_width", guides(w=0, stats=None))]
        + _bounce_host("rt_query_scatter", scatter, ("rays", "hits", "surfaces", "rng", "scatter"), True)
        + _bounce_host("rt_query_bsdf", bsdf, ("rays", "hits", "surfaces", "dirs", "rgb", "pdf"), False)
        + _bounce_host("rt_trace_paths", trace_paths, ("rays", "rng", "rgb"), True)
        + [("rt_trace_paths.depth_17_null_scene", trace_paths(depth=17))]
        + [("rt_bake_rays.struct_size", bake_rays(stats=8)), ("rt_bake_rays.struct_size_over_mode", bake_rays(stats=80, mode=2)),
           ("rt_bake_rays.mode_2", bake_rays(mode=2)), ("rt_bake_rays.mode_-1", bake_rays(mode=-1)), ("rt_bake_rays.mode_over_flags", bake_rays(mode=27, flags=2)),
           ("rt_bake_rays.flags_2", bake_rays(flags=2, mode=1)), ("rt_bake_rays.flags_all", bake_rays(flags=0xFFFFFFFF)),
           ("rt_bake_rays.flags_over_null", bake_rays(flags=4, drop=("points",)))]
        + [(f"rt_bake_rays.null_{a}", bake_rays(drop=(a,))) for a in ("points", "rng", "rays")]
        + [("rt_bake_rays.engine_0_at_0", _rng_x(0, 0, bake_rays())), ("rt_bake_rays.engine_2^32-1_at_3", _rng_x(N - 1, 2**32 - 1, bake_rays())),
           ("rt_bake_rays.engine_beyond_n", _rng_x(N, 0, bake_rays())), ("rt_bake_rays.engine_device_array", _rng_x(0, 0, bake_rays(flags=DEV))),
           ("rt_bake_rays.null_scene", bake_rays(mode=1)), ("rt_bake_rays.null_scene_n_0", bake_rays(n=0, drop=("points", "rng", "rays"), stats=None))]
        + _baker_host("rt_bake", bake, 8, [])
        + [(f"rt_render_paths.null_{a}", render_paths(drop=(a,))) for a in ("rays", "rng", "rgb")]
        + [("rt_render_paths.null_over_struct_size", render_paths(drop=("rays",), stats=8)), ("rt_render_paths.struct_size", render_paths(stats=8)),
           ("rt_render_paths.struct_size_over_flags", render_paths(stats=80, flags=2)), ("rt_render_paths.flags_2", render_paths(flags=2)),
           ("rt_render_paths.flags_all", render_paths(flags=0xFFFFFFFF)), ("rt_render_paths.flags_over_engine", _rng_x(0, 0, render_paths(flags=2))),
           ("rt_render_paths.engine_0_at_0", _rng_x(0, 0, render_paths())), ("rt_render_paths.engine_over_depth", _rng_x(N - 1, 2**31 - 1, render_paths(depth=17))),
           ("rt_render_paths.engine_beyond_n", _rng_x(N, 0, render_paths())), ("rt_render_paths.engine_device_array", _rng_x(0, 0, render_paths(flags=DEV))),
           ("rt_render_paths.depth_17", render_paths(depth=17)), ("rt_render_paths.depth_1000", render_paths(depth=1000)),
           ("rt_render_paths.null_scene", render_paths(depth=16)), ("rt_render_paths.null_scene_n_0", render_paths(n=0, drop=("rays", "rng", "rgb"), stats=None))]
        + _baker_host("rt_render_bake", render_bake, 2, [
            ("rt_render_bake.per_stream_2^25", render_bake(samples=2**25, streams=1)), ("rt_render_bake.per_stream_2^25_streams_2", render_bake(samples=2**26, streams=2)),
            ("rt_render_bake.points_over_per_stream", render_bake(n=2**31, samples=2**25, streams=1)), ("rt_render_bake.sh9", render_bake(mode=1)),
            ("rt_render_bake.per_stream_over_sh9", render_bake(mode=1, samples=2**25, streams=1)), ("rt_render_bake.sh9_over_null", render_bake(mode=1, drop=("points",)))]))


# ---- on a GPU: a live scene, device arrays ------------------------------------------------------------------------------------------
def _flavor_and_flags(tag, make, bad_flags):
    return [(f"{tag}.flags", make(scene="hw8", flags=bad_flags)), (f"{tag}.flags_over_flavor", make(scene="hw6", flags=bad_flags)), (f"{tag}.flavor", make(scene="hw6"))]


def _misaligned(tag, make, arrays, flags=DEV, **kw):
    """Each array in turn offset into its allocation; host arrays with the same offsets are no refusal and are not asked."""
    return [(f"{tag}.{a}+{by}", make(scene="hw8", flags=flags, off={a: by}, **kw)) for a, by in arrays]


GPU = (_flavor_and_flags("rt_query_closest", closest, 4)
       + [("rt_query_closest.null_rays", closest(scene="hw8", drop=("rays",))), ("rt_query_closest.null_out", closest(scene="hw8", drop=("hits",))),
          ("rt_query_closest.null_over_alignment", closest(scene="hw8", flags=DEV, drop=("rays",), off={"hits": 4}))]
       + _misaligned("rt_query_closest", closest, (("hits", 4), ("hits", 8)))
       + _flavor_and_flags("rt_query_light_pdf", light_pdf, 4)
       + [("rt_query_light_pdf.no_lights", light_pdf(scene="dark")), ("rt_query_light_pdf.no_lights_over_null", light_pdf(scene="dark", drop=("rays",))),
          ("rt_query_light_pdf.null_rays", light_pdf(scene="hw8", drop=("rays",))), ("rt_query_light_pdf.null_out", light_pdf(scene="hw8", drop=("pdf",)))]
       + [("rt_query_occluded.flavor", occluded(scene="hw6"))] + _misaligned("rt_query_occluded", occluded, (("tmax", 1), ("tmax", 2)))
       + _flavor_and_flags("rt_query_surface", surface, 2)
       + [("rt_query_surface.null_hits", surface(scene="hw8", drop=("hits",))), ("rt_query_surface.null_out", surface(scene="hw8", drop=("surfaces",)))]
       + _misaligned("rt_query_surface", surface, (("hits", 4), ("surfaces", 4)))
       + _flavor_and_flags("rt_query_environment", environment, 2)
       + [("rt_query_environment.null_rays", environment(scene="hw8", drop=("rays",))), ("rt_query_environment.null_out", environment(scene="hw8", drop=("rgb",)))]
       + _flavor_and_flags("rt_camera_rays", camera_rays, 2)
       + [("rt_camera_rays.width_0", camera_rays(scene="hw8", w=0)), ("rt_camera_rays.height_-1", camera_rays(scene="hw8", h=-1)),
          ("rt_camera_rays.width_over_null", camera_rays(scene="hw8", w=0, drop=("xy",))), ("rt_camera_rays.null_xy", camera_rays(scene="hw8", drop=("xy",))),
          ("rt_camera_rays.null_out", camera_rays(scene="hw8", drop=("rays",))), ("rt_camera_rays.xy_nan", _xy(np.nan, camera_rays(scene="hw8"))),
          ("rt_camera_rays.xy_inf", _xy(np.inf, camera_rays(scene="hw8")))]
       + _flavor_and_flags("rt_render_guides", guides, 2)
       + [("rt_render_guides.width_0", guides(scene="hw8", w=0)), ("rt_render_guides.height_0", guides(scene="hw8", h=0)),
          ("rt_render_guides.too_large", guides(scene="hw8", w=65536, h=32768)), ("rt_render_guides.too_large_2^31-1", guides(scene="hw8", w=2147483647, h=1))]
       + [("rt_query_scatter.flavor", scatter(scene="hw6"))]
       + _misaligned("rt_query_scatter", scatter, (("hits", 4), ("surfaces", 4), ("rng", 4), ("scatter", 8)))
       + [("rt_query_bsdf.flavor", bsdf(scene="hw6"))]
       + _misaligned("rt_query_bsdf", bsdf, (("hits", 4), ("surfaces", 4), ("dirs", 1), ("rgb", 1), ("pdf", 2)))
       + [("rt_query_bsdf.16_over_4", bsdf(scene="hw8", flags=DEV, off={"hits": 4, "dirs": 1}))]
       + [("rt_trace_paths.flavor", trace_paths(scene="hw6")), ("rt_trace_paths.flavor_over_depth", trace_paths(scene="hw6", depth=17)),
          ("rt_trace_paths.depth_17", trace_paths(scene="hw8", depth=17)), ("rt_trace_paths.depth_over_alignment", trace_paths(scene="hw8", depth=17, flags=DEV, off={"rng": 4}))]
       + _misaligned("rt_trace_paths", trace_paths, (("rng", 4), ("rays", 1), ("rgb", 1)))
       + [("rt_trace_paths.16_over_4", trace_paths(scene="hw8", flags=DEV, off={"rng": 4, "rays": 1}))]
       + [("rt_bake_rays.flavor", bake_rays(scene="hw6"))] + _misaligned("rt_bake_rays", bake_rays, (("rng", 8), ("points", 1), ("rays", 2)))
       + [("rt_bake.flavor", bake(scene="hw6"))] + _misaligned("rt_bake", lambda flags, **kw: bake(flags=flags | REF | LOCKSTEP, **kw), (("rng", 4), ("points", 1), ("out", 1)))
       + [("rt_render_paths.flavor", render_paths(scene="hw6"))] + _misaligned("rt_render_paths", render_paths, (("rng", 4), ("rays", 1), ("rgb", 1)))
       + [("rt_render_paths.alignment_over_pipeline", _env("RTAMD_KERNEL", "wavefront", render_paths(scene="hw8", flags=DEV, off={"rng": 4}))),
          ("rt_render_paths.wavefront", _env("RTAMD_KERNEL", "wavefront", render_paths(scene="hw8"))),
          ("rt_render_paths.wavefront_n_0", _env("RTAMD_KERNEL", "wavefront", render_paths(scene="hw8", n=0))),
          ("rt_render_paths.mega", _env("RTAMD_KERNEL", "mega", render_paths(scene="hw8")))]
       + [("rt_render_bake.flavor", render_bake(scene="hw6"))] + _misaligned("rt_render_bake", render_bake, (("rng", 4), ("points", 1), ("out", 1)))
       + [("rt_render_bake.wavefront", _env("RTAMD_KERNEL", "wavefront", render_bake(scene="hw8"))),
          ("rt_render_bake.wavefront_n_0", _env("RTAMD_KERNEL", "wavefront", render_bake(scene="hw8", n=0))),
          ("rt_render_bake.mega", _env("RTAMD_KERNEL", "mega", render_bake(scene="hw8")))])


def _line(c, name, fn):
    rc = fn(c)
    return f"{name}, {rc}, " + c.lib.rt_last_error().decode("utf-8", "replace")


def run_host(rt):
    """The lines of HOST: no call reaches HIP, with or without a GPU."""
    c = Ctx(rt)
    return [_line(c, name, fn) for name, fn in HOST]


def run_gpu(rt):
    """The lines of GPU, on device 0.  torch opens the GPU before the library does (the order bench.py keeps): call this in a process
    of its own."""
    import torch
    c = Ctx(rt, torch)
    c.scenes = {"hw8": rt.Scene(rt.load_gltf(os.path.join(SPHERE_DIR, "sphere_emissive.gltf"))),
                "hw6": rt.Scene(rt.load_gltf(os.path.join(SPHERE_DIR, "sphere_emissive.gltf"), flavor=rt.RT_INTEGRATOR_HW6)),
                "dark": rt.Scene(rt.load_gltf(os.path.join(SPHERE_DIR, "sphere.gltf")))}
    assert c.scenes["dark"].info().n_lights == 0 and c.scenes["hw8"].info().n_lights > 0
    lines = [_line(c, name, fn) for name, fn in GPU]
    for s in c.scenes.values():
        s.close()
    return lines


if __name__ == "__main__":  # python tests/query_refusal_cases.py host|gpu FILE: writes the transcript ("-": to stdout)
    import importlib
    if sys.argv[1] == "gpu":
        import torch
        torch.zeros(1, device="cuda")  # torch first, as bench.py has it: one HIP runtime serves both
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-course-hw_amd")
    lines = run_host(rt) + (run_gpu(rt) if sys.argv[1] == "gpu" else [])
    if sys.argv[2] == "-":
        print("\n".join(lines))
    else:
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{len(lines)} lines -> {sys.argv[2]}")

"""rt_render_paths and rt_render_bake, the part that needs no GPU: the header declares them under ABI 6, the library exports them and
the package binds them; every refusal that is decided before the scene is looked at arrives on a null scene with a message naming
what is wrong, and writes nothing.  The pattern is tests/test_bake_host.py's."""
import ctypes as C
import os
import re

import numpy as np

import scatter_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
F = np.float32


def test_header_declares_the_calls_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    for proto in (r"^int rt_render_paths\(rt_scene \*\w*, const rt_ray \*\w+, rt_rng \*\w+[^,]*, size_t \w+, int32_t \w+,\s+uint32_t \w+, float \*\w+[^,]*, rt_query_stats \*\w+",
                  r"^int rt_render_bake\(rt_scene \*\w*, const rt_bake_point \*\w+, size_t \w+, const rt_bake_params \*\w+,\s+rt_rng \*\w+ /\*[^/]*\*/, float \*\w+[^,]*, rt_bake_stats \*\w+"):
        assert re.search(proto, text, re.M), proto


def test_library_exports_and_package_binds_them(rt):
    for fn in ("rt_render_paths", "rt_render_bake"):
        assert fn in rt.ABI_SYMBOLS and hasattr(rt.lib, fn), fn
    assert rt.lib.rt_abi_version() == 6
    for name in ("render_paths", "render_bake"):
        assert callable(getattr(rt.Scene, name)) and callable(getattr(rt.Scene, name + "_device")), name
    assert (len(rt.lib.rt_render_paths.argtypes), len(rt.lib.rt_render_bake.argtypes)) == (8, 7)


class _Raw:
    """Raw calls on eight points of four streams, or 32 rays, and a null scene; nothing may be written."""

    def __init__(self, rt):
        self.rt = rt
        self.points = rt.pack_bake_points(np.zeros((8, 3), F), np.tile(np.array([0, 1, 0], F), (8, 1)))
        self.rays = rt.pack_rays(np.zeros((32, 3), F), np.tile(np.array([0, 0, -1], F), (32, 1)))
        self.rng = model.seed(1 + 7919 * np.arange(32))
        self.before = self.rng.copy()
        self.out = np.zeros((32, 3), F)

    def _done(self, code):
        assert not self.out.any() and np.array_equal(self.rng, self.before)
        return code, self.rt.lib.rt_last_error().decode()

    def paths_call(self, n=32, depth=0, flags=0, stats=None, drop=None):
        p = {k: (None if k == drop else v.ctypes.data) for k, v in (("rays", self.rays), ("rng", self.rng), ("out", self.out))}
        return self._done(self.rt.lib.rt_render_paths(None, p["rays"], p["rng"], n, depth, flags, p["out"], C.byref(stats) if stats is not None else None))

    def bake_call(self, n=8, stats=None, drop=None, params="made", **fields):
        made = self.rt.make_bake_params(8, 4, self.rt.RT_BAKE_IRRADIANCE, 4)
        for k, v in fields.items():
            if k == "reserved":
                made.reserved[v] = 1
            else:
                setattr(made, k, v)
        p = {k: (None if k == drop else v.ctypes.data) for k, v in (("points", self.points), ("rng", self.rng), ("out", self.out))}
        return self._done(self.rt.lib.rt_render_bake(None, p["points"], n, C.byref(made) if params == "made" else None, p["rng"], p["out"],
                                                     C.byref(stats) if stats is not None else None))


def test_render_paths_refusals_that_need_no_device(rt):
    raw, fn, bad, limit = _Raw(rt), "rt_render_paths: ", rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    assert raw.paths_call() == (bad, fn + "null argument")                                       # everything in order but the scene
    assert raw.paths_call(depth=16, flags=rt.RT_QUERY_DEVICE_POINTERS) == (bad, fn + "null argument")
    for drop in ("rays", "rng", "out"):
        assert raw.paths_call(drop=drop) == (bad, fn + "null argument"), drop
    for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
        st = rt.rt_query_stats()
        st.struct_size = size
        assert raw.paths_call(stats=st) == (bad, fn + "struct_size mismatch (ABI skew)")
    for flags in (2, 4, 8, 0x80000000, 1 | 2):
        assert raw.paths_call(flags=flags) == (bad, fn + "flags other than RT_QUERY_DEVICE_POINTERS"), flags
    for depth in (17, 1000):
        assert raw.paths_call(depth=depth) == (limit, fn + "ray_depth above 16")
    for x in (0, 2**31 - 1, 2**32 - 1):
        for at in (0, 31):
            raw.rng["x"][at] = raw.before["x"][at] = x
            assert raw.paths_call() == (bad, fn + f"rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)")
            assert raw.paths_call(flags=rt.RT_QUERY_DEVICE_POINTERS) == (bad, fn + "null argument")  # a device array is not the host's to read
            raw.rng["x"][at] = raw.before["x"][at] = 1 + at
    raw.rng["x"][8] = raw.before["x"][8] = 0                                                     # beyond the n records: not the call's to judge
    assert raw.paths_call(n=8) == (bad, fn + "null argument")


def test_render_bake_refusals_that_need_no_device(rt):
    raw, fn, bad, limit = _Raw(rt), "rt_render_bake: ", rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    assert raw.bake_call() == (bad, fn + "null argument (scene)")                                # everything in order but the scene
    assert raw.bake_call(streams=0, ray_depth=0, flags=1) == (bad, fn + "null argument (scene)")
    assert raw.bake_call(ray_depth=16, streams=1, samples=1) == (bad, fn + "null argument (scene)")
    assert raw.bake_call(params=None) == (bad, fn + "null argument (params)")
    for size in (0, 28, 36):
        assert raw.bake_call(struct_size=size) == (bad, fn + "params.struct_size mismatch (ABI skew)")
    for size in (0, C.sizeof(rt.rt_bake_stats) - 8, C.sizeof(rt.rt_query_stats)):
        st = rt.rt_bake_stats()
        st.struct_size = size
        assert raw.bake_call(stats=st) == (bad, fn + "stats.struct_size mismatch (ABI skew)")
    for mode in (2, -1):
        assert raw.bake_call(mode=mode) == (bad, fn + f"params.mode = {mode} is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9")
    for flags in (2, 4, 8, 0x80000000, 1 | 4):
        assert raw.bake_call(flags=flags) == (bad, fn + "params.flags other than RT_QUERY_DEVICE_POINTERS"), flags
    for word in (0, 1):
        assert raw.bake_call(reserved=word) == (bad, fn + "params.reserved must be zero")
    for samples in (0, -8):
        assert raw.bake_call(samples=samples) == (bad, fn + "params.samples must be at least 1")
    assert raw.bake_call(streams=65, samples=65) == (limit, fn + "params.streams above 64")
    assert raw.bake_call(streams=-1) == (bad, fn + "params.streams must not be negative")
    for samples, streams in ((6, 4), (63, 64), (1, 2)):
        assert raw.bake_call(samples=samples, streams=streams) == (bad, fn + f"params.samples = {samples} is no multiple of params.streams = {streams}")
    for depth in (17, 1000):
        assert raw.bake_call(ray_depth=depth) == (limit, fn + "params.ray_depth above 16")
    for n, streams in ((2**25, 64), (2**31, 1), (2**31 // 3 + 1, 3)):
        assert raw.bake_call(n=n, streams=streams, samples=192) == (limit, fn + "n_points * params.streams must stay below 2^31")
    for samples, streams in ((2**25, 1), (2**26, 2)):
        assert raw.bake_call(samples=samples, streams=streams) == (limit, fn + "params.samples / params.streams must stay below 2^25 (the path record's sample index)")
    assert raw.bake_call(samples=2**25 - 1, streams=1) == (bad, fn + "null argument (scene)")
    code, msg = raw.bake_call(mode=rt.RT_BAKE_SH9)
    assert code == rt.RT_ERR_UNSUPPORTED and msg.startswith(fn + "RT_BAKE_SH9") and "rt_bake serves it" in msg
    for drop in ("points", "rng", "out"):
        assert raw.bake_call(drop=drop) == (bad, fn + "null argument"), drop
    for x in (0, 2**31 - 1):
        for at in (0, 31):
            raw.rng["x"][at] = raw.before["x"][at] = x
            assert raw.bake_call() == (bad, fn + f"rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)")
            assert raw.bake_call(flags=rt.RT_QUERY_DEVICE_POINTERS) == (bad, fn + "null argument (scene)")
            raw.rng["x"][at] = raw.before["x"][at] = 1 + at

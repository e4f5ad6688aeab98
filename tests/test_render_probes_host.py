"""rt_render_probes, the part that needs no GPU: the header declares it under ABI 6, the library exports it and the package binds it;
every refusal that is decided before the scene is looked at arrives on a null scene with its exact message, and writes nothing -- not
the 27 floats per point, not the engines, not the caller's stats.  The pattern is tests/test_render_paths_host.py's."""
import ctypes as C
import os
import re

import numpy as np

import scatter_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
F = np.float32
FN = "rt_render_probes: "


def test_header_declares_the_call_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    proto = (r"^int rt_render_probes\(rt_scene \*\w+, const rt_bake_point \*\w+, size_t \w+, const rt_bake_params \*\w+,\s+"
             r"rt_rng \*\w+ /\*[^/]*\*/, float \*\w+ /\* n_points\*27[^/]*\*/,\s+rt_bake_stats \*\w+ /\* nullable \*/\);")
    assert re.search(proto, text, re.M), proto


def test_library_exports_and_package_binds_it(rt):
    assert "rt_render_probes" in rt.ABI_SYMBOLS and hasattr(rt.lib, "rt_render_probes")
    assert rt.lib.rt_abi_version() == 6
    assert callable(rt.Scene.render_probes) and callable(rt.Scene.render_probes_device)
    assert len(rt.lib.rt_render_probes.argtypes) == 7 and rt.lib.rt_render_probes.argtypes == rt.lib.rt_bake.argtypes


class _Raw:
    """Raw calls on eight points of four streams and a null scene; nothing may be written."""

    def __init__(self, rt):
        self.rt = rt
        self.points = rt.pack_bake_points(np.zeros((8, 3), F), np.tile(np.array([0, 1, 0], F), (8, 1)))
        self.rng = model.seed(1 + 7919 * np.arange(32))
        self.before = self.rng.copy()
        self.out = np.zeros((8, 27), F)

    def call(self, n=8, stats=None, drop=None, params="made", **fields):
        made = self.rt.make_bake_params(8, 4, self.rt.RT_BAKE_SH9, 4)
        for k, v in fields.items():
            if k == "reserved":
                made.reserved[v] = 1
            else:
                setattr(made, k, v)
        p = {k: (None if k == drop else v.ctypes.data) for k, v in (("points", self.points), ("rng", self.rng), ("out", self.out))}
        seen = bytes(stats) if stats is not None else None
        code = self.rt.lib.rt_render_probes(None, p["points"], n, C.byref(made) if params == "made" else None, p["rng"], p["out"],
                                            C.byref(stats) if stats is not None else None)
        assert not self.out.any() and np.array_equal(self.rng, self.before)
        assert stats is None or bytes(stats) == seen
        return code, self.rt.lib.rt_last_error().decode()


def _stats(rt, size=None):
    st = rt.rt_bake_stats()
    C.memset(C.byref(st), 0xA5, C.sizeof(st))                  # a refusal leaves the caller's stats as they were
    st.struct_size = C.sizeof(st) if size is None else size
    return st


def test_refusals_that_need_no_device(rt):
    raw, bad, limit = _Raw(rt), rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    scene = (bad, FN + "null argument (scene)")                 # everything in order but the scene
    assert raw.call() == scene
    assert raw.call(stats=_stats(rt)) == scene
    assert raw.call(streams=0, ray_depth=0, flags=rt.RT_QUERY_DEVICE_POINTERS) == scene
    assert raw.call(ray_depth=16, streams=1, samples=1) == scene
    assert raw.call(streams=64, samples=64, n=0, drop="points") == scene
    # null arguments and struct_size
    assert raw.call(params=None) == (bad, FN + "null argument (params)")
    for drop in ("points", "rng", "out"):
        assert raw.call(drop=drop) == (bad, FN + "null argument"), drop
    for size in (0, 28, 36):
        assert raw.call(struct_size=size) == (bad, FN + "params.struct_size mismatch (ABI skew)")
    for size in (0, C.sizeof(rt.rt_bake_stats) - 8, C.sizeof(rt.rt_query_stats)):
        assert raw.call(stats=_stats(rt, size)) == (bad, FN + "stats.struct_size mismatch (ABI skew)")
    # reserved words and flags
    for word in (0, 1):
        assert raw.call(reserved=word) == (bad, FN + "params.reserved must be zero")
    for flags in (2, 4, 8, 0x80000000, 1 | 4, rt.RT_BAKE_LOCKSTEP):
        assert raw.call(flags=flags) == (bad, FN + "params.flags other than RT_QUERY_DEVICE_POINTERS"), flags
    # the mode: neither, and the one rt_render_bake serves
    for mode in (2, -1):
        assert raw.call(mode=mode) == (bad, FN + f"params.mode = {mode} is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9")
    irradiance = (bad, FN + "params.mode = RT_BAKE_IRRADIANCE: this call bakes RT_BAKE_SH9 probes, rt_render_bake serves irradiance")
    assert raw.call(mode=rt.RT_BAKE_IRRADIANCE) == irradiance
    assert raw.call(mode=rt.RT_BAKE_IRRADIANCE, stats=_stats(rt)) == irradiance
    assert raw.call(mode=rt.RT_BAKE_IRRADIANCE, drop="points") == irradiance      # decided before the arrays are looked at
    # streams, slots, samples
    assert raw.call(streams=65, samples=65) == (limit, FN + "params.streams above 64")
    assert raw.call(streams=-1) == (bad, FN + "params.streams must not be negative")
    for samples in (0, -8):
        assert raw.call(samples=samples) == (bad, FN + "params.samples must be at least 1")
    for n, streams in ((2**25, 64), (2**31, 1), (2**31 // 3 + 1, 3)):
        assert raw.call(n=n, streams=streams, samples=192) == (limit, FN + "n_points * params.streams must stay below 2^31")
    for samples, streams in ((6, 4), (63, 64), (1, 2)):
        assert raw.call(samples=samples, streams=streams) == (bad, FN + f"params.samples = {samples} is no multiple of params.streams = {streams}")
    for samples, streams in ((2**25, 1), (2**26, 2)):
        assert raw.call(samples=samples, streams=streams) == (limit, FN + "params.samples / params.streams must stay below 2^25 (the path record's sample index)")
    assert raw.call(samples=2**25 - 1, streams=1) == scene
    assert raw.call(samples=2**25, streams=1, mode=rt.RT_BAKE_IRRADIANCE)[0] == limit  # the limit is judged before the mode
    for depth in (17, 1000):
        assert raw.call(ray_depth=depth) == (limit, FN + "params.ray_depth above 16")
    # a host engine outside 1 .. 2^31-2, at a named index; a device array is not the host's to read
    for x in (0, 2**31 - 1):
        for at in (0, 13, 31):
            raw.rng["x"][at] = raw.before["x"][at] = x
            assert raw.call() == (bad, FN + f"rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)")
            assert raw.call(flags=rt.RT_QUERY_DEVICE_POINTERS) == scene
            raw.rng["x"][at] = raw.before["x"][at] = 1 + at
    raw.rng["x"][16] = raw.before["x"][16] = 0                  # beyond the 4 x 4 engines of the call: not its to judge
    assert raw.call(n=4) == scene


def test_no_points_need_no_arrays(rt):
    """n_points == 0 with null arrays: nothing about the arrays is refused, the one thing left to name is the null scene.  On a scene the
    call is RT_OK without a launch (tests/test_gpu_render_probes.py: a scene needs a GPU)."""
    params = rt.make_bake_params(8, 4, rt.RT_BAKE_SH9, 4)
    assert rt.lib.rt_render_probes(None, None, 0, C.byref(params), None, None, None) == rt.RT_ERR_INVALID_ARG
    assert rt.lib.rt_last_error().decode() == FN + "null argument (scene)"

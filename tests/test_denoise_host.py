"""Denoised previews, host side (no GPU): rt_denoise and rt_accum_denoise are declared, exported and bound, the ABI is still 6, the
structs have the binding's sizes, and everything the two calls refuse before any device work answers its code and names its field.
Those checks look at the handle only for NULL, so a block of zeros stands in for a scene and for an accumulator here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARG, RT_ERR_LIMIT = -1, -7


def test_symbols_are_declared_exported_and_bound(rt):
    header = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    declared = set(re.findall(r"^extern int (rt_[a-z_]*denoise)\(", header, re.M))
    assert declared == {"rt_denoise", "rt_accum_denoise"}
    for name in declared:
        assert name in rt.DENOISE_SYMBOLS and hasattr(rt.lib, name), name
    assert rt.lib.rt_abi_version() == 6 and "#define RTAMD_ABI_VERSION 6" in header
    assert C.sizeof(rt.rt_render_params) == 64 and C.sizeof(rt.rt_stats) == 96 and C.sizeof(rt.rt_noise_summary) == 64
    for struct, size in ((rt.rt_denoise_params, 32), (rt.rt_denoise_stats, 32)):
        name = struct.__name__
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        names = []
        for line in re.findall(r"^\s*(?:uint32_t|int32_t|uint64_t|double|float)\s+([a-z_, ]+);", fields, re.M):
            names += [n.strip() for n in line.split(",")]
        assert names == [f[0] for f in struct._fields_] and C.sizeof(struct) == size, name
    assert f"#define RT_DENOISE_DEVICE_POINTERS {rt.RT_DENOISE_DEVICE_POINTERS}u" in header
    assert f"#define RT_DENOISE_ALBEDO          {rt.RT_DENOISE_ALBEDO}u" in header
    for cls, methods in ((rt.Scene, ("denoise", "denoise_device")), (rt.Accumulator, ("denoise",))):
        assert all(callable(getattr(cls, m)) for m in methods)
    assert not hasattr(rt.MultiAccumulator, "denoise")   # out of scope: frames of rt_multi_* go through Scene.denoise


class Call:
    """One call of either function with good arguments, any of which a case replaces."""

    def __init__(self, rt, which):
        self.rt, self.which = rt, which
        self.handle = C.create_string_buffer(4096)   # never read: the checks under test come before the handle is looked into
        self.planes = {k: (C.c_float * 48)() for k in ("rgb", "normal", "depth")}
        self.out = (C.c_float * 48)()
        self.out8 = (C.c_uint8 * 48)()
        self.stats = rt.rt_denoise_stats()
        self.stats.struct_size = C.sizeof(rt.rt_denoise_stats)

    def __call__(self, params="default", handle="default", out="default", out8="default", stats="default", **planes):
        rt = self.rt
        p = rt.make_denoise_params(4, 4) if params == "default" else params
        h = self.handle if handle == "default" else handle
        o = self.out if out == "default" else out
        o8 = self.out8 if out8 == "default" else out8
        st = C.byref(self.stats) if stats == "default" else stats
        pp = None if p is None else C.byref(p)
        rt.lib.rt_load_gltf(b"/nonexistent.gltf", 8, C.byref(C.c_void_p()))   # leaves some other message behind
        if self.which == "rt_denoise":
            pl = [planes.get(k, self.planes[k]) for k in ("rgb", "normal", "depth")]
            code = rt.lib.rt_denoise(h, pp, *pl, None, None, None, o, o8, st)
        else:
            code = rt.lib.rt_accum_denoise(h, None, pp, o, o8, st)
        return code, rt.lib.rt_last_error().decode()


def _params(rt, **fields):
    p = rt.make_denoise_params(4, 4)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


PARAM_CASES = [("struct_size", dict(struct_size=28)), ("struct_size", dict(struct_size=0)), ("reserved", dict(reserved=1)),
               ("flags", dict(flags=4)), ("flags", dict(flags=0x80000001)), ("iterations", dict(iterations=-1)), ("iterations", dict(iterations=9)),
               ("sigma_depth", dict(sigma_depth=-1.0)), ("sigma_depth", dict(sigma_depth=float("nan"))), ("sigma_depth", dict(sigma_depth=float("inf"))),
               ("sigma_luminance", dict(sigma_luminance=-0.5)), ("sigma_luminance", dict(sigma_luminance=float("nan"))),
               ("sigma_luminance", dict(sigma_luminance=float("-inf")))]


@pytest.mark.parametrize("which", ["rt_denoise", "rt_accum_denoise"])
def test_bad_params_are_invalid_arguments_that_name_the_field(rt, which):
    call = Call(rt, which)
    for field, change in PARAM_CASES:
        code, msg = call(params=_params(rt, **change))
        assert code == RT_ERR_INVALID_ARG and msg.startswith(which + ": ") and field in msg, (change, code, msg)
    code, msg = call(params=None)
    assert code == RT_ERR_INVALID_ARG and msg.startswith(which + ": ") and "params" in msg
    code, msg = call(handle=None)
    assert code == RT_ERR_INVALID_ARG and msg.startswith(which + ": ") and ("scene" if which == "rt_denoise" else "accum") in msg
    code, msg = call(out=None, out8=None)
    assert code == RT_ERR_INVALID_ARG and "out_rgb" in msg and "out_rgb8" in msg
    bad_stats = rt.rt_denoise_stats()
    bad_stats.struct_size = 24
    code, msg = call(stats=C.byref(bad_stats))
    assert code == RT_ERR_INVALID_ARG and "stats" in msg and "struct_size" in msg


def test_rt_denoise_refuses_the_albedo_flag_null_planes_and_bad_sizes(rt):
    call = Call(rt, "rt_denoise")
    code, msg = call(params=_params(rt, flags=rt.RT_DENOISE_ALBEDO))     # rt_accum_denoise's flag: there is an albedo argument here
    assert code == RT_ERR_INVALID_ARG and "flags" in msg
    for plane in ("rgb", "normal", "depth"):
        code, msg = call(**{plane: None})
        assert code == RT_ERR_INVALID_ARG and msg == f"rt_denoise: null argument ({plane})"
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -7)):
        code, msg = call(params=_params(rt, width=w, height=h))
        assert code == RT_ERR_INVALID_ARG and "width" in msg and "height" in msg
    for w, h in ((8193, 8192), (1, 2 ** 26 + 1), (2 ** 30, 2 ** 30)):
        code, msg = call(params=_params(rt, width=w, height=h))
        assert code == RT_ERR_LIMIT and "2^26" in msg, (w, h, code, msg)

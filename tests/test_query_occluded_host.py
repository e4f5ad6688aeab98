"""rt_query_occluded, the part that needs no GPU: the header declares it under ABI 6, the library exports it and the package binds it
with its three constants, the refusals that are decided before the scene is looked at name their argument, and the Python wrapper
refuses mismatched shapes before anything reaches C.  (n == 0 needs a scene: tests/test_gpu_query_occluded.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
FN = "rt_query_occluded"


def test_header_declares_the_query_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    for name, value in (("RT_OCCLUSION_OCCLUDED", 1), ("RT_OCCLUSION_EXACT_WALK", 2), ("RT_OCCLUSION_INVALID_RAY", 4)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), text, re.M), name
    assert re.search(r"^int rt_query_occluded\(rt_scene \*\w*, const rt_ray \*\w*, const float \*\w*[^,]*, size_t \w+,\s*uint32_t \w+, uint8_t \*\w*[^,]*, rt_query_stats \*",
                     text, re.M)


def test_library_exports_and_package_binds_it(rt):
    assert FN in rt.ABI_SYMBOLS and hasattr(rt.lib, FN)
    assert rt.lib.rt_abi_version() == 6
    assert (rt.RT_OCCLUSION_OCCLUDED, rt.RT_OCCLUSION_EXACT_WALK, rt.RT_OCCLUSION_INVALID_RAY) == (1, 2, 4)
    assert callable(rt.Scene.query_occluded) and callable(rt.Scene.query_occluded_device)
    assert len(rt.lib.rt_query_occluded.argtypes) == 7


def _call(rt, scene=None, n=4, flags=0, out=True, stats=None):
    rays = rt.pack_rays(np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1)))
    tmax = np.ones(4, np.float32)
    o = np.zeros(4, np.uint8)
    code = rt.lib.rt_query_occluded(scene, rays.ctypes.data, tmax.ctypes.data, n, flags, o.ctypes.data if out else None,
                                    C.byref(stats) if stats is not None else None)
    assert not o.any()
    return code, rt.lib.rt_last_error().decode()


def test_refusals_that_need_no_device(rt):
    code, msg = _call(rt)
    assert code == rt.RT_ERR_INVALID_ARG and msg == FN + ": null argument (scene)"
    code, msg = _call(rt, n=0)
    assert code == rt.RT_ERR_INVALID_ARG and msg == FN + ": null argument (scene)"
    code, msg = _call(rt, out=False)
    assert code == rt.RT_ERR_INVALID_ARG and msg == FN + ": null argument (out)"
    for flags in (4, 8, 0x80000000, 3 | 16):
        code, msg = _call(rt, flags=flags)
        assert code == rt.RT_ERR_INVALID_ARG and msg.startswith(FN + ": flags other than RT_QUERY_DEVICE_POINTERS"), (flags, code, msg)
    for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
        st = rt.rt_query_stats()
        st.struct_size = size
        code, msg = _call(rt, stats=st)
        assert code == rt.RT_ERR_INVALID_ARG and msg == FN + ": struct_size mismatch (ABI skew)", (size, code, msg)


class _NoCalls:
    """Stands in for a Scene whose handle must never be used: the wrapper has to refuse before it calls into C."""
    _h = None


@pytest.mark.parametrize("o,d,tmax", [(np.zeros((4, 3)), np.zeros((5, 3)), None), (np.zeros((4, 3)), np.ones((4, 3)), np.ones(5)),
                                      (np.zeros((4, 3)), np.ones((4, 3)), np.ones((4, 1))), (np.zeros((4, 3)), np.ones((4, 3)), 1.0)])
def test_wrapper_refuses_mismatched_shapes_before_c(rt, o, d, tmax):
    with pytest.raises(ValueError):
        rt.Scene.query_occluded(_NoCalls(), o, d, tmax)


def test_wrapper_refuses_the_device_flag_on_host_arrays(rt):
    with pytest.raises(ValueError):
        rt.Scene.query_occluded(_NoCalls(), np.zeros((1, 3)), np.ones((1, 3)), flags=rt.RT_QUERY_DEVICE_POINTERS)

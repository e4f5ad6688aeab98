"""Batched ray queries, the part that needs no GPU: the header declares them under ABI 6, rt_ray / rt_hit have the sizes the kernels
read and write them by, the ctypes and numpy mirrors agree with the C compiler, and the Python wrappers refuse mismatched shapes
before anything reaches C."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")

SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rtamd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_ray), sizeof(rt_hit), sizeof(rt_query_stats), offsetof(rt_hit, triangle),
           offsetof(rt_hit, ns), offsetof(rt_hit, flags), offsetof(rt_query_stats, kernel_ms));
    return 0;
}
"""


def test_header_declares_the_queries_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    for name in ("rt_ray", "rt_hit", "rt_query_stats"):
        assert re.search(r"^typedef struct %s\b" % name, text, re.M), name
    for name, value in (("RT_HIT_INSIDE", 1), ("RT_HIT_EXACT_WALK", 2), ("RT_HIT_INVALID_RAY", 4), ("RT_QUERY_DEVICE_POINTERS", 1), ("RT_QUERY_REFERENCE_WALK", 2)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), text, re.M), name
    assert re.search(r"^int rt_query_closest\(rt_scene \*\w*, const rt_ray \*\w*, size_t \w+, uint32_t \w+, rt_hit \*\w*, rt_query_stats \*", text, re.M)
    assert re.search(r"^int rt_query_light_pdf\(rt_scene \*\w*, const rt_ray \*\w*, size_t \w+, uint32_t \w+, float \*\w*, rt_query_stats \*", text, re.M)


def test_library_exports_the_queries(rt):
    assert "rt_query_closest" in rt.ABI_SYMBOLS and "rt_query_light_pdf" in rt.ABI_SYMBOLS
    assert hasattr(rt.lib, "rt_query_closest") and hasattr(rt.lib, "rt_query_light_pdf")
    assert rt.lib.rt_abi_version() == 6
    assert (rt.RT_HIT_INSIDE, rt.RT_HIT_EXACT_WALK, rt.RT_HIT_INVALID_RAY) == (1, 2, 4)
    assert (rt.RT_QUERY_DEVICE_POINTERS, rt.RT_QUERY_REFERENCE_WALK) == (1, 2)


def test_struct_sizes_as_the_c_compiler_sees_them(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no C compiler to read include/rtamd.h with"
    src = tmp_path / "sizes.c"
    src.write_text(SIZES_C)
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-x", "c", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 24 and got[1] == 64
    assert got == [C.sizeof(rt.rt_ray), C.sizeof(rt.rt_hit), C.sizeof(rt.rt_query_stats), rt.rt_hit.triangle.offset, rt.rt_hit.ns.offset,
                   rt.rt_hit.flags.offset, rt.rt_query_stats.kernel_ms.offset]
    assert rt.RAY_DTYPE.itemsize == 24 and rt.HIT_DTYPE.itemsize == 64
    for field in ("t", "triangle", "ng", "texcoord", "ns", "tangent", "flags", "reserved"):
        assert rt.HIT_DTYPE.fields[field][1] == getattr(rt.rt_hit, field).offset, field
    assert rt.RAY_DTYPE.fields["d"][1] == rt.rt_ray.d.offset == 12


def test_pack_rays_lays_out_rt_ray(rt):
    o = np.arange(12, dtype=np.float32).reshape(4, 3)
    d = -np.arange(12, dtype=np.float64).reshape(4, 3)
    rays = rt.pack_rays(o, d)
    assert rays.dtype == rt.RAY_DTYPE and rays.shape == (4,) and rays.flags["C_CONTIGUOUS"]
    flat = rays.view(np.float32).reshape(4, 6)
    assert np.array_equal(flat[:, :3], o) and np.array_equal(flat[:, 3:], d.astype(np.float32))
    one = rt.pack_rays([0, 0, 1], [0, 0, -1])
    assert one.shape == (1,)


class _NoCalls:
    """Stands in for a Scene whose handle must never be used: the wrappers have to refuse before they call into C."""
    _h = None

    def _query(self, *a):
        raise AssertionError("the wrapper called into C")


@pytest.mark.parametrize("o,d", [(np.zeros((4, 3)), np.zeros((5, 3))), (np.zeros((4, 2)), np.zeros((4, 2))), (np.zeros((4, 3)), np.zeros(3)),
                                 (np.zeros((2, 2, 3)), np.zeros((2, 2, 3))), (np.zeros(4), np.zeros(4))])
def test_wrappers_refuse_mismatched_shapes_before_c(rt, o, d):
    with pytest.raises(ValueError):
        rt.Scene.query_closest(_NoCalls(), o, d)
    with pytest.raises(ValueError):
        rt.Scene.query_light_pdf(_NoCalls(), o, d)


def test_wrappers_refuse_the_device_flag_on_host_arrays(rt):
    with pytest.raises(ValueError):
        rt.Scene.query_closest(_NoCalls(), np.zeros((1, 3)), np.ones((1, 3)), flags=rt.RT_QUERY_DEVICE_POINTERS)
    with pytest.raises(ValueError):
        rt.Scene.query_light_pdf(_NoCalls(), np.zeros((1, 3)), np.ones((1, 3)), flags=rt.RT_QUERY_DEVICE_POINTERS)

"""The bounce step (rt_rng_*, rt_query_scatter, rt_query_bsdf, rt_trace_paths), the part that needs no GPU: the header declares it under
ABI 6, the library exports it and the package binds it; the two records have the sizes the C compiler sees; rt_rng_seed and
rt_rng_uniform are the oracle's engine; the validity predicate holds on its edge values, through the refusal of a host array that is
decided before the scene is looked at; the wrapper refuses mismatched shapes; and tests/scatter_model.py, fed by the oracle's
per-function answers, folds Hw8Oracle.render's frame -- so the model is checked before it judges the GPU (tests/test_gpu_scatter.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib
import scatter_model as model
import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
CALLS = ["rt_query_scatter", "rt_query_bsdf", "rt_trace_paths"]
EDGE_SEEDS = [0, 1, 2**31 - 2, 2**31 - 1, 2**32 - 1]

SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rtamd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_rng), sizeof(rt_scatter), offsetof(rt_rng, saved), offsetof(rt_rng, has_saved),
           offsetof(rt_scatter, pdf), offsetof(rt_scatter, flags), offsetof(rt_scatter, weight), offsetof(rt_scatter, component), offsetof(rt_scatter, brdf));
    return 0;
}
"""


def test_header_declares_the_calls_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    for name, value in (("RT_SCATTER_END_BRDF", 1), ("RT_SCATTER_END_CLAMP", 2), ("RT_SCATTER_NO_SURFACE", 4), ("RT_SCATTER_INVALID", 8)):
        assert re.search(r"^#define %s\s+%du\b" % (name, value), text, re.M), name
    for proto in (r"^void rt_rng_seed\(rt_rng \*\w+, uint32_t \w+\);", r"^extern float rt_rng_uniform\(rt_rng \*\w+\);",
                  r"^int rt_query_scatter\(rt_scene \*\w*, const rt_ray \*\w+, const rt_hit \*\w+, const rt_surface \*\w+, rt_rng \*\w+",
                  r"^int rt_query_bsdf\(rt_scene \*\w*, const rt_ray \*\w+, const rt_hit \*\w+, const rt_surface \*\w+, const float \*\w+",
                  r"^int rt_trace_paths\(rt_scene \*\w*, const rt_ray \*\w+, rt_rng \*\w+[^,]*, size_t \w+, int32_t \w+"):
        assert re.search(proto, text, re.M), proto


def test_library_exports_and_package_binds_them(rt):
    for fn in CALLS + ["rt_rng_seed"]:
        assert fn in rt.ABI_SYMBOLS and hasattr(rt.lib, fn), fn
    assert rt.RNG_SYMBOLS == ["rt_rng_uniform"] and hasattr(rt.lib, "rt_rng_uniform")
    assert rt.lib.rt_abi_version() == 6
    assert (rt.RT_SCATTER_END_BRDF, rt.RT_SCATTER_END_CLAMP, rt.RT_SCATTER_NO_SURFACE, rt.RT_SCATTER_INVALID) == (1, 2, 4, 8)
    for name in ("query_scatter", "query_bsdf", "trace_paths"):
        assert callable(getattr(rt.Scene, name)) and callable(getattr(rt.Scene, name + "_device")), name
    assert callable(rt.rng_seed) and callable(rt.rng_uniform)
    assert (len(rt.lib.rt_query_scatter.argtypes), len(rt.lib.rt_query_bsdf.argtypes), len(rt.lib.rt_trace_paths.argtypes)) == (9, 10, 8)


def test_struct_sizes_as_the_c_compiler_sees_them(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no C compiler to read include/rtamd.h with"
    src = tmp_path / "sizes.c"
    src.write_text(SIZES_C)
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-x", "c", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [16, 64]
    assert got == [C.sizeof(rt.rt_rng), C.sizeof(rt.rt_scatter), rt.rt_rng.saved.offset, rt.rt_rng.has_saved.offset, rt.rt_scatter.pdf.offset,
                   rt.rt_scatter.flags.offset, rt.rt_scatter.weight.offset, rt.rt_scatter.component.offset, rt.rt_scatter.brdf.offset]
    assert rt.RNG_DTYPE.itemsize == 16 and rt.SCATTER_DTYPE.itemsize == 64
    for struct, dtype in ((rt.rt_rng, rt.RNG_DTYPE), (rt.rt_scatter, rt.SCATTER_DTYPE)):
        for field, _ in struct._fields_:
            assert dtype.fields[field][1] == getattr(struct, field).offset, field


def _seeds():
    return EDGE_SEEDS + [int(s) for s in np.random.default_rng(28).integers(0, 2**32, 1000)]


def test_the_engine_is_the_oracles(rt):
    """rt_rng_seed / rt_rng_uniform, and the model's numpy engine, against rto_rng_kat: 64 draws from each of 1,005 seeds."""
    L = oracle_lib.lib()
    seeds = _seeds()
    want = np.zeros((len(seeds), 64), np.float32)
    for i, s in enumerate(seeds):
        L.rto_rng_kat(s, 64, 0, want[i].ctypes.data)
    rng, mrng = rt.rng_seed(seeds), model.seed(seeds)
    assert np.array_equal(rng, mrng) and not rng["has_saved"].any() and not rng["saved"].any() and not rng["reserved"].any()
    assert rng["x"][:5].tolist() == [1, 1, 2**31 - 2, 1, 1]          # 0 -> 1; 2^31-1 = 0 mod m -> 1; 2^32-1 = 1 mod m
    got = np.stack([rt.rng_uniform(rng) for _ in range(64)], axis=1)
    mgot = np.stack([model.uniform(mrng) for _ in range(64)], axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mgot.view(np.uint32), want.view(np.uint32)) and np.array_equal(rng, mrng)
    assert got.min() >= 0 and got.max() < 1


def test_the_largest_draw_stays_below_one(rt):
    """x' = 2^31 - 2 gives float(2^31 - 3) / 2^31, which rounds to 1: the distribution hands out the float below 1 instead."""
    inv = pow(48271, -1, model.M)
    rng = np.zeros(1, rt.RNG_DTYPE)
    rng["x"] = (model.M - 1) * inv % model.M
    assert rt.rng_uniform(rng)[0] == np.float32(0.99999994) and rng["x"][0] == model.M - 1
    assert model.u01_of(model.M - 1) == np.float32(0.99999994)


def _raw(rt, fn, x=(1, 2, 3, 4), scene=None, n=4, flags=0, stats=None, drop=None):
    """One raw call on four records with the engine states x; `drop` names an array to pass as NULL.  Returns (code, message)."""
    a = {"rays": rt.pack_rays(np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1))),
         "hits": np.zeros(4, rt.HIT_DTYPE), "surfaces": np.zeros(4, rt.SURFACE_DTYPE), "rng": np.zeros(4, rt.RNG_DTYPE),
         "dirs": np.ones((4, 3), np.float32), "out": np.zeros(4, rt.SCATTER_DTYPE), "brdf": np.zeros((4, 3), np.float32), "pdf": np.zeros(4, np.float32)}
    a["rng"]["x"] = x
    p = {k: (None if k == drop else v.ctypes.data) for k, v in a.items()}
    st = C.byref(stats) if stats is not None else None
    if fn == "rt_query_scatter":
        code = rt.lib.rt_query_scatter(scene, p["rays"], p["hits"], p["surfaces"], p["rng"], n, flags, p["out"], st)
    elif fn == "rt_query_bsdf":
        code = rt.lib.rt_query_bsdf(scene, p["rays"], p["hits"], p["surfaces"], p["dirs"], n, flags, p["brdf"], p["pdf"], st)
    else:
        code = rt.lib.rt_trace_paths(scene, p["rays"], p["rng"], n, 0, flags, p["brdf"], st)
    assert not a["out"].view(np.uint32).any() and not a["brdf"].any() and a["rng"]["x"].tolist() == list(x)
    return code, rt.lib.rt_last_error().decode()


@pytest.mark.parametrize("fn", CALLS)
def test_refusals_that_need_no_device(rt, fn):
    code, msg = _raw(rt, fn)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"
    for drop in {"rt_query_scatter": ("rays", "hits", "surfaces", "rng", "out"), "rt_query_bsdf": ("rays", "hits", "surfaces", "dirs", "brdf", "pdf"),
                 "rt_trace_paths": ("rays", "rng", "brdf")}[fn]:
        code, msg = _raw(rt, fn, drop=drop)
        assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument", (drop, code, msg)
    for flags in (4, 8, 0x80000000, 3 | 16):
        code, msg = _raw(rt, fn, flags=flags)
        assert code == rt.RT_ERR_INVALID_ARG and msg.startswith(fn + ": flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK"), (flags, code, msg)
    for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
        st = rt.rt_query_stats()
        st.struct_size = size
        code, msg = _raw(rt, fn, stats=st)
        assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": struct_size mismatch (ABI skew)", (size, code, msg)


@pytest.mark.parametrize("fn", ["rt_query_scatter", "rt_trace_paths"])
def test_a_state_the_engine_never_has_is_refused_before_the_scene(rt, fn):
    """The one predicate (rq_rng_valid) on its edge values: 0, 2^31-1 and everything above are refused and the record is named;
    1 and 2^31-2 pass it, and the call goes on to the missing scene.  The model's restatement agrees."""
    for bad in (0, 2**31 - 1, 2**31, 2**32 - 1):
        assert not model.valid_state(bad)
        for at in (0, 3):
            x = [1, 2, 3, 4]
            x[at] = bad
            code, msg = _raw(rt, fn, x=tuple(x))
            assert code == rt.RT_ERR_INVALID_ARG and msg == f"{fn}: rng[{at}].x = {bad} is no state of the engine (1 .. 2147483646)", (bad, at, msg)
    for good in (1, 2, 2**31 - 3, 2**31 - 2):
        assert model.valid_state(good)
        code, msg = _raw(rt, fn, x=(good, good, 1, 2**31 - 2))
        assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument", (good, msg)
    # a device array is not the host's to read: the sample kernel judges it
    code, msg = _raw(rt, fn, x=(0, 0, 0, 0), flags=rt.RT_QUERY_DEVICE_POINTERS)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"


class _NoCalls:
    """Stands in for a Scene whose handle must never be used: the wrapper has to refuse before it calls into C."""
    _h = None


def test_wrapper_refuses_mismatched_shapes_before_c(rt):
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    hits, surf, rng = np.zeros(4, rt.HIT_DTYPE), np.zeros(4, rt.SURFACE_DTYPE), rt.rng_seed(np.arange(4))
    S = rt.Scene
    bad = [lambda: S.query_scatter(_NoCalls(), o, d[:3], hits, surf, rng), lambda: S.query_scatter(_NoCalls(), o, d, hits[:3], surf, rng),
           lambda: S.query_scatter(_NoCalls(), o, d, hits, surf[:3], rng), lambda: S.query_scatter(_NoCalls(), o, d, hits, surf, rng[:3]),
           lambda: S.query_scatter(_NoCalls(), o, d, surf, hits, rng), lambda: S.query_scatter(_NoCalls(), o, d, hits, surf, np.zeros((4, 4), np.uint32)),
           lambda: S.query_scatter(_NoCalls(), o, d, hits, surf, rng[::2]), lambda: S.query_scatter(_NoCalls(), o, d, hits, surf, rng, flags=rt.RT_QUERY_DEVICE_POINTERS),
           lambda: S.query_bsdf(_NoCalls(), o, d, hits, surf, np.ones((3, 3))), lambda: S.query_bsdf(_NoCalls(), o, d, hits, surf, np.ones((4, 2))),
           lambda: S.query_bsdf(_NoCalls(), o, d, hits[:2], surf, np.ones((4, 3))), lambda: S.query_bsdf(_NoCalls(), o, d, hits, surf, np.ones((4, 3)), flags=rt.RT_QUERY_DEVICE_POINTERS),
           lambda: S.trace_paths(_NoCalls(), o, d, rng[:3]), lambda: S.trace_paths(_NoCalls(), o, d[:, :2], rng),
           lambda: S.trace_paths(_NoCalls(), o, d, rng, flags=rt.RT_QUERY_DEVICE_POINTERS), lambda: rt.rng_uniform(np.zeros(4, np.uint32))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} reached C")


def test_the_model_folds_the_oracles_frame(rt):
    """Closest hits, surfaces, background, scatters (tests/scatter_model.py over the oracle's per-function answers) composed by
    model.frame: Hw8Oracle.render's 8x8 frame of soup_a at 2 samples, depth 6, every word; the engines end where the oracle's
    camera rays say the pixels' streams went."""
    w, h, samples, depth = 8, 8, 2, 6
    sd, oracle = sc.scene_data("soup_a"), sc.oracle("soup_a")
    cam_o, cam_d, lengths, any_miss, any_hit = model.traced_paths(oracle, w, h, samples, depth)
    assert any_miss and any_hit and len(np.unique(lengths)) >= 3
    calls = model.OracleCalls(sd, oracle)
    seen = []

    def camera_rays(s, xy):
        seen.append(xy)
        return cam_o[s], cam_d[s]
    got, _ = model.frame(calls, camera_rays, w, h, samples, depth)
    want, _, _ = oracle.render(w, h, samples, ray_depth=depth)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), sc.first_difference(got.reshape(-1, 3).view(np.uint32), want.reshape(-1, 3).view(np.uint32))
    assert np.array_equal(seen[0].view(np.uint32), sc.jitter(w, h).view(np.uint32))        # the two jitter draws are the renderer's
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 32

"""The baker (rt_bake_rays, rt_bake), the part that needs no GPU: the header declares it under ABI 6, the library exports it and the
package binds it; the three records have the sizes the C compiler sees; every refusal that is decided before the scene is looked at
arrives on a null scene with a message naming the field; the wrapper refuses mismatched shapes; and tests/bake_model.py is checked
against the oracle before it judges the GPU (tests/test_gpu_bake.py): its cosine direction and stream position are the oracle's,
its SH polynomials are the real ones to float32 rounding, and its loop over the oracle's calls folds what scatter_model.trace folds.
The same refusals run under the host sanitizers in tools/sanitize/query_sanitize.cpp, stand-alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bake_model as bm
import scatter_model as model
import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
F = np.float32

SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rtamd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_bake_point), sizeof(rt_bake_params), sizeof(rt_bake_stats),
           offsetof(rt_bake_point, n), offsetof(rt_bake_params, streams), offsetof(rt_bake_params, flags), offsetof(rt_bake_params, reserved),
           offsetof(rt_bake_stats, points), offsetof(rt_bake_stats, live_ray_slots), offsetof(rt_bake_stats, kernel_ms), offsetof(rt_bake_stats, launches));
    return 0;
}
"""


def test_header_declares_the_baker_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    for name, value in (("RT_BAKE_IRRADIANCE", "0"), ("RT_BAKE_SH9", "1"), ("RT_BAKE_LOCKSTEP", "4u")):
        assert re.search(r"^#define %s\s+%s\b" % (name, value), text, re.M), name
    for proto in (r"^int rt_bake_rays\(rt_scene \*\w*, const rt_bake_point \*\w+, rt_rng \*\w+[^,]*, size_t \w+, int32_t \w+, uint32_t \w+,\s+rt_ray \*\w+, rt_query_stats \*\w+",
                  r"^int rt_bake\(rt_scene \*\w*, const rt_bake_point \*\w+, size_t \w+, const rt_bake_params \*\w+,\s+rt_rng \*\w+ /\*[^/]*\*/, float \*\w+, rt_bake_stats \*\w+"):
        assert re.search(proto, text, re.M), proto


def test_library_exports_and_package_binds_them(rt):
    for fn in ("rt_bake_rays", "rt_bake"):
        assert fn in rt.ABI_SYMBOLS and hasattr(rt.lib, fn), fn
    assert rt.lib.rt_abi_version() == 6
    assert (rt.RT_BAKE_IRRADIANCE, rt.RT_BAKE_SH9, rt.RT_BAKE_LOCKSTEP) == (0, 1, 4)
    assert rt.RT_BAKE_LOCKSTEP & (rt.RT_QUERY_DEVICE_POINTERS | rt.RT_QUERY_REFERENCE_WALK) == 0
    for name in ("bake_rays", "bake"):
        assert callable(getattr(rt.Scene, name)) and callable(getattr(rt.Scene, name + "_device")), name
    assert (len(rt.lib.rt_bake_rays.argtypes), len(rt.lib.rt_bake.argtypes)) == (8, 7)
    assert rt.BAKE_POINT_DTYPE.itemsize == 24 and rt.BAKE_POINT_DTYPE.names == ("p", "n")


def test_struct_sizes_as_the_c_compiler_sees_them(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no C compiler to read include/rtamd.h with"
    src = tmp_path / "sizes.c"
    src.write_text(SIZES_C)
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-x", "c", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [24, 32, 88]
    P, S = rt.rt_bake_params, rt.rt_bake_stats
    assert got == [C.sizeof(rt.rt_bake_point), C.sizeof(P), C.sizeof(S), rt.rt_bake_point.n.offset, P.streams.offset, P.flags.offset, P.reserved.offset,
                   S.points.offset, S.live_ray_slots.offset, S.kernel_ms.offset, S.launches.offset]
    assert rt.BAKE_POINT_DTYPE.fields["n"][1] == rt.rt_bake_point.n.offset


class _Raw:
    """Raw calls on eight points of four streams and a null scene; nothing may be written."""

    def __init__(self, rt):
        self.rt = rt
        self.points = rt.pack_bake_points(np.zeros((8, 3), F), np.tile(np.array([0, 1, 0], F), (8, 1)))
        self.rng = model.seed(1 + 7919 * np.arange(32))
        self.before = self.rng.copy()
        self.rays = np.zeros(8, rt.RAY_DTYPE)
        self.out = np.zeros((8, 27), F)

    def _done(self, code):
        assert not self.rays.view(np.uint32).any() and not self.out.any() and np.array_equal(self.rng, self.before)
        return code, self.rt.lib.rt_last_error().decode()

    def rays_call(self, mode=0, flags=0, n=8, stats=None, drop=None):
        p = {k: (None if k == drop else v.ctypes.data) for k, v in (("points", self.points), ("rng", self.rng), ("out", self.rays))}
        return self._done(self.rt.lib.rt_bake_rays(None, p["points"], p["rng"], n, mode, flags, p["out"], C.byref(stats) if stats is not None else None))

    def bake_call(self, n=8, stats=None, drop=None, params="made", **fields):
        made = self.rt.make_bake_params(8, 4, self.rt.RT_BAKE_SH9, 4)
        for k, v in fields.items():
            if k == "reserved":
                made.reserved[v] = 1
            else:
                setattr(made, k, v)
        p = {k: (None if k == drop else v.ctypes.data) for k, v in (("points", self.points), ("rng", self.rng), ("out", self.out))}
        return self._done(self.rt.lib.rt_bake(None, p["points"], n, C.byref(made) if params == "made" else None, p["rng"], p["out"],
                                              C.byref(stats) if stats is not None else None))


def test_bake_rays_refusals_that_need_no_device(rt):
    raw, fn, bad = _Raw(rt), "rt_bake_rays: ", rt.RT_ERR_INVALID_ARG
    assert raw.rays_call() == (bad, fn + "null argument")                                        # everything in order but the scene
    for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
        st = rt.rt_query_stats()
        st.struct_size = size
        assert raw.rays_call(stats=st) == (bad, fn + "struct_size mismatch (ABI skew)")
    for mode in (2, -1, 27):
        assert raw.rays_call(mode=mode) == (bad, fn + f"mode = {mode} is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9")
    for flags in (2, 4, 8, 0x80000000, 1 | 4):
        assert raw.rays_call(flags=flags) == (bad, fn + "flags other than RT_QUERY_DEVICE_POINTERS"), flags
    for drop in ("points", "rng", "out"):
        assert raw.rays_call(drop=drop) == (bad, fn + "null argument"), drop
    for x in (0, 2**31 - 1, 2**32 - 1):
        for at in (0, 7):
            raw.rng["x"][at] = raw.before["x"][at] = x
            assert raw.rays_call() == (bad, fn + f"rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)")
            assert raw.rays_call(flags=rt.RT_QUERY_DEVICE_POINTERS) == (bad, fn + "null argument")     # a device array is not the host's to read
            raw.rng["x"][at] = raw.before["x"][at] = 1 + at
    raw.rng["x"][8] = raw.before["x"][8] = 0                                                     # beyond the n records: not the call's to judge
    assert raw.rays_call() == (bad, fn + "null argument")


def test_bake_refusals_that_need_no_device(rt):
    raw, fn, bad, limit = _Raw(rt), "rt_bake: ", rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    assert raw.bake_call() == (bad, fn + "null argument (scene)")                                # everything in order but the scene
    assert raw.bake_call(streams=0, ray_depth=0, mode=0, flags=1 | 2 | 4) == (bad, fn + "null argument (scene)")
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
    for flags in (8, 16, 0x80000000, 7 | 32):
        code, msg = raw.bake_call(flags=flags)
        assert code == bad and msg == fn + "params.flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK | RT_BAKE_LOCKSTEP", flags
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
    for drop in ("points", "rng", "out"):
        assert raw.bake_call(drop=drop) == (bad, fn + "null argument"), drop
    for x in (0, 2**31 - 1):
        for at in (0, 31):
            raw.rng["x"][at] = raw.before["x"][at] = x
            assert raw.bake_call() == (bad, fn + f"rng[{at}].x = {x} is no state of the engine (1 .. 2147483646)")
            assert raw.bake_call(flags=rt.RT_QUERY_DEVICE_POINTERS) == (bad, fn + "null argument (scene)")
            raw.rng["x"][at] = raw.before["x"][at] = 1 + at


class _NoCalls:
    """Stands in for a Scene whose handle must never be used: the wrapper has to refuse before it calls into C."""
    _h = None


def test_wrapper_refuses_mismatched_shapes_before_c(rt):
    points, rng = rt.pack_bake_points(np.zeros((4, 3)), np.ones((4, 3))), rt.rng_seed(np.arange(16))
    S = rt.Scene
    bad = [lambda: S.bake_rays(_NoCalls(), points, rng[:3]), lambda: S.bake_rays(_NoCalls(), np.zeros((4, 6), F), rng[:4]),
           lambda: S.bake_rays(_NoCalls(), points, rng[:8:2]), lambda: S.bake(_NoCalls(), points, rng[:4], 8, streams=4),
           lambda: S.bake(_NoCalls(), points, rng, 8, streams=2), lambda: S.bake(_NoCalls(), points, rng, 8, streams=4, mode=2),
           lambda: S.bake(_NoCalls(), points, rng, 8, streams=4, flags=rt.RT_QUERY_DEVICE_POINTERS), lambda: S.bake(_NoCalls(), rng, rng, 8, streams=1),
           lambda: rt.pack_bake_points(np.zeros((4, 3)), np.zeros((3, 3))), lambda: rt.pack_bake_points(np.zeros((4, 2)))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} reached C")
    assert rt.pack_bake_points(np.ones((5, 3))).shape == (5,) and not rt.pack_bake_points(np.ones((5, 3)))["n"].any()


def test_the_models_ray_maker_is_the_oracles(rt):
    """Fresh engines: the cosine direction is rto_hw8_cosine_sample_pdf's and the engine ends at its stream position; the uniform
    direction is normalize of rto_rng_kat's first three normals, and the cosine one is normalize(that + n) -- so the two modes agree
    on the draw.  A second call enters with the saved normal and leaves without one, one polar round further."""
    L = bm._lib()
    gen = np.random.default_rng(29)
    n = 64
    normals = gen.normal(0, 1, (n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    points = rt.pack_bake_points(gen.uniform(-2, 2, (n, 3)), normals)
    seeds = 1 + 7919 * np.arange(n)
    irr_rng, sh_rng = model.seed(seeds), model.seed(seeds)
    irr, bad_i = bm.expected_rays(points, irr_rng, bm.IRRADIANCE)
    sh, bad_s = bm.expected_rays(points, sh_rng, bm.SH9)
    assert bad_i == bad_s == 0 and np.array_equal(irr_rng, sh_rng) and irr_rng["has_saved"].all()
    assert np.array_equal(sh["o"], points["p"]) and np.array_equal(irr["o"], (points["p"] + model.EPS * points["n"]).astype(F))
    out = np.zeros(5, F)
    for i in range(n):
        L.rto_hw8_cosine_sample_pdf(int(seeds[i]), normals[i].ctypes.data, out.ctypes.data)
        assert np.array_equal(irr["d"][i].view(np.uint32), out[0:3].view(np.uint32))
        assert model.u01_of(model.next_state(irr_rng["x"][i])) == out[4]                      # the oracle's stream position
        assert np.array_equal(model._normals(int(seeds[i]), 4)[3:4].view(np.uint32), irr_rng["saved"][i:i + 1].view(np.uint32))
        u = sh["d"][i]
        with np.errstate(all="ignore"):
            d = u + normals[i]
            cos = ((F(1) / np.sqrt(bm.sm.dot(d, d))) * d).astype(F)
        assert np.array_equal(cos.view(np.uint32), irr["d"][i].view(np.uint32)) or bm.sm.dot(d, normals[i]) <= F(1e-9)
    assert np.abs(np.linalg.norm(sh["d"].astype(np.float64), axis=1) - 1).max() < 1e-6
    again = irr_rng.copy()
    second, _ = bm.expected_rays(points, again, bm.SH9)
    assert not again["has_saved"].any() and not again["saved"].any()
    for i in range(n):
        p, q = model._normals(int(irr_rng["x"][i]), 2)
        assert np.array_equal(second["d"][i].view(np.uint32), bm.sm.normalize(np.array([irr_rng["saved"][i], p, q], F)).view(np.uint32))
        assert again["x"][i] == model._polar_round(int(irr_rng["x"][i]))
    # an invalid record: the invalid ray, the engine as it was
    points["p"][5, 1] = np.nan
    points["n"][9] = 0
    one = model.seed(seeds)
    one["x"][11] = 0
    rays, invalid = bm.expected_rays(points, one, bm.IRRADIANCE)
    assert invalid == 3 and np.all(rays[[5, 9, 11]].view(np.uint32).reshape(3, 6) == bm.NO_RAY) and np.array_equal(one[[5, 9, 11]]["x"], [seeds[5], seeds[9], 0])
    _, invalid = bm.expected_rays(points, model.seed(seeds), bm.SH9)
    assert invalid == 1                                                                        # a zero n is valid where n is not read


def test_the_models_sh_basis_scales_and_sums():
    gen = np.random.default_rng(30)
    d = gen.normal(0, 1, (4096, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    Y = bm.sh_basis(d)
    x, y, z = (d[:, k].astype(np.float64) for k in range(3))
    real = np.stack([np.full(len(d), 0.5 * np.sqrt(1 / np.pi)), np.sqrt(3 / (4 * np.pi)) * y, np.sqrt(3 / (4 * np.pi)) * z, np.sqrt(3 / (4 * np.pi)) * x,
                     0.5 * np.sqrt(15 / np.pi) * x * y, 0.5 * np.sqrt(15 / np.pi) * y * z, 0.25 * np.sqrt(5 / np.pi) * (3 * z * z - 1),
                     0.5 * np.sqrt(15 / np.pi) * x * z, 0.25 * np.sqrt(15 / np.pi) * (x * x - y * y)], axis=1)
    assert Y.dtype == F and np.abs(Y - real).max() < 2e-6                                      # the header's six-digit constants
    gram = (4 * np.pi / len(d)) * Y.astype(np.float64).T @ Y.astype(np.float64)                # orthonormal over the sphere, to Monte Carlo error
    assert np.abs(gram - np.eye(9)).max() < 0.1
    assert bm.scale_of(bm.IRRADIANCE, 8) == F(np.pi / 8) and bm.scale_of(bm.SH9, 4096) == F(4 * np.pi / 4096)
    L = gen.uniform(0, 2, (6, 3)).astype(F)
    acc = bm.accumulate(bm.accumulate(np.zeros((6, 3), F), d[:6], L, bm.IRRADIANCE), d[:6], L, bm.IRRADIANCE)
    assert np.array_equal(acc, L + L)
    sh = bm.accumulate(np.zeros((6, 9, 3), F), d[:6], L, bm.SH9)
    assert np.array_equal(sh[:, 0, :], (F(0.282095) * L).astype(F)) and np.array_equal(sh[:, 3, 1], ((F(0.488603) * d[:6, 0]) * L[:, 1]).astype(F))
    out = bm.resolve(acc, np.array([True, False, True]), 2, bm.IRRADIANCE, 4)
    assert np.array_equal(out[0], bm.scale_of(0, 4) * (acc[0] + acc[1])) and not out[1].any() and out.shape == (3, 3)


def test_the_models_loop_folds_what_scatter_model_trace_folds(rt):
    """bake over the oracle's calls on soup_a, 8 points x 2 samples x depth 3: trace_counted's radiance is scatter_model.trace's, its
    counts are between 1 and the depth, and the loop's answer is the sums of those radiances."""
    sd, oracle = sc.scene_data("soup_a"), sc.oracle("soup_a")
    calls = model.OracleCalls(sd, oracle)
    o, d, hit = sc.traced_frame("soup_a", 8, 8)
    hits = calls.closest(o[hit][:8], d[hit][:8])
    p = (o[hit][:8] + hits["t"][:, None] * d[hit][:8]).astype(F)
    points = rt.pack_bake_points(p, hits["ng"])
    seen = []

    def tracer(ro, rd, rng):
        plain_rng = rng.copy()
        plain = model.trace(calls, ro, rd, plain_rng, 3)
        L, count = bm.trace_counted(calls, ro, rd, rng, 3)
        assert np.array_equal(L.view(np.uint32), plain.view(np.uint32)) and np.array_equal(rng, plain_rng)
        assert count.min() >= 1 and count.max() <= 3
        seen.append(L)
        return L, count
    rng = model.seed(1 + 7919 * np.arange(8))
    out, queries, valid = bm.bake(calls, points, rng, 2, 1, bm.IRRADIANCE, 3, tracer=tracer)
    assert valid.all() and queries.shape == (8, 2) and len(seen) == 2
    assert np.array_equal(out, (bm.scale_of(0, 2) * (seen[0] + seen[1])).astype(F)) and out.max() > 0
    assert not np.array_equal(rng, model.seed(1 + 7919 * np.arange(8)))

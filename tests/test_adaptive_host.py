"""Adaptive sampling, the part that needs no GPU: the header declares rt_adaptive_* under ABI 6 and the library exports them; the
decision (csrc/host/rt_adaptive_decide.h, through the test hook rtt_adaptive_decide) equals tests/adaptive_model.py on constructed tile
tables -- thresholds hit exactly, pixels == 0, batches == min_batches - 1, the cap, dilation at the grid's corners and edges; and every
entry point refuses null arguments and a wrong struct_size before it looks at a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def hooks(rt):
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_adaptive_decide.argtypes = [C.c_void_p, C.POINTER(rt.rt_adaptive_params), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return L


def test_header_declares_the_family_under_abi_6(rt):
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    declared = set(re.findall(r"^(?:int|void)\s+(rt_adaptive_[a-z_]+)\(", text, re.M))
    want = {"rt_adaptive_create", "rt_adaptive_render", "rt_adaptive_render_tiles", "rt_adaptive_tiles", "rt_adaptive_resolve",
            "rt_adaptive_noise", "rt_adaptive_sample_map", "rt_adaptive_destroy"}
    assert declared == want
    for name in want:
        assert name in rt.ABI_SYMBOLS and hasattr(rt.lib, name), name
    assert C.sizeof(rt.rt_adaptive_params) == 24 and rt.ADAPTIVE_TILE_DTYPE.itemsize == 32 and C.sizeof(rt.rt_adaptive_stats) == 80
    for word in ("checkpoints of an rt_adaptive", "rt_multi_*", "hw7 / hw6", "rt_accum_denoise on it"):
        assert word in text, word                                # what is out of scope is said


def _table(rt, rows, cols, **fields):
    t = np.zeros((rows, cols), dtype=rt.ADAPTIVE_TILE_DTYPE)
    t["samples"], t["batches"], t["pixels"] = 16, 4, 64
    t["sum_luminance"], t["sum_se2"] = F(64.0), F(64.0)            # mean luminance 1, tile noise 1
    for k, v in fields.items():
        t[k] = v
    return t


def _both(rt, hooks, tiles, target, min_batches=0, max_samples=0, flags=0, n_samples=4):
    p = rt.make_adaptive_params(target, min_batches, max_samples, flags)
    got = np.zeros(tiles.shape, dtype=np.uint32)
    tiles = np.ascontiguousarray(tiles)
    assert hooks.rtt_adaptive_decide(tiles.ctypes.data, C.byref(p), tiles.shape[1], tiles.shape[0], n_samples, got.ctypes.data) == 0
    want = am.decide(tiles, target, min_batches, max_samples, flags, n_samples)
    assert np.array_equal(got, want), (got, want)
    return got


def test_threshold_hit_exactly(rt, hooks):
    """sqrt(sum_se2 / pixels) == target * L converges, the next float above does not."""
    t = _table(rt, 2, 3)
    t["sum_se2"][0, 0] = F(16.0)                                   # noise 0.5
    t["sum_se2"][0, 1] = np.nextafter(F(16.0), F(32.0))            # just above it
    t["sum_se2"][1, 2] = F(4.0)                                    # 0.25: below
    got = _both(rt, hooks, t, 0.5)
    assert got[0, 0] == am.CONVERGED and got[0, 1] == am.ACTIVE and got[1, 2] == am.CONVERGED
    assert (got[np.array([[0, 0, 1], [1, 1, 0]], bool)] == am.ACTIVE).all()
    # the bound scales with the frame's mean luminance, which only the tiles with an estimate and a finite pixel make up
    t["sum_luminance"] = F(128.0)
    got = _both(rt, hooks, t, 0.25)
    assert got[0, 0] == am.CONVERGED and got[0, 1] == am.ACTIVE
    t["flags"][1, 0] = am.NO_ESTIMATE
    t["sum_luminance"][1, 0] = F(1e9)                              # not part of L
    assert _both(rt, hooks, t, 0.25)[0, 0] == am.CONVERGED | 0


def test_converged_is_sticky_and_no_estimate_is_not_judged(rt, hooks):
    t = _table(rt, 1, 4)
    t["flags"][0, 0] = am.CONVERGED | am.ACTIVE                    # noise 1 against a target of 0.5: it would not converge today
    t["flags"][0, 1] = am.NO_ESTIMATE | am.ACTIVE
    t["pixels"][0, 1], t["sum_se2"][0, 1] = 0, 0                   # an entry without an estimate: its zeros mean nothing
    t["batches"][0, 1] = 1
    got = _both(rt, hooks, t, 0.5)
    assert got[0, 0] == am.CONVERGED
    assert got[0, 1] == am.NO_ESTIMATE | am.ACTIVE
    assert got[0, 2] == am.ACTIVE and got[0, 3] == am.ACTIVE


def test_no_finite_pixel_converges_at_once(rt, hooks):
    t = _table(rt, 2, 2, batches=2)                                # below min_batches = 4: nothing else is judged
    t["pixels"][1, 1], t["nonfinite"][1, 1], t["sum_se2"][1, 1], t["sum_luminance"][1, 1] = 0, 64, 0, 0
    got = _both(rt, hooks, t, 100.0)
    assert got[1, 1] == am.CONVERGED and (got.reshape(-1)[:3] == am.ACTIVE).all()
    everything = _table(rt, 2, 2, pixels=0, sum_se2=0, sum_luminance=0)
    assert (_both(rt, hooks, everything, 0.5) == am.CONVERGED).all()  # L = 0 and nothing divides by it


def test_one_batch_short_of_min_batches(rt, hooks):
    for min_batches, default in ((0, 4), (2, 2), (7, 7)):
        t = _table(rt, 1, 3, sum_se2=F(0.0))                       # as quiet as can be
        t["batches"][0] = [default - 1, default, default + 1]
        got = _both(rt, hooks, t, 0.5, min_batches=min_batches)
        assert list(got[0]) == [am.ACTIVE, am.CONVERGED, am.CONVERGED], min_batches


def test_the_cap(rt, hooks):
    t = _table(rt, 1, 4)
    t["samples"][0] = [24, 28, 29, 32]
    got = _both(rt, hooks, t, 0.5, max_samples=32, n_samples=4)
    assert list(got[0]) == [am.ACTIVE, am.ACTIVE, am.CAPPED, am.CAPPED]   # 28 + 4 = 32 does not pass it, 29 + 4 does
    got = _both(rt, hooks, t, 0.5, max_samples=32, n_samples=8)
    assert list(got[0]) == [am.ACTIVE, am.CAPPED, am.CAPPED, am.CAPPED]
    t["samples"][0] = [0, (1 << 25) - 5, (1 << 25) - 4, 5]
    got = _both(rt, hooks, t, 0.5, n_samples=4)                    # max_samples = 0: the sample-index limit
    assert list(got[0]) == [am.ACTIVE, am.ACTIVE, am.CAPPED, am.ACTIVE]
    t["sum_se2"] = F(0.0)
    got = _both(rt, hooks, t, 0.5, n_samples=4)
    assert got[0, 2] == am.CONVERGED | am.CAPPED


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 5), (5, 1), (4, 6)])
def test_dilation_at_corners_and_edges(rt, hooks, rows, cols):
    """One noisy sub-tile at every place of the grid in turn, everything else quiet: with RT_ADAPTIVE_DILATE its 8-neighbours inside the
    grid stay active, nothing else; a capped neighbour keeps nobody active, and a capped sub-tile is never active."""
    for hy in range(rows):
        for hx in range(cols):
            t = _table(rt, rows, cols, sum_se2=F(0.0))
            t["sum_se2"][hy, hx] = F(64.0)
            plain = _both(rt, hooks, t, 0.5)
            assert plain[hy, hx] == am.ACTIVE and (plain == am.ACTIVE).sum() == 1
            got = _both(rt, hooks, t, 0.5, flags=am.DILATE)
            for y in range(rows):
                for x in range(cols):
                    near = max(abs(y - hy), abs(x - hx)) <= 1
                    want = am.ACTIVE if (y, x) == (hy, hx) else am.CONVERGED | (am.ACTIVE if near else 0)
                    assert got[y, x] == want, (hy, hx, y, x)
            t["samples"][hy, hx] = 100                             # the noisy one is capped: no neighbour has a reason left
            got = _both(rt, hooks, t, 0.5, max_samples=64, flags=am.DILATE)
            assert got[hy, hx] == am.CAPPED and ((got & am.ACTIVE) == 0).all()
    rng = np.random.default_rng(rows * 16 + cols)                  # and random tables against the model
    for _ in range(20):
        t = _table(rt, rows, cols)
        t["sum_se2"] = rng.choice([0.0, 16.0, 64.0], size=(rows, cols)).astype(F)
        t["batches"] = rng.integers(1, 7, size=(rows, cols))
        t["samples"] = rng.integers(0, 40, size=(rows, cols))
        t["pixels"] = rng.choice([0, 7, 64], size=(rows, cols))
        t["flags"] = rng.choice([0, am.CONVERGED, am.NO_ESTIMATE, am.ACTIVE], size=(rows, cols))
        _both(rt, hooks, t, 0.5, max_samples=32, flags=am.DILATE)
        _both(rt, hooks, t, 0.5, min_batches=2)


def test_the_hook_refuses_nulls(rt, hooks):
    p = rt.make_adaptive_params(0.5)
    t = _table(rt, 1, 1)
    out = np.zeros(1, np.uint32)
    assert hooks.rtt_adaptive_decide(None, C.byref(p), 1, 1, 4, out.ctypes.data) == rt.RT_ERR_INVALID_ARG
    assert hooks.rtt_adaptive_decide(t.ctypes.data, None, 1, 1, 4, out.ctypes.data) == rt.RT_ERR_INVALID_ARG
    assert hooks.rtt_adaptive_decide(t.ctypes.data, C.byref(p), 0, 1, 4, out.ctypes.data) == rt.RT_ERR_INVALID_ARG


def test_null_arguments_and_struct_sizes(rt):
    bad = rt.RT_ERR_INVALID_ARG
    err = lambda: rt.lib.rt_last_error().decode()
    p, ap, out = rt.make_params(8, 8, 0), rt.make_adaptive_params(0.1), C.c_void_p(0x5a5a)
    buf = np.zeros(64, np.uint8)
    for scene, pp, aa, oo in ((None, C.byref(p), C.byref(ap), C.byref(out)), (None, None, C.byref(ap), C.byref(out)),
                              (None, C.byref(p), None, C.byref(out)), (None, C.byref(p), C.byref(ap), None)):
        assert rt.lib.rt_adaptive_create(scene, pp, aa, oo) == bad and err() == "rt_adaptive_create: null argument"
    assert out.value == 0x5a5a                                     # a refusal for a null argument writes nothing
    st = rt.rt_adaptive_stats()
    st.struct_size = C.sizeof(st)
    assert rt.lib.rt_adaptive_render(None, 4, C.byref(st)) == bad and err() == "rt_adaptive_render: null argument"
    assert rt.lib.rt_adaptive_render(None, 4, None) == bad
    assert rt.lib.rt_adaptive_render_tiles(None, 4, buf.ctypes.data, None) == bad and err() == "rt_adaptive_render_tiles: null argument"
    for size in (0, C.sizeof(st) - 8, C.sizeof(rt.rt_stats)):
        st.struct_size = size
        assert rt.lib.rt_adaptive_render(None, 4, C.byref(st)) == bad and err() == "rt_adaptive_render: stats.struct_size mismatch (ABI skew)"
        assert rt.lib.rt_adaptive_render_tiles(None, 4, buf.ctypes.data, C.byref(st)) == bad
        assert err() == "rt_adaptive_render_tiles: stats.struct_size mismatch (ABI skew)"
    assert rt.lib.rt_adaptive_tiles(None, buf.ctypes.data) == bad and err() == "rt_adaptive_tiles: null argument"
    assert rt.lib.rt_adaptive_resolve(None, 0, None, None) == bad and err() == "rt_adaptive_resolve: null argument"
    assert rt.lib.rt_adaptive_sample_map(None, buf.ctypes.data) == bad and err() == "rt_adaptive_sample_map: null argument"
    s = rt.rt_noise_summary()
    s.struct_size = C.sizeof(s)
    assert rt.lib.rt_adaptive_noise(None, 0, None, C.byref(s)) == bad and err() == "rt_adaptive_noise: null argument"
    s.struct_size = 8
    assert rt.lib.rt_adaptive_noise(None, 0, None, C.byref(s)) == bad and err() == "rt_adaptive_noise: struct_size mismatch (ABI skew)"
    rt.lib.rt_adaptive_destroy(None)                               # like free(NULL)

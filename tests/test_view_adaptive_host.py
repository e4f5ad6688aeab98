"""Adaptive view sets, the part that needs no GPU: the header declares rt_view_adaptive_* under ABI 6 with the binding's struct size and
the library exports them; the planning step of a slice (csrc/host/rt_view_adaptive_plan.h, through the test hook rtt_view_adaptive_plan)
equals a numpy restatement built on tests/adaptive_model.py -- the decision per view, the ascending list of words view * tiles +
sub-tile, the monitor's numbers per (view, sub-tile) -- on hand-made tables of 3 views x (3 x 2) sub-tiles: every flag combination, a
masked-out view, the cap at this call's n_samples, dilation that stays inside a view, an all-frozen set; and every entry point refuses
null arguments and a wrong struct_size before it looks at a scene or a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
WANT = {"rt_view_adaptive_create", "rt_view_adaptive_set_cameras", "rt_view_adaptive_render", "rt_view_adaptive_render_tiles",
        "rt_view_adaptive_tiles", "rt_view_adaptive_resolve", "rt_view_adaptive_noise", "rt_view_adaptive_sample_map", "rt_view_adaptive_destroy"}
VIEWS, ROWS, COLS = 3, 2, 3
ARGS_DTYPE = np.dtype([("n", F), ("N", F), ("N1", F), ("first", np.uint32), ("dof", F), ("d", F)])   # AdTileArgs, device/rt_types_adaptive.h


@pytest.fixture(scope="module")
def hooks(rt):
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_view_adaptive_plan.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt.rt_adaptive_params), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    return L


def test_header_declares_the_family_under_abi_6(rt):
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    assert set(re.findall(r"^(?:int|void)\s+(rt_view_adaptive_[a-z_]+)\(", text, re.M)) == WANT and len(WANT) == 9
    for name in WANT:
        assert name in rt.ABI_SYMBOLS and hasattr(rt.lib, name), name
    section = re.sub(r"\s*\n \*\s+", " ", text[text.index("adaptive view sets: freeze converged 8x8 sub-tiles per camera"):])   # the comment's lines joined
    for words in ("checkpoints of an adaptive view set", "rt_multi_*", "hw7 and hw6", "rt_denoise and guide images for a view's camera", "views of different sizes"):
        assert words in section, words                           # what is out of scope is said
    assert "rt_view_adaptive_* below" in text                    # and the view sets' paragraph says where adaptive sampling per view lives


def test_stats_size_equals_the_headers(rt):
    """The header's layout, worked out by hand (the .hip has the same static_assert): 6*4 + 8 + 2*4 + 5*8 + 2*4 + 8; and field by field
    against the header's text."""
    S = rt.rt_view_adaptive_stats
    assert C.sizeof(S) == 96
    source = open(os.path.join(ROOT, "raytracing-course-hw_amd", "csrc", "rtamd_view_adaptive.hip")).read()
    assert "static_assert(sizeof(rt_view_adaptive_stats) == 96" in source
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    body = re.search(r"typedef struct rt_view_adaptive_stats \{(.*?)\} rt_view_adaptive_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in S._fields_], names
    assert S.samples.offset == 24 and S.kernel_ms.offset == 40 and S.total_ms.offset == 72 and S.exact_walks.offset == 88


def _tables(rt, **fields):
    """VIEWS tables of ROWS x COLS entries: 16 samples in 4 batches, mean luminance 1, tile noise 1, nothing decided yet."""
    t = np.zeros((VIEWS, ROWS, COLS), dtype=rt.ADAPTIVE_TILE_DTYPE)
    t["samples"], t["batches"], t["pixels"] = 16, 4, 64
    t["sum_luminance"], t["sum_se2"] = F(64.0), F(64.0)
    for k, v in fields.items():
        t[k] = v
    return t


def _model(tiles, observed, target, min_batches, max_samples, flags, n_samples, view_mask, tile_mask):
    """The plan restated: adaptive_model.decide per view that takes part, the ascending words, the numbers per word."""
    per_view = ROWS * COLS
    if tile_mask is not None:
        new = tiles["flags"].copy()
        drawn = np.asarray(tile_mask).reshape(-1) != 0
    else:
        new = np.stack([am.decide(tiles[v], target, min_batches, max_samples, flags, n_samples) if view_mask is None or view_mask[v] else tiles["flags"][v]
                        for v in range(VIEWS)])
        part = np.repeat(np.ones(VIEWS, bool) if view_mask is None else np.asarray(view_mask) != 0, per_view)
        drawn = ((new.reshape(-1) & am.ACTIVE) != 0) & part
    words = np.flatnonzero(drawn).astype(np.uint32)
    flat, N = tiles.reshape(-1), observed.reshape(-1).astype(np.int64)
    args = np.zeros(VIEWS * per_view, ARGS_DTYPE)
    args["n"], args["N"], args["N1"], args["first"] = F(n_samples), N.astype(F), (N + n_samples).astype(F), N == 0
    args["dof"] = (flat["batches"].astype(np.int64) + drawn - 1).astype(F)
    args["d"] = (flat["samples"].astype(np.int64) + n_samples * drawn).astype(F)
    return new.astype(np.uint32), words, args


def _both(rt, hooks, tiles, observed=None, target=0.5, min_batches=0, max_samples=0, flags=0, n_samples=4, view_mask=None, tile_mask=None):
    tiles = np.ascontiguousarray(tiles)
    observed = np.ascontiguousarray(tiles["samples"] if observed is None else observed, dtype=np.int32)
    p = rt.make_adaptive_params(target, min_batches, max_samples, flags)
    n = tiles.size
    got_flags, got_list, got_n, got_args = np.zeros(tiles.shape, np.uint32), np.full(n, 0xdeadbeef, np.uint32), C.c_uint32(77), np.zeros(n, ARGS_DTYPE)
    vm = None if view_mask is None else np.ascontiguousarray(view_mask, dtype=np.uint8)
    tm = None if tile_mask is None else np.ascontiguousarray(np.asarray(tile_mask, dtype=np.uint8).reshape(-1))
    assert hooks.rtt_view_adaptive_plan(tiles.ctypes.data, observed.ctypes.data, C.byref(p), COLS, ROWS, VIEWS, n_samples,
                                        None if vm is None else vm.ctypes.data, None if tm is None else tm.ctypes.data,
                                        got_flags.ctypes.data, got_list.ctypes.data, C.byref(got_n), got_args.ctypes.data) == 0
    want_flags, want_list, want_args = _model(tiles, observed, target, min_batches, max_samples, flags, n_samples, view_mask, tile_mask)
    assert np.array_equal(got_flags, want_flags), (got_flags, want_flags)
    words = got_list[:got_n.value]
    assert np.array_equal(words, want_list) and (got_list[got_n.value:] == 0xdeadbeef).all(), (words, want_list)
    assert (np.diff(words.astype(np.int64)) > 0).all()             # ascending, no word twice
    assert got_args.tobytes() == want_args.tobytes(), (got_args, want_args)
    return got_flags, words, got_args


def test_every_flag_combination(rt, hooks):
    """Stored flags 0 .. 15 over the 18 entries, twice shifted, plain and dilated, every view and with the middle one masked out."""
    for shift in (0, 5):
        t = _tables(rt)
        t["flags"] = ((np.arange(VIEWS * ROWS * COLS) + shift) % 16).reshape(VIEWS, ROWS, COLS)
        t["sum_se2"][:, 0, :] = F(4.0)                             # a quiet first row: converges wherever an estimate is there to judge
        for flags in (0, am.DILATE):
            for view_mask in (None, [1, 0, 1]):
                got, words, _ = _both(rt, hooks, t, flags=flags, view_mask=view_mask)
                if view_mask:
                    assert np.array_equal(got[1], t["flags"][1]) and not ((words >= 6) & (words < 12)).any()
        _both(rt, hooks, t, tile_mask=(np.arange(18) % 3 == 1))    # the mechanism: the stored flags, the mask's words


def test_each_view_is_judged_by_its_own_luminance(rt, hooks):
    """Tile noise 0.5 everywhere; mean luminance 1, 2 and 0.5 per view: a target of 0.4 converges the middle view only."""
    t = _tables(rt, sum_se2=F(16.0))
    t["sum_luminance"][1], t["sum_luminance"][2] = F(128.0), F(32.0)
    got, words, _ = _both(rt, hooks, t, target=0.4)
    assert (got[0] == am.ACTIVE).all() and (got[1] == am.CONVERGED).all() and (got[2] == am.ACTIVE).all()
    assert list(words) == list(range(0, 6)) + list(range(12, 18))


def test_a_masked_out_view_keeps_its_flags_and_draws_nothing(rt, hooks):
    t = _tables(rt)
    t["flags"][1] = am.ACTIVE | am.CAPPED | am.NO_ESTIMATE         # no decision would leave this
    got, words, args = _both(rt, hooks, t, view_mask=[1, 0, 1])
    assert (got[1] == (am.ACTIVE | am.CAPPED | am.NO_ESTIMATE)).all()
    assert list(words) == list(range(0, 6)) + list(range(12, 18))
    a = args.reshape(VIEWS, ROWS, COLS)
    assert (a["d"][1] == 16).all() and (a["dof"][1] == 3).all()    # nothing added to the view that sits out
    assert (a["d"][0] == 20).all() and (a["dof"][2] == 4).all()
    got, words, _ = _both(rt, hooks, t, view_mask=[0, 0, 0])
    assert len(words) == 0 and np.array_equal(got, t["flags"])


def test_the_cap_is_this_calls(rt, hooks):
    t = _tables(rt)
    t["samples"][0, 0] = [24, 28, 29]
    t["samples"][2, 1] = [28, 25, 32]
    got, words, _ = _both(rt, hooks, t, max_samples=32, n_samples=4)
    assert list(got[0, 0]) == [am.ACTIVE, am.ACTIVE, am.CAPPED] and list(got[2, 1]) == [am.ACTIVE, am.ACTIVE, am.CAPPED]
    assert 2 not in words and 17 not in words and len(words) == 16
    got, words, _ = _both(rt, hooks, t, max_samples=32, n_samples=8)
    assert list(got[0, 0]) == [am.ACTIVE, am.CAPPED, am.CAPPED] and list(got[2, 1]) == [am.CAPPED, am.CAPPED, am.CAPPED]
    assert len(words) == 13


def test_dilation_stays_inside_a_view(rt, hooks):
    """View 0 and view 2 quiet, the whole first row of view 1 noisy: under RT_ADAPTIVE_DILATE the second row of view 1 goes on drawing;
    the last sub-tiles of view 0, next to them in memory and below them if the views were stacked, do not, nor do the first of view 2."""
    t = _tables(rt, sum_se2=F(0.0))
    t["sum_se2"][1, 0, :] = F(64.0)
    plain, words, _ = _both(rt, hooks, t)
    assert list(words) == [6, 7, 8]
    got, words, _ = _both(rt, hooks, t, flags=am.DILATE)
    assert (got[0] == am.CONVERGED).all() and (got[2] == am.CONVERGED).all()
    assert (got[1, 0] == am.ACTIVE).all() and (got[1, 1] == am.CONVERGED | am.ACTIVE).all()
    assert list(words) == [6, 7, 8, 9, 10, 11]
    t = _tables(rt, sum_se2=F(0.0))
    t["sum_se2"][1, 0, 0] = F(64.0)                                 # view 1's first sub-tile alone: view 0's last is its neighbour in memory only
    got, words, _ = _both(rt, hooks, t, flags=am.DILATE)
    assert got[0, 1, 2] == am.CONVERGED and list(words) == [6, 7, 9, 10]


def test_an_all_frozen_set_gives_an_empty_list(rt, hooks):
    t = _tables(rt, sum_se2=F(0.0))
    t["samples"][2] = 100
    got, words, args = _both(rt, hooks, t, max_samples=64, flags=am.DILATE)
    assert len(words) == 0 and ((got & am.ACTIVE) == 0).all() and (got[2] == am.CONVERGED | am.CAPPED).all()
    assert np.array_equal(args["d"].reshape(t.shape), t["samples"].astype(F))       # and nobody's numbers move
    _both(rt, hooks, t, tile_mask=np.zeros(18, np.uint8))


def test_the_monitors_numbers(rt, hooks):
    """A fresh sub-tile (N = 0) is `first`; observed samples need not be the samples; a drawn sub-tile has one batch and n samples more."""
    t = _tables(rt)
    t["samples"][0, 0, 0], t["batches"][0, 0, 0], t["flags"][0, 0, 0] = 0, 0, am.ACTIVE | am.NO_ESTIMATE
    observed = t["samples"].copy()
    observed[1] = 12
    mask = np.zeros((VIEWS, ROWS, COLS), np.uint8)
    mask[0, 0, 0] = mask[1, 1, 2] = mask[2, 0, 1] = 1
    _, words, args = _both(rt, hooks, t, observed=observed, n_samples=3, tile_mask=mask)
    assert list(words) == [0, 11, 13]
    a = args.reshape(VIEWS, ROWS, COLS)
    assert tuple(a[0, 0, 0]) == (3.0, 0.0, 3.0, 1, 0.0, 3.0)
    assert tuple(a[1, 1, 2]) == (3.0, 12.0, 15.0, 0, 4.0, 19.0)
    assert tuple(a[1, 0, 0]) == (3.0, 12.0, 15.0, 0, 3.0, 16.0)     # not drawn


def test_the_hook_refuses_nulls(rt, hooks):
    t = _tables(rt)
    obs = np.zeros(18, np.int32)
    p = rt.make_adaptive_params(0.5)
    out, n = np.zeros(18 * 6, np.uint32), C.c_uint32()
    ok = [t.ctypes.data, obs.ctypes.data, C.byref(p), COLS, ROWS, VIEWS, 4, None, None, out.ctypes.data, out.ctypes.data, C.byref(n), out.ctypes.data]
    assert hooks.rtt_view_adaptive_plan(*ok) == 0
    for k, v in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, 0), (9, None), (10, None), (11, None), (12, None)):
        args = list(ok)
        args[k] = v
        assert hooks.rtt_view_adaptive_plan(*args) == rt.RT_ERR_INVALID_ARG, k


def test_null_arguments_and_struct_sizes(rt):
    bad = rt.RT_ERR_INVALID_ARG
    err = lambda: rt.lib.rt_last_error().decode()
    cams = C.cast((rt.rt_camera * 2)(), C.c_void_p)
    p, ap, out = rt.make_views_params(8, 8, 2), rt.make_adaptive_params(0.1), C.c_void_p(0x5a5a)
    fake = C.c_void_p(0x1000)                                      # never looked at: the refusal comes first
    for scene, pp, aa, cc, oo in ((None, C.byref(p), C.byref(ap), cams, C.byref(out)), (fake, None, C.byref(ap), cams, C.byref(out)),
                                  (fake, C.byref(p), None, cams, C.byref(out)), (fake, C.byref(p), C.byref(ap), None, C.byref(out)),
                                  (fake, C.byref(p), C.byref(ap), cams, None)):
        assert rt.lib.rt_view_adaptive_create(scene, pp, aa, cc, oo) == bad and err() == "rt_view_adaptive_create: null argument"
    for size in (0, 36, C.sizeof(rt.rt_render_params)):
        p.struct_size = size
        assert rt.lib.rt_view_adaptive_create(fake, C.byref(p), C.byref(ap), cams, C.byref(out)) == bad
        assert err() == "rt_view_adaptive_create: params.struct_size mismatch (ABI skew)"
    p.struct_size = C.sizeof(p)
    for size in (0, 20, C.sizeof(p)):
        ap.struct_size = size
        assert rt.lib.rt_view_adaptive_create(fake, C.byref(p), C.byref(ap), cams, C.byref(out)) == bad
        assert err() == "rt_view_adaptive_create: adaptive.struct_size mismatch (ABI skew)"
    assert out.value == 0x5a5a                                     # a refusal for a null argument writes nothing
    st = rt.rt_view_adaptive_stats()
    st.struct_size = C.sizeof(st)
    buf = np.zeros(64, np.uint8)
    for fn, who in ((rt.lib.rt_view_adaptive_render, "rt_view_adaptive_render"), (rt.lib.rt_view_adaptive_render_tiles, "rt_view_adaptive_render_tiles")):
        st.struct_size = C.sizeof(st)
        assert fn(None, 4, buf.ctypes.data, C.byref(st)) == bad and err() == who + ": null argument"
        assert fn(fake, 4, buf.ctypes.data, None) == bad and err() == who + ": null argument"
        for size in (0, C.sizeof(st) - 8, C.sizeof(rt.rt_views_stats), C.sizeof(rt.rt_adaptive_stats)):
            st.struct_size = size
            assert fn(fake, 4, buf.ctypes.data, C.byref(st)) == bad and err() == who + ": stats.struct_size mismatch (ABI skew)"
    assert rt.lib.rt_view_adaptive_set_cameras(None, 0, 1, cams) == bad and err() == "rt_view_adaptive_set_cameras: null argument"
    assert rt.lib.rt_view_adaptive_set_cameras(fake, 0, 1, None) == bad and err() == "rt_view_adaptive_set_cameras: null argument"
    assert rt.lib.rt_view_adaptive_tiles(None, 0, buf.ctypes.data) == bad and err() == "rt_view_adaptive_tiles: null argument"
    assert rt.lib.rt_view_adaptive_tiles(fake, 0, None) == bad and err() == "rt_view_adaptive_tiles: null argument"
    assert rt.lib.rt_view_adaptive_resolve(None, 0, 0, None, None) == bad and err() == "rt_view_adaptive_resolve: null argument"
    assert rt.lib.rt_view_adaptive_sample_map(None, 0, buf.ctypes.data) == bad and err() == "rt_view_adaptive_sample_map: null argument"
    assert rt.lib.rt_view_adaptive_sample_map(fake, 0, None) == bad and err() == "rt_view_adaptive_sample_map: null argument"
    s = rt.rt_noise_summary()
    s.struct_size = C.sizeof(s)
    assert rt.lib.rt_view_adaptive_noise(None, 0, 0, None, C.byref(s)) == bad and err() == "rt_view_adaptive_noise: null argument"
    s.struct_size = 8
    assert rt.lib.rt_view_adaptive_noise(fake, 0, 0, None, C.byref(s)) == bad and err() == "rt_view_adaptive_noise: struct_size mismatch (ABI skew)"
    rt.lib.rt_view_adaptive_destroy(None)                          # like free(NULL)

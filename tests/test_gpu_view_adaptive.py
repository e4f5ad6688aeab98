"""Adaptive view sets on the GPU (include/rtamd.h: rt_view_adaptive_*): view v of a set driven by the policy equals, after every slice and
bit for bit -- tile entries, picture, sample map, noise map and summary -- an rt_adaptive with the same parameters on a scene created with
camera = cameras[v], for the six cameras of tests/view_cases.py, plain and with RT_ADAPTIVE_DILATE, whatever the other views drew; the
mechanism with hand-made masks gives rt_render's pixels per distinct count and the uniform run's statistics per batch count; with every
sub-tile active a view is rt_views' view; view masks, set_cameras, the launch count, chunk seams, the surroundings untouched, and every
refusal with its status and cause.  Scenes soup_a and sphere_emissive_env, depth 4, slices of 4; frames 8x8 (one sub-tile), 40x24 (15
whole sub-tiles) and 43x21 (6 x 3 with padded right and bottom borders).  The referees are computed once and kept read-only."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as am
import pin_cases
import surface_cases as sc
import view_cases as vc

pytestmark = pytest.mark.gpu

SLICE, DEPTH = vc.SLICE, vc.DEPTH
SCENES = ["soup_a", "sphere_emissive_env"]
GRIDS = [(40, 24), (43, 21)]                       # more than one sub-tile
MASKS = ([0, 0, 1, 0, 0], [1, 0, 1, 0, 1], [0, 1, 1, 1, 1])         # tests/test_gpu_views.py::MASKS: one alone, alternating, all but the first
SUMMARY = ("batches", "samples_observed", "samples_total", "pixels", "nonfinite_pixels", "mean_luminance", "rms_error", "noise", "worst_tile_noise")
_RENDER, _UNIFORM, _TARGET = {}, {}, {}


@pytest.fixture(scope="module")
def scenes(rt):
    """scenes(name): the scene as it is; scenes(name, camera name): the scene created with that camera of the table."""
    made = {}

    def get(name, cam=None):
        if (name, cam) not in made:
            sd = sc.scene_data(name)
            made[(name, cam)] = rt.Scene(sd if cam is None else vc.swapped(sd, vc.table(sd)[cam]))
        return made[(name, cam)]
    yield get
    for s in made.values():
        s.close()


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _cams(name, names):
    t = vc.table(sc.scene_data(name))
    return [t[n] for n in names]


def _render(scenes, name, cam, w, h, d):
    """rt_render(samples = d) on the scene created with camera `cam`: the referee of every sub-tile of that view that has drawn d."""
    key = (name, cam, w, h, d)
    if key not in _RENDER:
        rgb, rgb8, st = scenes(name, cam).render(w, h, d, ray_depth=DEPTH)
        assert st.reference_exact == 1
        _RENDER[key] = _ro(rgb, rgb8)
    return _RENDER[key]


def _state(obj, *view):
    """Everything an rt_adaptive (no argument) or view `view` of a set says: raw words, the noise only once a sub-tile has 2 batches."""
    tiles = obj.tiles(*view)
    rgb, rgb8 = obj.resolve(*view)
    out = dict(tiles=tiles.tobytes(), rgb=rgb.view(np.uint32), rgb8=rgb8, spp=obj.sample_map(*view))
    if tiles["batches"].max() >= 2:
        se, s = obj.noise(*view)
        out["se"], out["summary"] = se.view(np.uint32), tuple(getattr(s, f) for f in SUMMARY)
    return out


def _same(got, want):
    return got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) if isinstance(got[k], np.ndarray) else got[k] == want[k] for k in got)


def _differing(got, want):
    return [k for k in set(got) | set(want) if k not in got or k not in want or not (np.array_equal(got[k], want[k]) if isinstance(got[k], np.ndarray) else got[k] == want[k])]


def _per_pixel(tile_values, w, h):
    return np.repeat(np.repeat(tile_values, 8, axis=0), 8, axis=1)[:h, :w]


def _uniform(scenes, name, cam, w, h, k=3):
    """An rt_adaptive on the scene created with `cam`, every sub-tile drawn in each of k slices: per j = 1 .. k its tile table and, from
    j = 2 on, its noise map."""
    key = (name, cam, w, h)
    if key not in _UNIFORM:
        a = scenes(name, cam).adaptive(w, h, 1.0, ray_depth=DEPTH)
        ones, have = np.ones(a.grid, np.uint8), {}
        for j in range(1, k + 1):
            a.render_tiles(SLICE, ones)
            have[j] = (_ro(a.tiles())[0], _ro(a.noise()[0])[0] if j >= 2 else None)
        a.close()
        _UNIFORM[key] = have
    return _UNIFORM[key]


def _target(scenes, name, w, h):
    """The median over all views' sub-tiles of (sub-tile noise / that view's mean luminance) after three uniform slices of the referees:
    tests/test_gpu_adaptive.py::test_policy's recipe, pooled over the views."""
    if (name, w, h) not in _TARGET:
        ratios = []
        for cam in vc.NAMES:
            tiles = _uniform(scenes, name, cam, w, h)[3][0]
            L = am.mean_luminance(tiles)
            assert L > 0, cam
            ratios.append(np.nan_to_num(am.tile_noise(tiles)).reshape(-1) / L)
        _TARGET[(name, w, h)] = float(np.float32(np.median(np.concatenate(ratios))))
    return _TARGET[(name, w, h)]


@pytest.mark.parametrize("dilate", [False, True])
@pytest.mark.parametrize("w,h", GRIDS)
def test_policy_equals_stand_alone_referees(rt, scenes, w, h, dilate):
    name, min_batches, max_samples = "sphere_emissive_env", 3, 20      # lit by its environment: every sub-tile has noise of its own
    target = _target(scenes, name, w, h)
    print("target", target)
    assert target > 0
    kw = dict(min_batches=min_batches, max_samples=max_samples, dilate=dilate, ray_depth=DEPTH)
    refs = [scenes(name, cam).adaptive(w, h, target, **kw) for cam in vc.NAMES]
    # the referees alone, before the object is trusted: a mixed strip is really exercised
    history = []
    for _ in range(max_samples // SLICE + 2):
        stats = [r.render(SLICE) for r in refs]
        if sum(st.samples for st in stats) == 0:
            break
        history.append(([_state(r) for r in refs], stats))
    else:
        raise AssertionError("the referees did not end")
    n = len(refs) * refs[0].grid[0] * refs[0].grid[1]
    first = np.concatenate([np.frombuffer(s["tiles"], rt.ADAPTIVE_TILE_DTYPE)["flags"] for s in history[min_batches - 1][0]])   # the first decision that judges anything
    print("first judging decision: converged", ((first & am.CONVERGED) != 0).sum(), "active", ((first & am.ACTIVE) != 0).sum(), "of", n)
    assert ((first & am.CONVERGED) != 0).sum() * 4 >= n and ((first & am.ACTIVE) != 0).sum() * 4 >= n
    final = [s["spp"] for s in history[-1][0]]
    assert any(not np.array_equal(final[0], f) for f in final[1:])    # at least two views differ in their final sample maps
    # the set, slice by slice
    views = scenes(name).adaptive_views(w, h, _cams(name, vc.NAMES), target, **kw)
    for v in range(len(refs)):
        assert (views.tiles(v)["flags"] == am.ACTIVE | am.NO_ESTIMATE).all()
    for j, (want, stats) in enumerate(history):
        st = views.render(SLICE)
        assert st.reference_exact == 1 and all(s.reference_exact == 1 for s in stats)
        for v, cam in enumerate(vc.NAMES):
            got = _state(views, v)
            assert _same(got, want[v]), (j, cam, _differing(got, want[v]))
        assert st.samples == sum(s.samples for s in stats) and st.active_tiles == sum(s.active_tiles for s in stats)
        assert st.active_views == sum(s.active_tiles > 0 for s in stats)
        assert st.converged_tiles == sum(s.converged_tiles for s in stats) and st.capped_tiles == sum(s.capped_tiles for s in stats)
        assert (st.min_samples, st.max_samples) == (min(s.min_samples for s in stats), max(s.max_samples for s in stats))
    st = views.render(SLICE)                                           # nothing is active any more: no launch, nothing moves
    assert (st.samples, st.active_tiles, st.active_views, st.launches) == (0, 0, 0, 0)
    for v in range(len(refs)):
        assert _same(_state(views, v), history[-1][0][v])
    for cam, d in zip(vc.NAMES, final):                                # consequently: rt_render's pixels per count
        _check_picture(scenes, name, cam, w, h, history[-1][0][vc.NAMES.index(cam)], d)
    views.close()
    for r in refs:
        r.close()


def _check_picture(scenes, name, cam, w, h, state, spp):
    """Every pixel against rt_render at its own sample count on the scene created with `cam`, per distinct count; count 0 is zeros."""
    for d in np.unique(spp):
        at = spp == d
        if d == 0:
            assert not state["rgb"][at].any() and not state["rgb8"][at].any()
            continue
        ref, ref8 = _render(scenes, name, cam, w, h, int(d))
        assert np.array_equal(state["rgb"][at], ref.view(np.uint32)[at]), (name, cam, w, h, int(d))
        assert np.array_equal(state["rgb8"][at], ref8[at]), (name, cam, w, h, int(d))


def _tile_masks(n_views, rows, cols):
    """Three hand-made masks per (view, sub-tile): one border sub-tile of the last view alone, a checkerboard whose phase alternates per
    view and that holds that sub-tile, everything but view 0's first sub-tile."""
    alone = np.zeros((n_views, rows, cols), np.uint8)
    alone[-1, -1, -1] = 1
    vv, yy, xx = np.mgrid[0:n_views, 0:rows, 0:cols]
    board = ((vv + yy + xx) % 2 == (n_views - 1 + rows - 1 + cols - 1) % 2).astype(np.uint8)
    rest = np.ones((n_views, rows, cols), np.uint8)
    rest[0, 0, 0] = 0
    return alone, board, rest


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("w,h", GRIDS)
def test_mechanism_equals_rt_render_per_count(rt, scenes, name, w, h):
    views = scenes(name).adaptive_views(w, h, _cams(name, vc.NAMES), 0.05, ray_depth=DEPTH)
    rows, cols = views.grid
    masks = _tile_masks(6, rows, cols)
    flags = [views.tiles(v)["flags"] for v in range(6)]
    for mask in masks:
        st = views.render_tiles(SLICE, mask)
        inside = sum(int(_per_pixel(mask[v], w, h).sum()) for v in range(6))
        assert st.active_tiles == mask.sum() and st.samples == inside * SLICE and st.active_views == mask.reshape(6, -1).any(axis=1).sum()
        assert st.reference_exact == 1 and st.kernel_ms > 0 and st.launches >= 5
    counts = SLICE * sum(m.astype(np.int32) for m in masks)
    assert (st.min_samples, st.max_samples) == (counts.min(), counts.max())
    assert len(np.unique(counts)) >= 3 and counts.max() == 3 * SLICE
    for v, cam in enumerate(vc.NAMES):
        state, tiles = _state(views, v), views.tiles(v)
        assert np.array_equal(tiles["samples"], counts[v]) and np.array_equal(tiles["batches"] * SLICE, counts[v])
        assert np.array_equal(tiles["flags"] & ~np.uint32(am.NO_ESTIMATE), flags[v] & ~np.uint32(am.NO_ESTIMATE))   # the mechanism decides nothing
        assert np.array_equal(state["spp"], _per_pixel(counts[v], w, h))
        _check_picture(scenes, name, cam, w, h, state, state["spp"])
        # a sub-tile with j batches has the uniform run's statistics after j slices
        ref = _uniform(scenes, name, cam, w, h)
        per_pixel = _per_pixel(tiles["batches"], w, h)
        for j in np.unique(tiles["batches"]):
            at, of = per_pixel == j, tiles["batches"] == j
            if j < 2:
                assert ((tiles["flags"][of] & am.NO_ESTIMATE) != 0).all() and not state["se"][at].any() and not tiles["pixels"][of].any()
                continue
            want_tiles, want_se = ref[int(j)]
            assert np.array_equal(state["se"][at], want_se.view(np.uint32)[at]), (cam, int(j))
            for field in ("pixels", "nonfinite", "sum_se2", "sum_luminance"):
                assert np.array_equal(tiles[field][of].view(np.uint32), want_tiles[field][of].view(np.uint32)), (cam, int(j), field)
    views.close()


@pytest.mark.parametrize("name,w,h", [("soup_a", 8, 8), ("soup_a", 43, 21), ("sphere_emissive_env", 40, 24)])
def test_all_active_equals_rt_views(rt, scenes, name, w, h):
    cams = _cams(name, vc.NAMES)
    plain = scenes(name).views(w, h, cams, ray_depth=DEPTH)
    views = scenes(name).adaptive_views(w, h, cams, 0.05, ray_depth=DEPTH)
    ones = np.ones((6,) + views.grid, np.uint8)
    for j in (1, 2, 3):
        plain.render(SLICE)
        st = views.render_tiles(SLICE, ones)
        assert st.samples == 6 * w * h * SLICE and st.active_views == 6
        for v in range(6):
            got, want = views.resolve(v), plain.resolve(v)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]), (j, v)
    views.close(); plain.close()


@pytest.mark.parametrize("name", SCENES)
def test_view_masks_independence_and_set_cameras(rt, scenes, name):
    """A target so low that only sub-tiles without any noise converge: the policy draws for whole views, the view mask decides which."""
    w, h, names = 43, 21, list(vc.NAMES[:5])
    kw = dict(min_batches=2, max_samples=5 * SLICE, ray_depth=DEPTH)
    views = scenes(name).adaptive_views(w, h, _cams(name, names), 1e-6, **kw)
    refs = [scenes(name, cam).adaptive(w, h, 1e-6, **kw) for cam in names]
    for mask in MASKS:
        st = views.render(SLICE, mask)
        drew = [refs[v].render(SLICE) for v in range(5) if mask[v]]
        assert st.active_views == sum(s.samples > 0 for s in drew) and st.samples == sum(s.samples for s in drew)
        for v in range(5):                                            # a view's state after its own slices: the referee's with those slices only
            got, want = _state(views, v), _state(refs[v])
            assert _same(got, want), (mask, v, _differing(got, want))
    assert [int(views.sample_map(v).max()) for v in range(5)] == [SLICE * k for k in (1, 1, 3, 1, 2)]
    # set_cameras on one view resets it and nothing else
    before = [_state(views, v) for v in range(5)]
    views.set_cameras(2, _cams(name, ["far"]))
    for v in (0, 1, 3, 4):
        assert _same(_state(views, v), before[v]), v
    t = views.tiles(2)
    assert (t["flags"] == am.ACTIVE | am.NO_ESTIMATE).all() and not t["samples"].any() and not t["batches"].any()
    rgb, rgb8 = views.resolve(2)
    assert not rgb.any() and not rgb8.any() and not views.sample_map(2).any()
    with pytest.raises(rt.RtError, match="view 2: no sub-tile has 2 batches"):
        views.noise(2)
    fresh = scenes(name, "far").adaptive(w, h, 1e-6, **kw)
    for _ in range(2):
        views.render(SLICE, [0, 0, 1, 0, 0])
        fresh.render(SLICE)
        got, want = _state(views, 2), _state(fresh)
        assert _same(got, want), _differing(got, want)
    for v in (0, 1, 3, 4):
        assert _same(_state(views, v), before[v]), v
    views.close(); fresh.close()
    for r in refs:
        r.close()


def test_launch_count_does_not_grow_with_the_views(rt, scenes):
    w, h, name = 43, 21, "soup_a"
    six = scenes(name).adaptive_views(w, h, _cams(name, vc.NAMES), 0.05, ray_depth=DEPTH)
    one = scenes(name).adaptive_views(w, h, _cams(name, ["inside"]), 0.05, ray_depth=DEPTH)
    plain = scenes(name).views(w, h, _cams(name, vc.NAMES), ray_depth=DEPTH)
    for _ in range(2):
        a = six.render_tiles(SLICE, np.ones((6,) + six.grid, np.uint8))
        b = one.render_tiles(SLICE, np.ones((1,) + one.grid, np.uint8))
        c = plain.render(SLICE)
        print("launches: six views", a.launches, "one view", b.launches, "rt_views_render on the six", c.launches)
        assert a.launches == b.launches and a.active_tiles == 6 * b.active_tiles
        assert a.launches == c.launches + 2                           # rt_views' slice, then one update and one estimate for the whole set
    six.close(); one.close(); plain.close()


def test_chunk_seams(rt, scenes, monkeypatch):
    """RTAMD_QUERY_CHUNK = 128 slots, two sub-tiles a chunk, over three views of 18 sub-tiles: the checkerboard's nine active sub-tiles a
    view make chunks that straddle two views, every chunk's two list entries have a frozen sub-tile between them, and so do the seams;
    the border sub-tile alone is half a chunk."""
    w, h, name, names = 43, 21, "soup_a", ["within", "beside", "skew"]
    whole = scenes(name).adaptive_views(w, h, _cams(name, names), 0.05, ray_depth=DEPTH)
    masks = _tile_masks(3, *whole.grid)
    assert masks[1][0].sum() % 2 == 1
    plain = [whole.render_tiles(SLICE, m) for m in masks]
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "128")
    views = scenes(name).adaptive_views(w, h, _cams(name, names), 0.05, ray_depth=DEPTH)
    for mask, st in zip(masks, plain):
        got = views.render_tiles(SLICE, mask)
        assert got.samples == st.samples and got.active_tiles == st.active_tiles
        assert got.launches > st.launches if mask.sum() > 2 else got.launches == st.launches
    for v in range(3):
        got, want = _state(views, v), _state(whole, v)
        assert _same(got, want), (v, _differing(got, want))
    # and the policy in chunks: the same bits again
    monkeypatch.delenv("RTAMD_QUERY_CHUNK")
    st = whole.render(SLICE)
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "128")
    got = views.render(SLICE)
    assert got.samples == st.samples > 0
    for v in range(3):
        assert _same(_state(views, v), _state(whole, v)), v
    views.close(); whole.close()


def test_the_surroundings_are_untouched(rt, scenes):
    w, h, name = 40, 24, "soup_a"
    scene = scenes(name)
    before = scene.render(w, h, 2 * SLICE, ray_depth=DEPTH)
    acc = scene.accumulator(w, h, ray_depth=DEPTH)
    ad = scene.adaptive(w, h, 0.05, ray_depth=DEPTH)
    plain = scene.views(w, h, _cams(name, ["skew", "far"]), ray_depth=DEPTH)
    board = _tile_masks(1, *ad.grid)[1][0]
    acc.render(SLICE); ad.render_tiles(SLICE, board); plain.render(SLICE)
    a = scene.adaptive_views(w, h, _cams(name, ["far", "within", "beside"]), 0.05, ray_depth=DEPTH)
    b = scene.adaptive_views(w, h, _cams(name, ["skew", "own"]), 0.05, min_batches=2, ray_depth=DEPTH)
    a.render_tiles(SLICE, _tile_masks(3, *a.grid)[1])
    b.render(SLICE)
    a.render(SLICE, [1, 0, 1])
    a.set_cameras(1, _cams(name, ["inside"]))
    b.render(SLICE, [0, 1])
    acc.render(SLICE); ad.render_tiles(SLICE, board); plain.render(SLICE)
    after = scene.render(w, h, 2 * SLICE, ray_depth=DEPTH)
    want = _render(scenes, name, "own", w, h, 2 * SLICE)
    for got in (before, after, acc.resolve()):
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    state = _state(ad)
    _check_picture(scenes, name, "own", w, h, state, _per_pixel(2 * SLICE * board.astype(np.int32), w, h))
    for v, cam in enumerate(["skew", "far"]):
        got, ref = plain.resolve(v), _render(scenes, name, cam, w, h, 2 * SLICE)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1])
    for obj, names in ((a, ["far", "inside", "beside"]), (b, ["skew", "own"])):      # and the sets themselves stand
        for v, cam in enumerate(names):
            state = _state(obj, v)
            _check_picture(scenes, name, cam, w, h, state, state["spp"])
    acc.close(); ad.close(); plain.close(); a.close(); b.close()


def _create(rt, scene, params, adaptive, cams):
    arr = (rt.rt_camera * len(cams))(*cams)
    out = C.c_void_p()
    code = rt.lib.rt_view_adaptive_create(scene._h, C.byref(params), C.byref(adaptive), C.cast(arr, C.c_void_p), C.byref(out))
    assert code != 0 and not out
    return code, rt.lib.rt_last_error().decode()


def test_refusals_name_their_cause_and_leave_the_state(rt, scenes, monkeypatch):
    w, h, name = 40, 24, "soup_a"
    scene = scenes(name)
    unsupported, bad, limit = rt.RT_ERR_UNSUPPORTED, rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    names = ["inside", "within", "far"]
    cams = _cams(name, names)
    views = scene.adaptive_views(w, h, cams, 0.05, ray_depth=DEPTH)   # a good object beforehand
    masks = _tile_masks(3, *views.grid)
    views.render_tiles(SLICE, masks[1])
    views.render_tiles(SLICE, masks[2])
    states = [_state(views, v) for v in range(3)]
    who = "rt_view_adaptive_create: "
    good = lambda: rt.make_views_params(w, h, 3, ray_depth=DEPTH)
    ok = rt.make_adaptive_params(0.05)
    # what rt_views_create refuses
    for fields, code, word in ((dict(struct_size=36), bad, "struct_size"), (dict(flags=1), bad, "flags"), (dict(reserved=(0, 1)), bad, "reserved"),
                               (dict(n_views=0), bad, "n_views"), (dict(n_views=-3), bad, "n_views"), (dict(width=0), bad, "width"),
                               (dict(height=-1), bad, "height"), (dict(width=65536), limit, "width"), (dict(height=70000), limit, "height"),
                               (dict(ray_depth=17), limit, "ray_depth"), (dict(width=4096, height=4096, n_views=128), limit, "n_views")):
        p = good()
        for k, v in fields.items():
            setattr(p, k, v)
        got, msg = _create(rt, scene, p, ok, cams * 43)                # 129 cameras: enough for every n_views tried
        assert got == code and msg.startswith(who) and word in msg, (fields, msg)
    for v, (field, value, word) in enumerate((("position", float("nan"), "position[1]"), ("right", 2.0 ** 41, "right[1]"), ("fov_y", 3.1, "fov_y"))):
        broken = _cams(name, names)
        if field == "fov_y":
            broken[v].fov_y = value
        else:
            getattr(broken[v], field)[1] = value
        got, msg = _create(rt, scene, good(), ok, broken)
        assert got == bad and msg.startswith(who) and word in msg and "view %d" % v in msg, msg
        code = rt.lib.rt_view_adaptive_set_cameras(views._h, 1, 1, C.byref(broken[v]))
        msg = rt.lib.rt_last_error().decode()
        assert code == bad and msg.startswith("rt_view_adaptive_set_cameras: ") and word in msg and "view 1" in msg, msg
    coplanar = vc.camera((0, 0, 6), (1, 0, 0), (0, 1, 0), (1, 1, 0), 0.7)
    got, msg = _create(rt, scene, good(), ok, [cams[0], cams[1], coplanar])
    assert got == bad and "linearly independent" in msg and "view 2" in msg
    # what rt_adaptive_create refuses
    for fields, word in ((dict(target_noise=0.0), "target_noise"), (dict(target_noise=-1.0), "target_noise"), (dict(target_noise=float("nan")), "target_noise"),
                         (dict(target_noise=float("inf")), "target_noise"), (dict(min_batches=1), "min_batches"), (dict(min_batches=-2), "min_batches"),
                         (dict(max_samples=-1), "max_samples"), (dict(flags=2), "RT_ADAPTIVE_DILATE"), (dict(reserved=1), "reserved"),
                         (dict(struct_size=20), "struct_size")):
        ap = rt.make_adaptive_params(0.05)
        for k, v in fields.items():
            setattr(ap, k, v)
        got, msg = _create(rt, scene, good(), ap, cams)
        assert got == bad and msg.startswith(who) and word in msg, (fields, msg)
    # scenes the persistent hw8 kernel does not take
    st = rt.rt_view_adaptive_stats()
    st.struct_size = C.sizeof(st)
    ones = np.ones(masks[0].shape, np.uint8)
    for kernel, word in (("wavefront", "the persistent hw8 kernel does not take this scene or environment"), ("mega", "megakernel is in effect (RTAMD_KERNEL=mega")):
        monkeypatch.setenv("RTAMD_KERNEL", kernel)
        got, msg = _create(rt, scene, good(), ok, cams)
        assert got == unsupported and msg.startswith(who) and word in msg, msg
        assert rt.lib.rt_view_adaptive_render(views._h, SLICE, None, C.byref(st)) == unsupported
        msg = rt.lib.rt_last_error().decode()
        assert msg.startswith("rt_view_adaptive_render: ") and word in msg, msg
        assert rt.lib.rt_view_adaptive_render_tiles(views._h, SLICE, ones.ctypes.data, C.byref(st)) == unsupported
    monkeypatch.delenv("RTAMD_KERNEL")
    hw6 = rt.Scene(pin_cases.hw6_soup(n=40))                          # a scene without vertex normals is an hw6 scene: no hw8 scene
    got, msg = _create(rt, hw6, good(), ok, cams)
    assert got == unsupported and msg.startswith(who) and "RT_INTEGRATOR_HW8" in msg, msg
    hw6.close()
    # what a slice refuses, on the live object
    tiles_call = lambda n, m=ones: (rt.lib.rt_view_adaptive_render_tiles(views._h, n, m.ctypes.data if m is not None else None, C.byref(st)), rt.lib.rt_last_error().decode())
    policy_call = lambda n: (rt.lib.rt_view_adaptive_render(views._h, n, None, C.byref(st)), rt.lib.rt_last_error().decode())
    for n in (0, -4):
        for call in (tiles_call, policy_call):
            code, msg = call(n)
            assert code == bad and "n_samples must be positive" in msg
    code, msg = tiles_call(1 << 25)
    assert code == limit and "n_samples" in msg and "sample index" in msg
    code, msg = tiles_call((1 << 25) - 2 * SLICE)                     # fits view 0's first two sub-tiles, which have drawn 4, not the third, which has drawn 8
    assert code == limit and "n_samples" in msg and "view 0 sub-tile 2" in msg and "sample index" in msg, msg
    code, msg = tiles_call(SLICE, None)
    assert code == bad and "null argument (tile_mask)" in msg
    st.struct_size = 8
    code, msg = tiles_call(SLICE)
    assert code == bad and "stats.struct_size" in msg
    st.struct_size = C.sizeof(st)
    for first, n, word in ((-1, 1, "first"), (3, 1, "first"), (0, 0, "n ("), (1, 3, "n ("), (2, -1, "n (")):
        code = rt.lib.rt_view_adaptive_set_cameras(views._h, first, n, C.cast((rt.rt_camera * 3)(*cams), C.c_void_p))
        msg = rt.lib.rt_last_error().decode()
        assert code == bad and msg.startswith("rt_view_adaptive_set_cameras: ") and word in msg, (first, n, msg)
    buf = np.zeros(w * h * 3, np.float32)
    s = rt.rt_noise_summary()
    s.struct_size = C.sizeof(s)
    for view in (-1, 3):
        for fn, args in ((rt.lib.rt_view_adaptive_tiles, (buf.ctypes.data,)), (rt.lib.rt_view_adaptive_sample_map, (buf.ctypes.data,)),
                         (rt.lib.rt_view_adaptive_resolve, (0, buf.ctypes.data, None)), (rt.lib.rt_view_adaptive_noise, (0, None, C.byref(s)))):
            assert fn(views._h, view, *args) == bad
            assert "view (%d)" % view in rt.lib.rt_last_error().decode()
    assert not buf.any()
    assert rt.lib.rt_view_adaptive_resolve(views._h, 0, 2, None, None) == bad and "RT_FLAG_OUT_DEVICE" in rt.lib.rt_last_error().decode()
    assert rt.lib.rt_view_adaptive_noise(views._h, 0, 2, None, None) == bad and "RT_FLAG_OUT_DEVICE" in rt.lib.rt_last_error().decode()
    for v in range(3):                                                # every refused call left the state where it was
        assert _same(_state(views, v), states[v]), v
    views.render_tiles(SLICE, ones)                                   # and it carries on
    for v, cam in enumerate(names):
        state = _state(views, v)
        _check_picture(scenes, name, cam, w, h, state, state["spp"])
    views.close()

"""Adaptive sampling on the GPU (include/rtamd.h: rt_adaptive_*): a sub-tile that has drawn d samples holds rt_render(samples = d)'s
pixels, floats and bytes, whatever its neighbours drew; with every sub-tile active the object is rt_accum + rt_noise bit for bit; the
statistics of a sub-tile with j batches are the uniform run's after j slices; the policy's flags are tests/adaptive_model.py's after
every slice, converged sub-tiles freeze (or follow their neighbours under RT_ADAPTIVE_DILATE), the cap caps and the run ends; lists of
1, 2 and all sub-tiles, chunk seams, a second object on the scene, and every refusal with its status and cause.
Scenes soup_a and sphere_emissive_env (the environment instance of the kernel), depth 4, slices of 4; frames 8x8 (one sub-tile),
40x24 (15 whole sub-tiles) and 43x21 (6 x 3 with padded right and bottom borders).  The referees are computed once and kept read-only."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as am
import surface_cases as sc

pytestmark = pytest.mark.gpu

SLICE, DEPTH = 4, 4
SIZES = [(8, 8), (40, 24), (43, 21)]
GRIDS = [(40, 24), (43, 21)]                       # more than one sub-tile
SUMMARY = ("batches", "samples_observed", "samples_total", "pixels", "nonfinite_pixels", "mean_luminance", "rms_error", "noise", "worst_tile_noise")
_RENDER, _UNIFORM, _MECH = {}, {}, {}


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = rt.Scene(sc.scene_data(name))
        return made[name]
    yield get
    for s in made.values():
        s.close()


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _render(scenes, name, w, h, d):
    """rt_render(samples = d): the referee of every sub-tile that has drawn d samples."""
    key = (name, w, h, d)
    if key not in _RENDER:
        rgb, rgb8, _ = scenes(name).render(w, h, d, ray_depth=DEPTH)
        _RENDER[key] = _ro(rgb, rgb8)
    return _RENDER[key]


def _uniform(scenes, name, w, h, k):
    """rt_accum + rt_noise in slices of SLICE: per j = 1 .. k the picture, and from j = 2 on the map and the summary's fields."""
    key = (name, w, h)
    have = _UNIFORM.setdefault(key, {})
    if len(have) < k:
        have.clear()
        acc = scenes(name).accumulator(w, h, ray_depth=DEPTH)
        mon = acc.noise_monitor()
        for j in range(1, k + 1):
            acc.render(SLICE)
            mon.update()
            rgb, rgb8 = acc.resolve()
            se, s = mon.estimate() if j >= 2 else (None, None)
            have[j] = (_ro(rgb, rgb8), None if se is None else _ro(se)[0], None if s is None else tuple(getattr(s, f) for f in SUMMARY))
        acc.close()
    return have


def _masks(rows, cols):
    """Three hand-made masks: a border sub-tile alone (the last one), the checkerboard that holds it, all but the first."""
    alone = np.zeros((rows, cols), np.uint8)
    alone[-1, -1] = 1
    yy, xx = np.mgrid[0:rows, 0:cols]
    board = ((yy + xx) % 2 == (rows - 1 + cols - 1) % 2).astype(np.uint8)
    rest = np.ones((rows, cols), np.uint8)
    rest[0, 0] = 0
    return alone, board, rest


def _mechanism(scenes, name, w, h):
    """Three render_tiles slices with the hand-made masks, once per case: everything the object then says."""
    key = (name, w, h)
    if key not in _MECH:
        a = scenes(name).adaptive(w, h, 0.05, ray_depth=DEPTH)
        masks = _masks(*a.grid)
        stats = [a.render_tiles(SLICE, m) for m in masks]
        rgb, rgb8 = a.resolve()
        se, summary = a.noise()
        _MECH[key] = dict(masks=masks, stats=stats, rgb=rgb, rgb8=rgb8, spp=a.sample_map(), tiles=a.tiles(), se=se, summary=summary)
        a.close()
    return _MECH[key]


def _per_pixel(tile_values, w, h):
    return np.repeat(np.repeat(tile_values, 8, axis=0), 8, axis=1)[:h, :w]


def _check_picture(scenes, name, w, h, rgb, rgb8, spp):
    """Every pixel against rt_render at its own sample count, per distinct count; count 0 is zeros."""
    for d in np.unique(spp):
        at = spp == d
        if d == 0:
            assert not rgb[at].any() and not rgb8[at].any()
            continue
        ref, ref8 = _render(scenes, name, w, h, int(d))
        assert np.array_equal(rgb[at].view(np.uint32), ref[at].view(np.uint32)), (name, w, h, int(d))
        assert np.array_equal(rgb8[at], ref8[at]), (name, w, h, int(d))


@pytest.mark.parametrize("name", ["soup_a", "sphere_emissive_env"])
@pytest.mark.parametrize("w,h", GRIDS)
def test_mechanism_equals_rt_render_per_count(rt, scenes, name, w, h):
    m = _mechanism(scenes, name, w, h)
    counts = SLICE * sum(x.astype(np.int32) for x in m["masks"])
    assert np.array_equal(m["tiles"]["samples"], counts) and np.array_equal(m["tiles"]["batches"] * SLICE, counts)
    assert np.array_equal(m["spp"], _per_pixel(counts, w, h))
    assert len(np.unique(counts)) >= 3 and counts.max() == 3 * SLICE
    _check_picture(scenes, name, w, h, m["rgb"], m["rgb8"], m["spp"])
    for st, mask in zip(m["stats"], m["masks"]):
        inside = _per_pixel(mask, w, h).sum()
        assert st.active_tiles == mask.sum() and st.samples == int(inside) * SLICE
        assert st.reference_exact == 1 and st.launches >= 5 and st.kernel_ms > 0
    assert m["stats"][0].active_tiles == 1                       # the border sub-tile alone
    assert (m["stats"][-1].min_samples, m["stats"][-1].max_samples) == (int(counts.min()), int(counts.max()))


@pytest.mark.parametrize("name,w,h", [("soup_a", *s) for s in SIZES] + [("sphere_emissive_env", 43, 21)])
def test_uniform_case_equals_accum_and_noise(rt, scenes, name, w, h):
    k = 3
    ref = _uniform(scenes, name, w, h, k)
    a = scenes(name).adaptive(w, h, 0.05, ray_depth=DEPTH)
    ones = np.ones(a.grid, np.uint8)
    for j in range(1, k + 1):
        a.render_tiles(SLICE, ones)
        rgb, rgb8 = a.resolve()
        (want, want8), want_se, want_summary = ref[j]
        assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32)) and np.array_equal(rgb8, want8), j
        if j < 2:
            with pytest.raises(rt.RtError, match="2 batches"):
                a.noise()
            continue
        se, s = a.noise()
        assert np.array_equal(se.view(np.uint32), want_se.view(np.uint32)), j
        assert tuple(getattr(s, f) for f in SUMMARY) == want_summary, j
    _check_picture(scenes, name, w, h, rgb, rgb8, a.sample_map())
    a.close()


@pytest.mark.parametrize("name", ["soup_a", "sphere_emissive_env"])
@pytest.mark.parametrize("w,h", GRIDS)
def test_statistics_of_a_sub_tile_are_its_own(rt, scenes, name, w, h):
    """The map over the sub-tiles with j batches is the uniform run's after j slices; fewer than 2 batches: NO_ESTIMATE and 0."""
    m = _mechanism(scenes, name, w, h)
    batches = m["tiles"]["batches"]
    per_pixel = _per_pixel(batches, w, h)
    ref = _uniform(scenes, name, w, h, int(batches.max()))
    seen = 0
    for j in np.unique(batches):
        at = per_pixel == j
        none = (m["tiles"]["flags"][batches == j] & am.NO_ESTIMATE) != 0
        if j < 2:
            assert none.all() and not m["se"][at].any()
            assert not m["tiles"]["pixels"][batches == j].any() and not m["tiles"]["sum_se2"][batches == j].any()
            continue
        assert not none.any()
        assert np.array_equal(m["se"][at].view(np.uint32), ref[int(j)][1][at].view(np.uint32)), int(j)
        seen += 1
    assert seen >= 2
    s = m["summary"]                                              # the frame figures: over the sub-tiles that have an estimate
    have = batches >= 2
    assert s.batches == batches.max() and s.samples_total == SLICE * batches.max()
    assert s.pixels == int(m["tiles"]["pixels"][have].sum()) and s.pixels <= _per_pixel(have, w, h).sum()
    assert s.mean_luminance == am.mean_luminance(m["tiles"])


def _tile_noise_of_map(se, rows, cols):
    """sqrt(mean se^2) per sub-tile from a map, float64."""
    out = np.zeros((rows, cols))
    for y in range(rows):
        for x in range(cols):
            out[y, x] = np.sqrt(np.mean(se[8 * y:8 * y + 8, 8 * x:8 * x + 8].astype(np.float64) ** 2))
    return out


def _policy_run(rt, scenes, name, w, h, target, min_batches, max_samples, dilate):
    """rt_adaptive_render until nothing is active; after every slice the flags against the model.  Returns the history of tile tables."""
    a = scenes(name).adaptive(w, h, target, min_batches=min_batches, max_samples=max_samples, dilate=dilate, ray_depth=DEPTH)
    flags = am.DILATE if dilate else 0
    history = [a.tiles()]
    assert (history[0]["flags"] == am.ACTIVE | am.NO_ESTIMATE).all()
    for _ in range(max_samples // SLICE + 2):                     # the run ends: the cap sees to it
        before = history[-1]
        st = a.render(SLICE)
        now = a.tiles()
        drew = (before["flags"] & am.ACTIVE) != 0                  # the slice's active set is the last decision's
        if max_samples:
            drew &= before["samples"] + SLICE <= max_samples
        assert np.array_equal(now["samples"], before["samples"] + SLICE * drew)
        assert st.active_tiles == drew.sum() and st.samples == SLICE * int(_per_pixel(drew, w, h).sum())
        if st.samples == 0:
            assert st.launches == 0 and np.array_equal(now, before)
            break
        model_in = now.copy()                                      # the new sums under the last decision's flags
        model_in["flags"] = (before["flags"] & ~np.uint32(am.NO_ESTIMATE)) | np.where(now["batches"] < 2, am.NO_ESTIMATE, 0).astype(np.uint32)
        want = am.decide(model_in, target, min_batches, max_samples, flags, SLICE)
        assert np.array_equal(now["flags"], want), (len(history), now["flags"], want)
        assert st.converged_tiles == ((want & am.CONVERGED) != 0).sum() and st.capped_tiles == ((want & am.CAPPED) != 0).sum()
        history.append(now)
    else:
        raise AssertionError("the run did not end")
    final = history[-1]
    assert ((final["flags"] & am.ACTIVE) == 0).all() and ((final["flags"] & (am.CONVERGED | am.CAPPED)) != 0).all()
    assert final["samples"].max() <= max_samples
    rgb, rgb8 = a.resolve()
    _check_picture(scenes, name, w, h, rgb, rgb8, a.sample_map())
    a.close()
    return history


@pytest.mark.parametrize("w,h", GRIDS)
def test_policy(rt, scenes, w, h):
    name, min_batches, max_samples = "sphere_emissive_env", 3, 20      # lit by its environment: every sub-tile has noise of its own
    ref = _uniform(scenes, name, w, h, min_batches)
    se, summary = ref[min_batches][1], dict(zip(SUMMARY, ref[min_batches][2]))
    rows, cols = (h + 7) // 8, (w + 7) // 8
    target = float(np.float32(np.median(_tile_noise_of_map(se, rows, cols)) / summary["mean_luminance"]))
    assert target > 0
    history = _policy_run(rt, scenes, name, w, h, target, min_batches, max_samples, False)
    first = history[min_batches]["flags"]                          # the first decision that judges anything
    assert ((history[min_batches - 1]["flags"] & am.CONVERGED) == 0).all()
    n = rows * cols
    assert ((first & am.CONVERGED) != 0).sum() * 4 >= n and ((first & am.ACTIVE) != 0).sum() * 4 >= n
    for before, now in zip(history, history[1:]):                  # a converged sub-tile's count stops growing
        frozen = (before["flags"] & am.CONVERGED) != 0
        assert np.array_equal(now["samples"][frozen], before["samples"][frozen])
        assert ((now["flags"] & am.CONVERGED) != 0)[frozen].all()  # and it stays converged
    final = history[-1]
    capped = (final["flags"] & am.CAPPED) != 0
    assert capped.any() and (final["samples"][capped] + SLICE > max_samples).all()
    assert len(np.unique(final["samples"])) >= 2
    # the same with RT_ADAPTIVE_DILATE: a converged sub-tile next to an unfinished one goes on drawing
    dilated = _policy_run(rt, scenes, name, w, h, target, min_batches, max_samples, True)
    assert np.array_equal(dilated[min_batches]["flags"] & am.CONVERGED, first & am.CONVERGED)   # the same sums up to there
    kept = (dilated[min_batches]["flags"] & (am.CONVERGED | am.ACTIVE)) == (am.CONVERGED | am.ACTIVE)
    assert kept.any()
    assert (dilated[min_batches + 1]["samples"][kept] == dilated[min_batches]["samples"][kept] + SLICE).all()
    assert dilated[-1]["samples"].sum() > final["samples"].sum()


@pytest.mark.parametrize("w,h", SIZES)
def test_lists_of_one_two_and_all(rt, scenes, w, h):
    a = scenes("soup_a").adaptive(w, h, 0.05, ray_depth=DEPTH)
    rows, cols = a.grid
    n = rows * cols
    for active in ([n // 2], [0, n - 1], list(range(n))):
        mask = np.zeros(n, np.uint8)
        mask[active] = 1
        assert a.render_tiles(SLICE, mask).active_tiles == len(set(active))
    rgb, rgb8 = a.resolve()
    _check_picture(scenes, "soup_a", w, h, rgb, rgb8, a.sample_map())
    empty = a.render_tiles(SLICE, np.zeros(n, np.uint8))          # nothing to do: no launch, nothing moves
    assert (empty.active_tiles, empty.samples, empty.launches) == (0, 0, 0)
    again, again8 = a.resolve()
    assert np.array_equal(again.view(np.uint32), rgb.view(np.uint32)) and np.array_equal(again8, rgb8)
    a.close()


def test_chunk_seams(rt, scenes, monkeypatch):
    """RTAMD_QUERY_CHUNK = 128 slots: the 18 sub-tiles of 43x21 run two at a time, nine chunks a slice."""
    w, h = 43, 21
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "128")
    a = scenes("soup_a").adaptive(w, h, 0.05, ray_depth=DEPTH)
    masks = _masks(*a.grid)
    whole = _mechanism(scenes, "soup_a", w, h)
    for mask, st in zip(masks, whole["stats"]):
        got = a.render_tiles(SLICE, mask)
        assert got.samples == st.samples and got.active_tiles == st.active_tiles
        assert got.launches > st.launches if mask.sum() > 2 else got.launches == st.launches
    rgb, rgb8 = a.resolve()
    assert np.array_equal(rgb.view(np.uint32), whole["rgb"].view(np.uint32)) and np.array_equal(rgb8, whole["rgb8"])
    assert np.array_equal(a.noise()[0].view(np.uint32), whole["se"].view(np.uint32))
    a.close()


def test_a_second_object_and_other_renders_between(rt, scenes):
    w, h = 40, 24
    scene = scenes("soup_a")
    a, b = scene.adaptive(w, h, 0.05, ray_depth=DEPTH), scene.adaptive(w, h, 0.05, ray_depth=DEPTH)
    ones = np.ones(b.grid, np.uint8)
    alone, board, _ = _masks(*b.grid)
    b.render_tiles(SLICE, board)
    a.render_tiles(SLICE, ones)
    scene.render(64, 64, 2, ray_depth=6)                           # the scene's path records and counters are everybody's
    acc = scene.accumulator(w, h, ray_depth=DEPTH)
    acc.render(SLICE)
    b.render_tiles(SLICE, alone)
    acc.render(SLICE)
    a.render_tiles(SLICE, ones)
    for obj in (a, b):
        rgb, rgb8 = obj.resolve()
        _check_picture(scenes, "soup_a", w, h, rgb, rgb8, obj.sample_map())
    assert np.array_equal(b.sample_map(), _per_pixel(SLICE * (board.astype(np.int32) + alone), w, h))
    want, want8 = _render(scenes, "soup_a", w, h, 2 * SLICE)
    got, got8 = acc.resolve()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got8, want8)
    acc.close(); a.close(); b.close()


def _create(rt, scene, params, adaptive):
    out = C.c_void_p()
    code = rt.lib.rt_adaptive_create(scene._h, C.byref(params), C.byref(adaptive), C.byref(out))
    assert code != 0 and not out
    return code, rt.lib.rt_last_error().decode()


def test_refusals_name_their_cause_and_leave_the_state(rt, scenes, monkeypatch):
    w, h = 40, 24
    scene = scenes("soup_a")
    ok = rt.make_adaptive_params(0.05)
    unsupported, bad, limit = rt.RT_ERR_UNSUPPORTED, rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    for kw, word in ((dict(integrator=rt.RT_INTEGRATOR_HW7), "RT_INTEGRATOR_HW8"), (dict(integrator=rt.RT_INTEGRATOR_HW6), "RT_INTEGRATOR_HW8"),
                     (dict(shard_count=2), "shard_count > 1"), (dict(sample_streams=2), "sample_streams > 1"),
                     (dict(flags=rt.RT_FLAG_COUNTERS), "render flags other than 0"), (dict(flags=rt.RT_FLAG_OUT_DEVICE), "render flags other than 0")):
        code, msg = _create(rt, scene, rt.make_params(w, h, 0, ray_depth=DEPTH, **kw), ok)
        assert code == unsupported and msg.startswith("rt_adaptive_create: ") and word in msg, (kw, msg)
    for kernel, word in (("wavefront", "the persistent hw8 kernel does not take this scene or environment"), ("mega", "megakernel is in effect (RTAMD_KERNEL=mega")):
        monkeypatch.setenv("RTAMD_KERNEL", kernel)
        code, msg = _create(rt, scene, rt.make_params(w, h, 0, ray_depth=DEPTH), ok)
        assert code == unsupported and msg.startswith("rt_adaptive_create: ") and word in msg, msg
    monkeypatch.delenv("RTAMD_KERNEL")
    good = rt.make_params(w, h, 0, ray_depth=DEPTH)
    for fields, word in ((dict(target_noise=0.0), "target_noise"), (dict(target_noise=-1.0), "target_noise"), (dict(target_noise=float("nan")), "target_noise"),
                         (dict(target_noise=float("inf")), "target_noise"), (dict(min_batches=1), "min_batches"), (dict(min_batches=-2), "min_batches"),
                         (dict(max_samples=-1), "max_samples"), (dict(flags=2), "RT_ADAPTIVE_DILATE"), (dict(reserved=1), "reserved"),
                         (dict(struct_size=20), "struct_size")):
        p = rt.make_adaptive_params(0.05)
        for k, v in fields.items():
            setattr(p, k, v)
        code, msg = _create(rt, scene, good, p)
        assert code == bad and word in msg, (fields, msg)
    code, msg = _create(rt, scene, rt.make_params(w, 0, 0, ray_depth=DEPTH), ok)
    assert code == bad and "positive" in msg
    code, msg = _create(rt, scene, rt.make_params(w, h, 0, ray_depth=17), ok)
    assert code == bad and "ray_depth" in msg
    code, msg = _create(rt, scene, rt.make_params(70000, 8, 0, ray_depth=DEPTH), ok)
    assert code == limit and "65,536" in msg
    # a live object: every refused slice leaves the state where it was
    a = scene.adaptive(w, h, 0.05, ray_depth=DEPTH)
    alone, board, _ = _masks(*a.grid)
    a.render_tiles(SLICE, board)
    a.render_tiles(SLICE, alone)
    rgb, rgb8 = a.resolve()
    tiles = a.tiles()
    st = rt.rt_adaptive_stats()
    st.struct_size = C.sizeof(st)
    mask = np.ones(a.grid, np.uint8)
    call = lambda n, m=mask: (rt.lib.rt_adaptive_render_tiles(a._h, n, m.ctypes.data if m is not None else None, C.byref(st)), rt.lib.rt_last_error().decode())
    for n in (0, -4):
        code, msg = call(n)
        assert code == bad and "n_samples must be positive" in msg
        assert rt.lib.rt_adaptive_render(a._h, n, None) == bad
    code, msg = call(1 << 25)
    assert code == limit and "sample index" in msg
    code, msg = call((1 << 25) - 2 * SLICE)                        # fits a fresh sub-tile, not one that has drawn 8
    assert code == limit and "sub-tile" in msg and "sample index" in msg
    code, msg = call(SLICE, None)
    assert code == bad and "null argument (mask)" in msg
    monkeypatch.setenv("RTAMD_KERNEL", "wavefront")
    code, msg = call(SLICE)
    assert code == unsupported and "the persistent hw8 kernel does not take this scene or environment" in msg
    assert rt.lib.rt_adaptive_render(a._h, SLICE, None) == unsupported
    monkeypatch.delenv("RTAMD_KERNEL")
    assert rt.lib.rt_adaptive_resolve(a._h, 2, None, None) == bad and "RT_FLAG_OUT_DEVICE" in rt.lib.rt_last_error().decode()
    assert rt.lib.rt_adaptive_noise(a._h, 2, None, None) == bad
    again, again8 = a.resolve()
    assert np.array_equal(again.view(np.uint32), rgb.view(np.uint32)) and np.array_equal(again8, rgb8)
    assert np.array_equal(a.tiles(), tiles)
    a.render_tiles(SLICE, mask)                                    # and it carries on
    got, got8 = a.resolve()
    _check_picture(scenes, "soup_a", w, h, got, got8, a.sample_map())
    a.close()

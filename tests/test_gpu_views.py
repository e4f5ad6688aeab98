"""View sets on the GPU (include/rtamd.h: rt_views_*): view v after d samples holds, floats and bytes, what rt_render(samples = d)
returns on a scene created with camera = cameras[v] -- for every camera of tests/view_cases.py on soup_a and on sphere_emissive_env
(the environment instance of the kernel), after every slice, whatever the other views drew; three of them also against the CPU oracle,
which knows nothing of grids; cameras outside the node grid or beyond the origin bound go to the exact role, the others to the walkers;
masks, set_cameras, chunk seams, the scene and its other objects untouched, and every refusal with its status and cause.
Depth 4, slices of 4; frames 8x8, 40x24 and 43x21.  The referees are computed once and kept read-only."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import pin_cases
import surface_cases as sc
import view_cases as vc

pytestmark = pytest.mark.gpu

SLICE, DEPTH = vc.SLICE, vc.DEPTH
SCENES = ["soup_a", "sphere_emissive_env"]
_REF = {}


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


def _ref(scenes, name, cam, w, h, d):
    """rt_render(samples = d) on the scene created with camera `cam`: (rgb, rgb8, rt_stats)."""
    key = (name, cam, w, h, d)
    if key not in _REF:
        rgb, rgb8, st = scenes(name, cam).render(w, h, d, ray_depth=DEPTH)
        _REF[key] = _ro(rgb, rgb8) + (st,)
    return _REF[key]


def _cams(name, names):
    t = vc.table(sc.scene_data(name))
    return [t[n] for n in names]


def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def _check_views(scenes, name, names, w, h, views, counts):
    for v, (cam, d) in enumerate(zip(names, counts)):
        assert _same(views.resolve(v), _ref(scenes, name, cam, w, h, int(d))), (name, cam, w, h, int(d))


@pytest.mark.parametrize("name", SCENES)
def test_every_camera_equals_a_fresh_scene_after_every_slice(rt, scenes, name):
    w, h = 43, 21
    views = scenes(name).views(w, h, _cams(name, vc.NAMES), ray_depth=DEPTH)
    for j in (1, 2, 3):
        st = views.render(SLICE)
        assert st.reference_exact == 1 and st.active_views == 6 and st.samples == 6 * w * h * SLICE
        assert (st.min_samples, st.max_samples) == (SLICE * j, SLICE * j)
        for cam in vc.NAMES:
            assert _ref(scenes, name, cam, w, h, SLICE * j)[2].reference_exact == 1
        _check_views(scenes, name, vc.NAMES, w, h, views, [SLICE * j] * 6)
    views.close()


def test_against_the_cpu_oracle(rt, scenes):
    w, h, names = 40, 24, ("inside", "beside", "far")
    sd = sc.scene_data("soup_a")
    views = scenes("soup_a").views(w, h, _cams("soup_a", names), ray_depth=DEPTH)
    views.render(SLICE)
    for v, cam in enumerate(names):
        want = oracle_lib.Hw8Oracle(vc.swapped(sd, vc.table(sd)[cam])).render(w, h, SLICE, ray_depth=DEPTH)
        assert _same(views.resolve(v), want[:2]), cam
    views.close()


@pytest.mark.parametrize("name", SCENES)
def test_routing(rt, scenes, name):
    w, h = 43, 21
    outside, fast = ("beside", "far"), ("own", "inside", "within")
    views = scenes(name).views(w, h, _cams(name, outside), ray_depth=DEPTH)
    st = views.render(SLICE)
    print(name, "outside: exact_walks", st.exact_walks, "camera samples", st.samples)
    assert st.exact_walks >= st.samples == 2 * w * h * SLICE         # every first ray went to the exact role
    views.close()
    for cam in fast:                                                  # the referee itself stays under the bound the views are held to
        ref = _ref(scenes, name, cam, w, h, SLICE)[2]
        print(name, cam, "referee: exact walks", ref.exact_closest_hits + ref.exact_light_sums, "camera samples", w * h * SLICE)
        assert 2 * (ref.exact_closest_hits + ref.exact_light_sums) < w * h * SLICE, cam
    views = scenes(name).views(w, h, _cams(name, fast), ray_depth=DEPTH)
    st = views.render(SLICE)
    print(name, "fast: exact_walks", st.exact_walks, "camera samples", st.samples)
    assert st.samples == 3 * w * h * SLICE and 2 * st.exact_walks < st.samples   # the fast path is really taken
    views.close()


MASKS = ([0, 0, 1, 0, 0], [1, 0, 1, 0, 1], [0, 1, 1, 1, 1])         # one alone, alternating, all but the first: counts 1 1 3 1 2 slices


@pytest.mark.parametrize("name", SCENES)
def test_masks_and_independence(rt, scenes, name):
    w, h, names = 43, 21, vc.NAMES[:5]
    views = scenes(name).views(w, h, _cams(name, names), ray_depth=DEPTH)
    counts = np.zeros(5, np.int32)
    assert np.array_equal(views.samples(), counts)
    for mask in MASKS:
        st = views.render(SLICE, mask)
        counts += SLICE * np.array(mask, np.int32)
        assert np.array_equal(views.samples(), counts)
        assert st.active_views == sum(mask) and st.samples == sum(mask) * w * h * SLICE
        assert (st.min_samples, st.max_samples) == (counts.min(), counts.max()) and st.launches >= 3
    assert len(set(counts.tolist())) >= 3 and list(counts) == [SLICE * k for k in (1, 1, 3, 1, 2)]
    _check_views(scenes, name, names, w, h, views, counts)
    views.close()


def test_one_view_of_one_sub_tile(rt, scenes):
    w, h = 8, 8
    views = scenes("soup_a").views(w, h, _cams("soup_a", ["inside"]), ray_depth=DEPTH)
    for mask, total in (([1], 1), ([0], 1), (None, 2)):
        st = views.render(SLICE, mask)
        active = 0 if mask == [0] else 1
        assert (st.active_views, st.samples) == (active, active * w * h * SLICE)
        assert (st.min_samples, st.max_samples) == (SLICE * total, SLICE * total)
        if not active:
            assert st.launches == 0                                   # nothing to do: no launch, nothing moves
        assert list(views.samples()) == [SLICE * total]
        _check_views(scenes, "soup_a", ["inside"], w, h, views, [SLICE * total])
    views.close()


def test_set_cameras(rt, scenes):
    w, h, name = 43, 21, "soup_a"
    names = ["inside", "skew", "far"]
    bad = rt.RT_ERR_INVALID_ARG
    views = scenes(name).views(w, h, _cams(name, names), ray_depth=DEPTH)
    views.render(SLICE)
    views.render(SLICE)
    first = [views.resolve(v) for v in range(3)]
    views.set_cameras(1, _cams(name, ["beside"]))
    assert list(views.samples()) == [2 * SLICE, 0, 2 * SLICE]
    assert rt.lib.rt_views_resolve(views._h, 1, 0, None, None) == bad and "view 1 has no samples" in rt.lib.rt_last_error().decode()
    for v in (0, 2):
        assert _same(views.resolve(v), first[v])                      # the other views' pictures: unchanged bytes
    st = views.render(SLICE, [0, 1, 0])
    assert st.active_views == 1 and (st.min_samples, st.max_samples) == (SLICE, 2 * SLICE)
    _check_views(scenes, name, ["inside", "beside", "far"], w, h, views, [2 * SLICE, SLICE, 2 * SLICE])
    views.set_cameras(1, _cams(name, ["skew"]))                       # back to the camera it had: the first pictures again
    views.render(SLICE, [0, 1, 0])
    views.render(SLICE, [0, 1, 0])
    for v in range(3):
        assert _same(views.resolve(v), first[v])
    views.close()


def test_chunk_seams(rt, scenes, monkeypatch):
    """RTAMD_QUERY_CHUNK = 128 slots: the 54 sub-tiles of three views at 43x21 run two at a time, chunks that straddle two views among them."""
    w, h, name, names = 43, 21, "soup_a", ["within", "beside", "skew"]
    whole = scenes(name).views(w, h, _cams(name, names), ray_depth=DEPTH)
    plain = [whole.render(SLICE, m) for m in (None, [1, 0, 1])]
    monkeypatch.setenv("RTAMD_QUERY_CHUNK", "128")
    views = scenes(name).views(w, h, _cams(name, names), ray_depth=DEPTH)
    for mask, st in zip((None, [1, 0, 1]), plain):
        got = views.render(SLICE, mask)
        assert got.samples == st.samples and got.launches > st.launches
    for v in range(3):
        assert _same(views.resolve(v), whole.resolve(v))
    _check_views(scenes, name, names, w, h, views, [2 * SLICE, SLICE, 2 * SLICE])
    views.close(); whole.close()


def test_the_scene_is_untouched(rt, scenes):
    w, h, name = 40, 24, "soup_a"
    scene = scenes(name)
    before = scene.render(w, h, 2 * SLICE, ray_depth=DEPTH)
    acc = scene.accumulator(w, h, ray_depth=DEPTH)
    acc.render(SLICE)
    a = scene.views(w, h, _cams(name, ["far", "within", "beside"]), ray_depth=DEPTH)
    b = scene.views(w, h, _cams(name, ["skew", "far"]), ray_depth=DEPTH)
    a.render(SLICE)
    b.render(SLICE, [0, 1])
    a.render(SLICE, [1, 1, 0])
    a.set_cameras(2, _cams(name, ["inside"]))
    b.render(SLICE)
    a.render(SLICE, [0, 0, 1])
    acc.render(SLICE)
    after = scene.render(w, h, 2 * SLICE, ray_depth=DEPTH)
    assert _same(after, before) and _same(before, _ref(scenes, name, "own", w, h, 2 * SLICE))
    assert _same(acc.resolve(), before)                               # the plain sliced frame
    _check_views(scenes, name, ["far", "within", "inside"], w, h, a, [2 * SLICE, 2 * SLICE, SLICE])
    _check_views(scenes, name, ["skew", "far"], w, h, b, [SLICE, 2 * SLICE])
    acc.close(); a.close(); b.close()


def _create(rt, scene, params, cams):
    arr = (rt.rt_camera * len(cams))(*cams)
    out = C.c_void_p()
    code = rt.lib.rt_views_create(scene._h, C.byref(params), C.cast(arr, C.c_void_p), C.byref(out))
    assert code != 0 and not out
    return code, rt.lib.rt_last_error().decode()


def test_refusals_name_their_cause_and_leave_the_state(rt, scenes, monkeypatch):
    w, h, name = 40, 24, "soup_a"
    scene = scenes(name)
    unsupported, bad, limit = rt.RT_ERR_UNSUPPORTED, rt.RT_ERR_INVALID_ARG, rt.RT_ERR_LIMIT
    names = ["inside", "within", "far"]
    cams = _cams(name, names)
    views = scene.views(w, h, cams, ray_depth=DEPTH)                  # a good object beforehand
    views.render(SLICE)
    views.render(SLICE, [0, 1, 1])
    counts = [SLICE, 2 * SLICE, 2 * SLICE]
    pictures = [views.resolve(v) for v in range(3)]
    who = "rt_views_create: "
    good = lambda **kw: rt.make_views_params(w, h, 3, ray_depth=DEPTH, **kw)
    for fields, code, word in ((dict(struct_size=36), bad, "struct_size"), (dict(flags=1), bad, "flags"), (dict(reserved=(0, 1)), bad, "reserved"),
                               (dict(reserved=(7, 0)), bad, "reserved"), (dict(n_views=0), bad, "n_views"), (dict(n_views=-3), bad, "n_views"),
                               (dict(width=0), bad, "width"), (dict(height=-1), bad, "height"), (dict(width=65536), limit, "width"),
                               (dict(height=70000), limit, "height"), (dict(ray_depth=17), limit, "ray_depth"),
                               (dict(width=4096, height=4096, n_views=128), limit, "n_views")):
        p = good()
        for k, v in fields.items():
            setattr(p, k, v)
        got, msg = _create(rt, scene, p, cams * 43)                   # 129 cameras: enough for every n_views tried
        assert got == code and msg.startswith(who) and word in msg, (fields, msg)
    for v, (field, value, word) in enumerate((("position", float("nan"), "position[1]"), ("right", 2.0 ** 41, "right[1]"), ("fov_y", 3.1, "fov_y"))):
        broken = _cams(name, names)
        if field == "fov_y":
            broken[v].fov_y = value
        else:
            getattr(broken[v], field)[1] = value
        got, msg = _create(rt, scene, good(), broken)
        assert got == bad and msg.startswith(who) and word in msg and "view %d" % v in msg, msg
        code = rt.lib.rt_views_set_cameras(views._h, 1, 1, C.byref(broken[v]))
        msg = rt.lib.rt_last_error().decode()
        assert code == bad and msg.startswith("rt_views_set_cameras: ") and word in msg and "view 1" in msg, msg
    coplanar = vc.camera((0, 0, 6), (1, 0, 0), (0, 1, 0), (1, 1, 0), 0.7)
    got, msg = _create(rt, scene, good(), [cams[0], cams[1], coplanar])
    assert got == bad and "linearly independent" in msg and "view 2" in msg
    for kernel, word in (("wavefront", "the persistent hw8 kernel does not take this scene or environment"), ("mega", "megakernel is in effect (RTAMD_KERNEL=mega")):
        monkeypatch.setenv("RTAMD_KERNEL", kernel)
        got, msg = _create(rt, scene, good(), cams)
        assert got == unsupported and msg.startswith(who) and word in msg, msg
        st = rt.rt_views_stats()
        st.struct_size = C.sizeof(st)
        assert rt.lib.rt_views_render(views._h, SLICE, None, C.byref(st)) == unsupported
        msg = rt.lib.rt_last_error().decode()
        assert msg.startswith("rt_views_render: ") and word in msg, msg
    monkeypatch.delenv("RTAMD_KERNEL")
    hw6 = rt.Scene(pin_cases.hw6_soup(n=40))                          # a scene without vertex normals is an hw6 scene: no hw8 scene
    got, msg = _create(rt, hw6, good(), cams)
    assert got == unsupported and msg.startswith(who) and "RT_INTEGRATOR_HW8" in msg, msg
    hw6.close()
    # the live object: every refused call leaves counts and pictures where they were
    st = rt.rt_views_stats()
    st.struct_size = C.sizeof(st)
    ones = np.ones(3, np.uint8)
    render = lambda n, mask=None: (rt.lib.rt_views_render(views._h, n, mask.ctypes.data if mask is not None else None, C.byref(st)), rt.lib.rt_last_error().decode())
    for n in (0, -4):
        code, msg = render(n)
        assert code == bad and msg == "rt_views_render: n_samples must be positive"
    code, msg = render(1 << 25)
    assert code == limit and "n_samples" in msg and "view 0" in msg and "sample index" in msg
    code, msg = render((1 << 25) - 2 * SLICE)                         # fits the view that has drawn 4, not those that have drawn 8
    assert code == limit and "view 1" in msg and "sample index" in msg
    st.struct_size = 8
    code, msg = render(SLICE, ones)
    assert code == bad and "stats.struct_size" in msg
    st.struct_size = C.sizeof(st)
    for first, n, word in ((-1, 1, "first"), (3, 1, "first"), (0, 0, "n ("), (1, 3, "n ("), (2, -1, "n (")):
        code = rt.lib.rt_views_set_cameras(views._h, first, n, C.cast((rt.rt_camera * 3)(*cams), C.c_void_p))
        msg = rt.lib.rt_last_error().decode()
        assert code == bad and msg.startswith("rt_views_set_cameras: ") and word in msg, (first, n, msg)
    for view in (-1, 3):
        assert rt.lib.rt_views_resolve(views._h, view, 0, None, None) == bad
        msg = rt.lib.rt_last_error().decode()
        assert msg.startswith("rt_views_resolve: ") and "view (%d)" % view in msg, msg
    assert rt.lib.rt_views_resolve(views._h, 0, 2, None, None) == bad and "RT_FLAG_OUT_DEVICE" in rt.lib.rt_last_error().decode()
    assert list(views.samples()) == counts
    for v in range(3):
        assert _same(views.resolve(v), pictures[v])
    views.render(SLICE)                                               # and it carries on
    _check_views(scenes, name, names, w, h, views, [c + SLICE for c in counts])
    views.close()

"""Resumable renders (rt_accum_*): a frame advanced in any number of slices is bit for bit the frame of one rt_render call, floats
and bytes, and the picture after d samples is bit for bit rt_render(samples = d).  No tolerance anywhere: the slices make the same
additions in the same order and the factor (float)(1.0 / d) is applied once, at resolve."""
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def _same(a, b):
    """(floats, bytes) pairs equal bit for bit (NaN equal to NaN whatever its payload, as the existing frame comparisons have it)."""
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and np.array_equal(a[1], b[1])


def _sliced(scene, w, h, slices, **kw):
    acc = scene.accumulator(w, h, **kw)
    stats = [acc.render(n) for n in slices]
    assert acc.samples == sum(slices)
    out = acc.resolve()
    acc.close()
    return out, stats


def _slicings(n):
    return [[n], [n // 3, n // 3, n - 2 * (n // 3)], [1, n - 1], [n - 1, 1]]


def test_slicing_invariance_hw8(rt, sphere_scene):
    w, h, n = 96, 64, 48
    scene = rt.Scene(sphere_scene)
    one, one8, st1 = scene.render(w, h, n)
    results = []
    for slices in ([48], [16, 16, 16], [1, 47], [47, 1], [5, 7, 11, 25]):
        out, stats = _sliced(scene, w, h, slices)
        results.append(out)
        assert _same(out, (one, one8)), slices
        for st, k in zip(stats, slices):
            assert st.samples == w * h * k and st.reference_exact == st1.reference_exact == 1 and st.pipeline == st1.pipeline
            assert st.launches >= 1 and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    scene.close()
    ref, ref8, _ = oracle_lib.Hw8Oracle(sphere_scene).render(w, h, n)
    assert _same(results[4], (ref.astype(np.float32), ref8))


def test_every_preview_is_a_frame(rt, sphere_scene):
    w, h = 96, 64
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(w, h)
    d = 0
    for k in (4, 4, 8, 16):
        acc.render(k)
        d += k
        assert acc.samples == d
        first, second = acc.resolve(), acc.resolve()
        assert _same(first, second)
        frame = scene.render(w, h, d)[:2]
        assert _same(first, frame), d
    f_only, none8 = acc.resolve(want_rgb8=False)
    none_f, b_only = acc.resolve(want_float=False)
    assert none8 is None and none_f is None and _same((f_only, b_only), frame)
    acc.close()
    scene.close()


@pytest.mark.parametrize("name", ["hw7", "hw6"])
def test_slicing_invariance_hw7_and_hw6(rt, name):
    if name == "hw7":
        sd, w, h, n, kw = pin_cases.load_hw7("practice7_1"), 48, 48, 8, dict(integrator=rt.RT_INTEGRATOR_HW7)
    else:
        sd, w, h, n, kw = pin_cases.load_hw6("practice6_1"), 64, 48, 6, dict(integrator=rt.RT_INTEGRATOR_HW6)
    scene = rt.Scene(sd)
    one, one8, st1 = scene.render(w, h, n, **kw)
    assert st1.pipeline == rt.RT_PIPELINE_PERSISTENT
    for slices in _slicings(n) + [[1] * n]:
        out, stats = _sliced(scene, w, h, slices, **kw)
        assert _same(out, (one, one8)), slices
        assert all(st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.samples == w * h * k for st, k in zip(stats, slices))
    scene.close()


def test_environment_map(rt, sphere_scene):
    env = np.random.default_rng(5).integers(0, 255, (32, 64, 3)).astype(np.uint8)
    sd = rt.SceneData(sphere_scene.positions[-960:], sphere_scene.texcoords[-960:], sphere_scene.normals[-960:], sphere_scene.tangents[-960:],
                      np.zeros(960, np.uint32), [sphere_scene.materials[0]], camera=sphere_scene.camera, environment=env)
    scene = rt.Scene(sd)
    one = scene.render(64, 48, 8)[:2]
    assert one[0].mean() > 0.01
    out, _ = _sliced(scene, 64, 48, [3, 5])
    assert _same(out, one)
    scene.close()


@pytest.mark.parametrize("name", ["hw8", "hw6"])
def test_several_passes_and_phases(rt, monkeypatch, name):
    """RTAMD_PT_BLOCKS=14 makes the 400x300 frame take 2 passes (hw8) / 4 (hw6) over the SAME path records, RTAMD_PT_PHASE0=1 gives every
    slice of two samples or more a re-deal phase: a state kept per record instead of per pixel slot cannot pass this."""
    w, h, n = 400, 300, 4
    if name == "hw8":
        sd, kw, passes = pin_cases.random_triangle_scene(n=300, seed=12), {}, 2
    else:
        sd, kw, passes = pin_cases.hw6_soup(), dict(integrator=rt.RT_INTEGRATOR_HW6), 4
    scene = rt.Scene(sd)
    one, one8, st1 = scene.render(w, h, n, **kw)   # without the knobs: one launch
    assert st1.launches == 1
    monkeypatch.setenv("RTAMD_PT_BLOCKS", "14")
    monkeypatch.setenv("RTAMD_PT_PHASE0", "1")
    for slices in ([1, 3], [2, 2]):
        out, stats = _sliced(scene, w, h, slices, **kw)
        for st, k in zip(stats, slices):
            print(f"{name} slices {slices}: slice of {k}: {st.launches} launches")
            assert st.launches >= passes
            assert st.launches == (2 * passes if k > 1 else passes)   # a slice of one sample has nothing to re-deal
        assert _same(out, (one, one8)), slices
    scene.close()


def test_round_pipeline_and_megakernel(rt, sphere_scene):
    w, h, n = 96, 64, 48
    try:
        os.environ["RTAMD_KERNEL"] = "wavefront"
        scene = rt.Scene(sphere_scene)
        one, one8, st1 = scene.render(w, h, n)
        assert st1.pipeline == rt.RT_PIPELINE_ROUNDS
        for slices in ([48], [16, 16, 16], [1, 47], [47, 1], [5, 7, 11, 25]):
            out, stats = _sliced(scene, w, h, slices)
            assert _same(out, (one, one8)), slices
            assert all(st.pipeline == rt.RT_PIPELINE_ROUNDS and st.reference_exact == st1.reference_exact for st in stats)
        os.environ["RTAMD_KERNEL"] = "mega"
        with pytest.raises(rt.RtError) as e:
            scene.accumulator(w, h)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "megakernel" in str(e.value)
        # an accumulator made under the default pipeline refuses a slice under the megakernel, and is none the worse for it
        os.environ.pop("RTAMD_KERNEL")
        acc = scene.accumulator(w, h)
        acc.render(8)
        os.environ["RTAMD_KERNEL"] = "mega"
        with pytest.raises(rt.RtError) as e:
            acc.render(8)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and acc.samples == 8
        os.environ.pop("RTAMD_KERNEL")
        acc.render(8)
        assert _same(acc.resolve(), scene.render(w, h, 16)[:2])
        acc.close()
        scene.close()
    finally:
        os.environ.pop("RTAMD_KERNEL", None)


def test_sharding(rt, sphere_scene):
    w, h, n = 96, 64, 12
    scene = rt.Scene(sphere_scene)
    one, one8, _ = scene.render(w, h, n)
    full, full8 = np.zeros_like(one), np.zeros_like(one8)
    for r in range(3):
        kw = dict(shard_index=r, shard_count=3, tile=32)
        (buf, buf8), _ = _sliced(scene, w, h, [5, 7], **kw)
        ref, ref8, _ = scene.render(w, h, n, **kw)
        assert _same((buf, buf8), (ref, ref8))   # the compact shard buffers themselves, padding included
        p = rt.make_params(w, h, n, **kw)
        full += rt.unshard(p, buf)
        full8 += rt.unshard(p, buf8)
    assert _same((full, full8), (one, one8))
    # a frame whose border tiles are padded: 100x70 in 32x32 tiles
    for r in range(3):
        kw = dict(shard_index=r, shard_count=3, tile=32)
        (buf, buf8), _ = _sliced(scene, 100, 70, [2, 2], **kw)
        assert _same((buf, buf8), scene.render(100, 70, 4, **kw)[:2])
    scene.close()


def test_isolation(rt, sphere_scene):
    w, h = 96, 64
    scene = rt.Scene(sphere_scene)
    a = scene.accumulator(w, h)
    b = scene.accumulator(80, 40, ray_depth=3)
    a.render(6)
    other = scene.render(50, 30, 5)[:2]
    b.render(4)
    a.render(10)
    assert _same(other, scene.render(50, 30, 5)[:2])
    b.render(3)
    assert _same(a.resolve(), scene.render(w, h, 16)[:2])
    assert _same(b.resolve(), scene.render(80, 40, 7, ray_depth=3)[:2])
    a.close()
    b.close()
    scene.close()


def test_checkpoint(rt):
    w, h = 96, 64
    sd = pin_cases.load_sphere()
    scene = rt.Scene(sd)
    want = scene.render(w, h, 48)[:2]
    acc = scene.accumulator(w, h)
    acc.render(16)
    blob = acc.save()
    assert len(blob) == rt.lib.rt_accum_state_bytes(acc.params) and blob[:4] == b"RTAC"
    assert int.from_bytes(blob[16:20], "little") == w and int.from_bytes(blob[20:24], "little") == h and int.from_bytes(blob[52:56], "little") == 16
    acc.close()
    scene.close()

    scene = rt.Scene(pin_cases.load_sphere())
    acc = scene.accumulator(w, h)
    acc.load(blob)
    assert acc.samples == 16
    acc.render(32)
    assert _same(acc.resolve(), want)
    assert acc.save()[128:] != blob[128:]
    # loading again goes back to the checkpoint
    acc.load(blob)
    assert acc.samples == 16 and acc.save() == blob

    def refused(other, field, data=blob):
        with pytest.raises(rt.RtError) as e:
            other.load(data)
        assert e.value.code == rt.RT_ERR_INVALID_ARG and field in str(e.value), str(e.value)
        assert other.samples == 0
        other.close()

    refused(scene.accumulator(w, h + 8), "height")
    refused(scene.accumulator(w + 8, h), "width")
    refused(scene.accumulator(w, h, integrator=rt.RT_INTEGRATOR_HW7), "integrator")
    refused(scene.accumulator(w, h, ray_depth=4), "ray depth")
    refused(scene.accumulator(w, h, shard_index=0, shard_count=2, tile=8), "shard count")
    refused(scene.accumulator(w, h), "truncated", blob[:-1])
    refused(scene.accumulator(w, h), "truncated", blob[:100])
    refused(scene.accumulator(w, h), "magic", b"XXXX" + blob[4:])
    acc.close()
    scene.close()
    # a scene with one triangle more
    pos = np.concatenate([sd.positions, sd.positions[:1] + np.float32(0.25)])
    more = rt.SceneData(pos, np.concatenate([sd.texcoords, sd.texcoords[:1]]), np.concatenate([sd.normals, sd.normals[:1]]),
                        np.concatenate([sd.tangents, sd.tangents[:1]]), np.concatenate([sd.material_index, sd.material_index[:1]]),
                        list(sd.materials)[:sd.n_materials], sd.texture_source, sd.images, camera=sd.camera, bg=sd.bg)
    scene = rt.Scene(more)
    refused(scene.accumulator(w, h), "triangle count")
    scene.close()


def test_limits_and_errors(rt, sphere_scene):
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(32, 16)
    for n in (0, -5):
        with pytest.raises(rt.RtError) as e:
            acc.render(n)
        assert e.value.code == rt.RT_ERR_INVALID_ARG
    with pytest.raises(rt.RtError) as e:
        acc.resolve()
    assert e.value.code == rt.RT_ERR_INVALID_ARG and acc.samples == 0
    with pytest.raises(rt.RtError) as e:
        scene.accumulator(32, 16, sample_streams=4)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and "throughput" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        scene.accumulator(32, 16, flags=rt.RT_FLAG_OUT_DEVICE)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    with pytest.raises(rt.RtError) as e:
        scene.accumulator(32, 16, integrator=rt.RT_INTEGRATOR_HW6)   # an hw8 scene
    assert e.value.code == rt.RT_ERR_INVALID_ARG
    import time
    t0 = time.time()
    with pytest.raises(rt.RtError) as e:
        acc.render(2 ** 25)
    assert e.value.code == rt.RT_ERR_LIMIT and time.time() - t0 < 1.0 and acc.samples == 0   # at once: nothing was launched
    acc.render(3)
    with pytest.raises(rt.RtError) as e:
        acc.render(2 ** 25 - 3)
    assert e.value.code == rt.RT_ERR_LIMIT and acc.samples == 3
    acc.render(2)
    assert _same(acc.resolve(), scene.render(32, 16, 5)[:2])   # the refusals left the state as it was
    acc.close()
    # counters are a slice's own
    acc = scene.accumulator(32, 16, flags=rt.RT_FLAG_COUNTERS)
    st = acc.render(4)
    ref = scene.render(32, 16, 4, counters=True)[2]
    assert st.closest_hit_queries == ref.closest_hit_queries > 0 and st.light_pdf_queries == ref.light_pdf_queries
    acc.close()
    scene.close()
    # the .txt integrators have no resumable state
    sd, w, h, spp, depth = rt.load_txt(os.path.join(SCENES, "txt", "hw2_sample.txt"), rt.RT_INTEGRATOR_HW2)
    scene = rt.Scene(sd)
    with pytest.raises(rt.RtError) as e:
        scene.accumulator(w, h, integrator=rt.RT_INTEGRATOR_HW2)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and "hw1 .. hw5" in str(e.value)
    scene.close()


@pytest.mark.parametrize("point_material", [3, 0])
def test_nan_frames(rt, point_material):
    """The degenerate-triangle scenes of test_gpu_edge_cases.py (zero-area triangles; with material 0 the point is emissive): whatever
    NaN / inf arithmetic they provoke goes through the state like any other float, NaN pixels in the same places."""
    sd0 = pin_cases.random_triangle_scene(n=120, seed=8)
    pos = sd0.positions.copy().reshape(-1, 3, 3)
    pos[5, 1] = pos[5, 0]            # two equal vertices
    pos[9] = pos[9, 0]               # a point
    pos[13, 2] = (pos[13, 0] + pos[13, 1]) / 2  # collinear
    mi = sd0.material_index.copy()
    mi[9] = point_material
    sd = rt.SceneData(pos.reshape(-1, 9), sd0.texcoords, sd0.normals, sd0.tangents, mi, list(sd0.materials)[:sd0.n_materials], camera=sd0.camera)
    scene = rt.Scene(sd)
    one, one8, _ = scene.render(48, 36, 6)
    (rgb, rgb8), _ = _sliced(scene, 48, 36, [2, 4])
    scene.close()
    print(f"degenerate scene, point material {point_material}: {int(np.isnan(one).any(axis=2).sum())} NaN pixels, {int(np.isinf(one).any(axis=2).sum())} inf pixels")
    assert np.array_equal(np.isnan(rgb), np.isnan(one))
    assert np.array_equal(rgb, one, equal_nan=True) and np.array_equal(rgb8, one8)


def test_nan_and_inf_sums_go_through_the_state(rt):
    """Sums that certainly are NaN / inf (a background with a NaN and an inf component behind two triangles, built as the `_scene` /
    `_mat` helpers of test_gpu_edge_cases.py build theirs): the state and the checkpoint carry them like any other float."""
    tris = np.asarray([[[-1, -1, 0], [1, -1, 0], [0, 1, 0]], [[-3, 3, -1], [3, 3, -1], [0, 3, 2]]], np.float32)
    n = len(tris)
    nrm = np.cross(tris[:, 0] - tris[:, 2], tris[:, 1] - tris[:, 2])
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    mats = []
    for emission in ((0, 0, 0), (4, 4, 3)):
        m = rt.rt_material()
        m.base_color, m.emission, m.metallic_factor, m.roughness_factor = (0.8, 0.8, 0.8), emission, 0.0, 0.6
        m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = m.normal_texture = -1
        mats.append(m)
    cam = rt.rt_camera()
    cam.position, cam.right, cam.up, cam.forward, cam.fov_y = (0, 0, 5), (1, 0, 0), (0, 1, 0), (0, 0, -1), 0.9
    sd = rt.SceneData(tris.reshape(n, 9), np.zeros((n, 6), np.float32), np.repeat(nrm[:, None, :], 3, axis=1).reshape(n, 9),
                      np.tile(np.array([1, 0, 0, 1], np.float32), (n, 3, 1)).reshape(n, 12), np.asarray([0, 1], np.uint32), mats, camera=cam,
                      bg=(float("nan"), float("inf"), 0.2))
    scene = rt.Scene(sd)
    one, one8, _ = scene.render(40, 24, 8)
    assert np.isnan(one).any() and np.isinf(one).any() and np.isfinite(one[..., 2]).all()
    acc = scene.accumulator(40, 24)
    acc.render(3)
    blob = acc.save()
    acc.close()
    acc = scene.accumulator(40, 24)
    acc.load(blob)
    acc.render(5)
    rgb, rgb8 = acc.resolve()
    acc.close()
    scene.close()
    assert np.array_equal(np.isnan(rgb), np.isnan(one))
    assert np.array_equal(rgb, one, equal_nan=True) and np.array_equal(rgb8, one8)

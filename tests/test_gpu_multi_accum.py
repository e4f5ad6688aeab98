"""Resumable renders on several devices (rt_multi_accum_*): a frame advanced in any slices on any number of device entries is bit for
bit the one-shot single-device frame, floats and bytes; every preview is the frame of that many samples; and the checkpoint is byte for
byte the unsharded single-device rt_accum's, so it moves between any numbers of devices and a plain Accumulator.  The device lists
repeat device 0 (as test_gpu_multi_device.py does): two physical GPUs are never involved.  No tolerance anywhere.

150x100 in 32x32 tiles is 5x4 tiles whose right and bottom ones hold whole padding sub-tiles (8x8 column 19, rows 13..15) next to
sub-tiles cut by the image edge (column 18, row 12): the smallest shape with all three kinds of sub-tile."""
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
W, H, SPP = 150, 100, 6


def _same(a, b):
    """(floats, bytes) pairs equal bit for bit (NaN equal to NaN whatever its payload, as the existing frame comparisons have it)."""
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def soup(rt):
    """The scene, one single-device Scene of it and its one-shot frames after d samples (rendered once per d, never changed)."""
    sd = pin_cases.random_triangle_scene(n=400, seed=33)
    scene = rt.Scene(sd)
    frames = {}

    def frame(d):
        if d not in frames:
            rgb, rgb8, st = scene.render(W, H, d)
            assert st.reference_exact == 1
            rgb.setflags(write=False)
            rgb8.setflags(write=False)
            frames[d] = (rgb, rgb8)
        return frames[d]

    yield sd, scene, frame
    scene.close()


@pytest.mark.parametrize("n_dev", [1, 2, 3, 5])
def test_slicing_invariance_and_previews(rt, soup, n_dev):
    sd, _, frame = soup
    multi = rt.MultiScene(sd, [0] * n_dev)
    for slices in ([6], [1, 5], [2, 2, 2]):
        acc = multi.accumulator(W, H)
        assert acc.samples == 0
        d = 0
        for n in slices:
            st = acc.render(n)
            d += n
            assert acc.samples == d and st.samples == W * H * n and st.reference_exact == 1, (slices, d)
            assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
            assert _same(acc.resolve(), frame(d)), (n_dev, slices, d)   # every preview is the frame of d samples
        assert d == SPP
        f_only, none8 = acc.resolve(want_rgb8=False)
        none_f, b_only = acc.resolve(want_float=False)
        assert none8 is None and none_f is None and _same((f_only, b_only), frame(SPP))
        acc.close()
    multi.close()


def test_blob_is_the_single_device_blob(rt, soup):
    sd, scene, _ = soup
    multi = rt.MultiScene(sd, [0, 0, 0])
    acc = multi.accumulator(W, H)
    acc.render(2)
    acc.render(4)
    blob = acc.save()
    one = scene.accumulator(W, H)
    one.render(3)
    one.render(3)
    want = one.save()
    one.close()
    slots = 19 * 13 * 64
    assert len(want) == 128 + 24 * slots == len(blob)
    assert blob[:128] == want[:128]                     # the header: 8x8 tiles, shard 0 of 1, ceil(W/8)*ceil(H/8)*64 slots
    hdr = np.frombuffer(blob[:128], np.uint32)
    assert list(hdr[4:6]) == [W, H] and list(hdr[8:14]) == [8, 8, 0, 1, slots, 6]
    assert blob[128:128 + 16 * slots] == want[128:128 + 16 * slots]   # {sum, engine}
    assert blob == want
    # saving reads only: the same bytes again, and the picture is still the frame
    assert acc.save() == blob
    acc.close()
    multi.close()


def test_checkpoint_moves_between_device_counts(rt, soup):
    sd, scene, frame = soup
    m3 = rt.MultiScene(sd, [0, 0, 0])
    a3 = m3.accumulator(W, H)
    a3.render(2)
    blob = a3.save()
    for n_dev in (5, 1):
        m = rt.MultiScene(sd, [0] * n_dev)
        a = m.accumulator(W, H)
        a.load(blob)
        assert a.samples == 2 and _same(a.resolve(), frame(2))
        assert a.save() == blob
        a.render(4)
        assert a.samples == 6 and _same(a.resolve(), frame(6)), n_dev
        a.close()
        m.close()
    plain = scene.accumulator(W, H)
    plain.load(blob)
    assert plain.samples == 2
    plain.render(4)
    assert _same(plain.resolve(), frame(6))
    plain.close()
    # the other way round: a plain Accumulator's blob into two devices
    plain = scene.accumulator(W, H)
    plain.render(2)
    blob1 = plain.save()
    plain.close()
    assert blob1 == blob
    m2 = rt.MultiScene(sd, [0, 0])
    a2 = m2.accumulator(W, H)
    a2.load(blob1)
    a2.render(4)
    assert _same(a2.resolve(), frame(6))
    # loading over a state that has moved on goes back to the checkpoint; the source was not disturbed by any of this
    a2.load(blob)
    assert a2.samples == 2 and a2.save() == blob
    a2.close()
    m2.close()
    a3.render(4)
    assert _same(a3.resolve(), frame(6))
    a3.close()
    m3.close()


def test_more_devices_than_tiles(rt, sphere_scene):
    w, h = 40, 33   # 2x2 tiles of 32 on six entries: two shards are empty
    multi = rt.MultiScene(sphere_scene, [0] * 6)
    acc = multi.accumulator(w, h)
    st1 = acc.render(1)
    st3 = acc.render(3)
    assert st1.samples == w * h and st3.samples == 3 * w * h and st3.reference_exact == 1 and st3.pipeline == rt.RT_PIPELINE_PERSISTENT
    out = acc.resolve()
    ref, ref8, _ = oracle_lib.Hw8Oracle(sphere_scene).render(w, h, 4)
    assert _same(out, (ref.astype(np.float32), ref8))
    blob = acc.save()
    assert len(blob) == 128 + 24 * 5 * 5 * 64
    other = multi.accumulator(w, h)
    other.load(blob)
    assert other.samples == 4 and other.save() == blob and _same(other.resolve(), out)
    other.close()
    acc.close()
    multi.close()


@pytest.mark.parametrize("name", ["hw6", "hw7"])
def test_hw6_and_hw7(rt, name):
    if name == "hw7":
        sd, w, h, n_dev, slices, kw = pin_cases.load_hw7("practice7_1"), 48, 48, 2, [3, 5], dict(integrator=rt.RT_INTEGRATOR_HW7)
    else:
        sd, w, h, n_dev, slices, kw = pin_cases.load_hw6("practice6_1"), 64, 48, 3, [2, 4], dict(integrator=rt.RT_INTEGRATOR_HW6)
    scene = rt.Scene(sd)
    one = scene.render(w, h, sum(slices), **kw)[:2]
    scene.close()
    multi = rt.MultiScene(sd, [0] * n_dev)
    acc = multi.accumulator(w, h, **kw)
    for n in slices:
        st = acc.render(n)
        assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.samples == w * h * n
    assert _same(acc.resolve(), one)
    acc.close()
    multi.close()


def test_refusals(rt, soup):
    sd, scene, frame = soup
    multi = rt.MultiScene(sd, [0, 0, 0])
    with pytest.raises(rt.RtError) as e:
        multi.accumulator(W, H, sample_streams=4)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and "throughput" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        multi.accumulator(W, H, flags=rt.RT_FLAG_OUT_DEVICE)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    with pytest.raises(rt.RtError) as e:
        multi.accumulator(W, H, shard_index=0, shard_count=2)
    assert e.value.code == rt.RT_ERR_INVALID_ARG and "shard_count" in str(e.value)

    acc = multi.accumulator(W, H)
    with pytest.raises(rt.RtError) as e:
        acc.resolve()                                   # no samples yet
    assert e.value.code == rt.RT_ERR_INVALID_ARG and acc.samples == 0
    for n in (0, -5):
        with pytest.raises(rt.RtError) as e:
            acc.render(n)
        assert e.value.code == rt.RT_ERR_INVALID_ARG
    acc.render(2)
    blob = acc.save()
    # a blob of another width, a truncated one, a damaged one: rejected with the field's name, the state as it was
    wide = multi.accumulator(W + 8, H)
    wide.render(1)
    other = wide.save()
    wide.close()
    for data, field in ((other, "width"), (blob[:-1], "truncated"), (blob[:100], "truncated"), (b"XXXX" + blob[4:], "magic")):
        with pytest.raises(rt.RtError) as e:
            acc.load(data)
        assert e.value.code == rt.RT_ERR_INVALID_ARG and field in str(e.value), str(e.value)
        assert acc.samples == 2
    assert _same(acc.resolve(), frame(2))
    # a shard's own checkpoint is not the frame's
    part = scene.accumulator(W, H, shard_index=1, shard_count=3, tile=32)
    with pytest.raises(rt.RtError) as e:
        acc.load(part.save())
    assert e.value.code == rt.RT_ERR_INVALID_ARG and "tile width" in str(e.value)
    part.close()
    # a slice across the sample index limit: refused at once, before any device launches; the object renders and resolves afterwards
    with pytest.raises(rt.RtError) as e:
        acc.render(2 ** 25 - 2)
    assert e.value.code == rt.RT_ERR_LIMIT and acc.samples == 2
    assert _same(acc.resolve(), frame(2))
    acc.render(4)
    assert _same(acc.resolve(), frame(6))
    acc.close()
    multi.close()
    # the .txt integrators have no resumable state
    sdt, w, h, spp, depth = rt.load_txt(os.path.join(SCENES, "txt", "hw3_practice3_5_64x48x8.txt"), rt.RT_INTEGRATOR_HW3)
    multi = rt.MultiScene(sdt, [0, 0])
    with pytest.raises(rt.RtError) as e:
        multi.accumulator(w, h, integrator=rt.RT_INTEGRATOR_HW3)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and "hw1 .. hw5" in str(e.value)
    multi.close()


def test_isolation_from_rt_multi_render_and_other_accumulators(rt, soup):
    sd, _, frame = soup
    multi = rt.MultiScene(sd, [0, 0, 0])
    a = multi.accumulator(W, H)
    b = multi.accumulator(80, 40, ray_depth=3)
    a.render(2)
    b.render(3)
    between = multi.render(W, H, 2)[:2]               # uses the same shard buffers and landing areas on every device
    assert _same(between, frame(2))
    small = multi.render(50, 30, 5)[:2]
    a.render(4)
    b.render(4)
    assert _same(a.resolve(), frame(6))
    assert _same(small, multi.render(50, 30, 5)[:2])
    scene = rt.Scene(sd)
    assert _same(b.resolve(), scene.render(80, 40, 7, ray_depth=3)[:2])
    scene.close()
    assert _same(a.resolve(), frame(6))
    multi.close()                                     # closes its accumulators first
    assert not a._h and not b._h

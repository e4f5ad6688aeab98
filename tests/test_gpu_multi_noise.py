"""Noise monitor on several device entries (rt_multi_noise_*): the map and EVERY field of the summary, doubles included, equal the
unsharded single-device monitor's of the same slicing with ==: each sub-tile is summed by one wave in the same order wherever it lies,
and the host adds the sub-tiles in the frame's order.  The device lists repeat device 0, as the other multi tests do it.

150x100 in 32x32 tiles has whole padding sub-tiles next to sub-tiles cut by the image edge; 40x33 on six entries leaves two shards empty."""
import numpy as np
import pytest

import pin_cases

pytestmark = pytest.mark.gpu
SLICES = [2, 4, 6]
FIELDS = ("batches", "samples_observed", "samples_total", "pixels", "nonfinite_pixels", "mean_luminance", "rms_error", "noise", "worst_tile_noise")


@pytest.fixture(scope="module")
def soup(rt):
    sd = pin_cases.random_triangle_scene(n=400, seed=33)
    scene = rt.Scene(sd)
    yield sd, scene
    scene.close()


def _single(scene, w, h):
    """The unsharded single-device monitor after every slice from the second on: [(map, summary)]."""
    acc = scene.accumulator(w, h)
    mon = acc.noise_monitor()
    out = []
    for n in SLICES:
        acc.render(n)
        mon.update()
        if mon.batches >= 2:
            out.append(mon.estimate())
    acc.close()
    return out


@pytest.mark.parametrize("w,h,devices", [(150, 100, [0, 0, 0]), (40, 33, [0] * 6)], ids=["150x100 on 3", "40x33 on 6"])
def test_equals_the_unsharded_monitor_in_every_field(rt, soup, w, h, devices):
    sd, scene = soup
    want = _single(scene, w, h)
    multi = rt.MultiScene(sd, devices)
    acc = multi.accumulator(w, h)
    mon = acc.noise_monitor()
    assert isinstance(mon, rt.MultiNoiseMonitor) and mon.batches == 0
    got = []
    for n in SLICES:
        acc.render(n)
        mon.update()
        if mon.batches >= 2:
            got.append(mon.estimate())
    assert len(got) == len(want) == 2
    for (se, s), (se1, s1) in zip(got, want):
        assert se.shape == (h, w) and np.array_equal(se, se1)
        for f in FIELDS:
            assert getattr(s, f) == getattr(s1, f), (f, getattr(s, f), getattr(s1, f))
        assert s.pixels == w * h and s.nonfinite_pixels == 0 and s.noise > 0
    none, s = mon.estimate(want_map=False)
    assert none is None and s.noise == want[-1][1].noise
    multi.close()   # closes the accumulator and with it the monitor
    assert not mon._h


def test_errors_and_load(rt, soup):
    sd, scene = soup
    w, h = 40, 33
    multi = rt.MultiScene(sd, [0, 0, 0])
    acc = multi.accumulator(w, h)
    mon = acc.noise_monitor()

    def refused(call, word):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID_ARG and word in str(e.value), str(e.value)

    refused(mon.update, "no samples")
    refused(mon.estimate, "0 batches")
    acc.render(2)
    mon.update()
    refused(mon.estimate, "1 batches")
    blob = acc.save()
    acc.render(2)
    mon.update()
    mon.estimate()
    acc.load(blob)
    refused(mon.update, "rt_multi_accum_load")
    refused(mon.estimate, "rt_multi_accum_load")
    acc.render(3)
    refused(mon.update, "rt_multi_accum_load")
    mon.reset()
    assert mon.batches == 0
    for n in (1, 2):
        acc.render(n)
        mon.update()
    se, s = mon.estimate()
    assert s.batches == 2 and s.samples_observed == 3 and s.samples_total == 8
    # the same through a plain accumulator that loads the frame's portable checkpoint at the same point
    one = scene.accumulator(w, h)
    one.load(blob)
    one.render(3)
    mon1 = one.noise_monitor()
    for n in (1, 2):
        one.render(n)
        mon1.update()
    se1, s1 = mon1.estimate()
    assert np.array_equal(se, se1) and all(getattr(s, f) == getattr(s1, f) for f in FIELDS)
    one.close()
    import ctypes as C
    summary = rt.rt_noise_summary()
    summary.struct_size = C.sizeof(rt.rt_noise_summary)
    assert rt.lib.rt_multi_noise_estimate(mon._h, rt.RT_FLAG_OUT_DEVICE, None, C.byref(summary)) == rt.RT_ERR_INVALID_ARG
    assert rt.lib.rt_last_error().startswith(b"rt_multi_noise_estimate: flags")
    multi.close()

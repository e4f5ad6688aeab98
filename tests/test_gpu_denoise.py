"""The preview filter on the GPU.  rt_denoise against tests/denoise_model.py, bit for bit in floats and bytes, on synthetic planes that
hold everything the filter tells apart; rt_accum_denoise against its definition, the composition of the public calls; and the refusals
that need a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
import pin_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def synthetic(h, w, seed=5):
    """Random rgb, two normal regions with a little scatter, a depth ramp with a step, and -- where the frame has room -- a block of
    misses, a block with emission, one NaN pixel, one infinite se and one infinite depth; albedo down to below its floor."""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    nrm = np.where((np.arange(w) < w // 2)[None, :, None], np.array([0, 0, 1], F), np.array([0.6, 0, 0.8], F)) + rng.normal(0, 0.05, (h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
    z = (F(2) + F(0.03) * np.arange(w, dtype=F)[None, :] + F(0.01) * np.arange(h, dtype=F)[:, None]).astype(F)
    z[:, (2 * w) // 3:] += F(1.5)
    alb = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
    alb[rng.uniform(size=(h, w)) < 0.05] = F(0.001)
    em = np.zeros((h, w, 3), F)
    se = rng.uniform(0.0, 0.4, (h, w)).astype(F)
    if h >= 16 and w >= 16:
        z[2:6, 3:8] = 0
        em[9:12, 10:14, 0] = 3
        rgb[7, 1, 1] = np.nan
        se[13, 4] = np.inf
        z[14, 9] = np.inf
    return dict(rgb=rgb, normal=nrm, depth=z, albedo=alb, emission=em, se=se)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def scene(rt, sphere_scene):
    s = rt.Scene(sphere_scene)
    yield s
    s.close()


@pytest.mark.parametrize("iterations", [1, 3, 5, 7])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (36, 20), (70, 33)])
def test_kernel_is_the_model_bit_for_bit(scene, w, h, iterations):
    pl = synthetic(h, w)
    for with_se in (False, True):
        for with_albedo in (False, True):
            kw = dict(emission=pl["emission"], se=pl["se"] if with_se else None, albedo=pl["albedo"] if with_albedo else None)
            want, want8, want_fixed = dm.denoise(pl["rgb"], pl["normal"], pl["depth"], iterations=iterations, **kw)
            got, got8, st = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], iterations=iterations, **kw)
            diff = np.argwhere(bits(got) != bits(want))
            assert same_bits(got, want), (with_se, with_albedo, len(diff), diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])
            assert np.array_equal(got8, want8), (with_se, with_albedo, np.argwhere(got8 != want8)[:5])
            assert st.fixed_pixels == want_fixed and st.launches == 1 + iterations and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
            if h >= 16:
                assert want_fixed == 20 + 12 + 2 + (1 if with_se else 0) and not same_bits(got, pl["rgb"])
    # other sigmas, and the defaults by name
    kw = dict(emission=pl["emission"], se=pl["se"], albedo=pl["albedo"], iterations=iterations)
    want, want8, _ = dm.denoise(pl["rgb"], pl["normal"], pl["depth"], sigma_depth=0.25, sigma_luminance=1.5, **kw)
    got, got8, _ = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], sigma_depth=0.25, sigma_luminance=1.5, **kw)
    assert same_bits(got, want) and np.array_equal(got8, want8)


def test_defaults_are_five_levels_and_sigmas_one_and_four(scene):
    pl = synthetic(20, 36)
    a = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], se=pl["se"])
    b = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], se=pl["se"], iterations=5, sigma_depth=1.0, sigma_luminance=4.0)
    assert a[2].launches == 6 and same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    only8 = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], se=pl["se"], want_float=False)
    onlyf = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], se=pl["se"], want_rgb8=False)
    assert only8[0] is None and onlyf[1] is None and np.array_equal(only8[1], a[1]) and same_bits(onlyf[0], a[0])


def test_a_frame_of_misses_comes_out_as_it_went_in(scene):
    """All depth zero: the floats are the input's bits and the bytes are rt_accum_resolve's for those floats."""
    w, h = 36, 20
    acc = scene.accumulator(w, h)
    acc.render(3)
    rgb, rgb8 = acc.resolve()
    acc.close()
    zero3, zero = np.zeros((h, w, 3), F), np.zeros((h, w), F)
    out, out8, st = scene.denoise(rgb, zero3, zero, iterations=5)
    assert same_bits(out, rgb) and np.array_equal(out8, rgb8) and st.fixed_pixels == w * h and rgb8.max() > 0


def test_aliased_output_and_a_second_call_give_the_same_bits(rt, scene):
    pl = synthetic(33, 70)
    want, want8, _ = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], albedo=pl["albedo"], emission=pl["emission"], se=pl["se"])
    again, again8, _ = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], albedo=pl["albedo"], emission=pl["emission"], se=pl["se"])
    assert same_bits(again, want) and np.array_equal(again8, want8)
    inout = pl["rgb"].copy()
    p = rt.make_denoise_params(70, 33)
    ptr = lambda k: pl[k].ctypes.data
    assert rt.lib.rt_denoise(scene._h, C.byref(p), inout.ctypes.data, ptr("normal"), ptr("depth"), ptr("albedo"), ptr("emission"), ptr("se"),
                             inout.ctypes.data, None, None) == 0, rt.lib.rt_last_error()
    assert same_bits(inout, want)


DEVICE_POINTERS = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import pin_cases
import test_gpu_denoise as t
scene = rt.Scene(pin_cases.load_sphere())
h, w = 33, 70
pl = t.synthetic(h, w)
want, want8, st = scene.denoise(pl["rgb"], pl["normal"], pl["depth"], albedo=pl["albedo"], emission=pl["emission"], se=pl["se"])
dev = {{k: torch.from_numpy(v).cuda() for k, v in pl.items()}}
out = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
out8 = torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ptrs = [dev[k].data_ptr() for k in ("rgb", "normal", "depth", "albedo", "emission", "se")]
st_d = scene.denoise_device(w, h, *ptrs, out_rgb_ptr=out.data_ptr(), out_rgb8_ptr=out8.data_ptr())
assert st_d.fixed_pixels == st.fixed_pixels and st_d.launches == st.launches
assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(out8.cpu().numpy(), want8)
for k in pl:   # the planes are only read
    assert np.array_equal(dev[k].cpu().numpy().view(np.uint32), pl[k].view(np.uint32)), k
scene.denoise_device(w, h, *ptrs, out_rgb_ptr=dev["rgb"].data_ptr())   # in place
assert np.array_equal(dev["rgb"].cpu().numpy().view(np.uint32), want.view(np.uint32))
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bits():
    """RT_DENOISE_DEVICE_POINTERS with torch tensors as planes, separate and in place.  In a process of its own, where torch opens the
    GPU before the library does."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


def summary_fields(s):
    return tuple(getattr(s, f[0]) for f in s._fields_)


def check_composition(rt, scene, w, h, slices, some_fixed=True, **kw):
    """After every slice from the second on: Accumulator.denoise equals Scene.denoise of what resolve, render_guides and estimate return."""
    guides, _ = scene.render_guides(w, h)
    acc = scene.accumulator(w, h, **kw)
    mon = acc.noise_monitor()
    for k, n in enumerate(slices):
        acc.render(n)
        mon.update()
        if k == 0:
            continue
        blob, (_, before) = acc.save(), mon.estimate(want_map=False)
        rgb, _ = acc.resolve()
        se, _ = mon.estimate()
        for monitor, albedo in ((mon, False), (mon, True), (None, False)):
            got, got8, st = acc.denoise(monitor=monitor, albedo=albedo)
            want, want8, st_w = scene.denoise(rgb, guides["normal"], guides["depth"], albedo=guides["albedo"] if albedo else None,
                                              emission=guides["emission"], se=se if monitor is not None else None)
            assert same_bits(got, want) and np.array_equal(got8, want8), (k, monitor is not None, albedo)
            assert st.fixed_pixels == st_w.fixed_pixels and st.launches == 6
            assert (0 < st.fixed_pixels < w * h or not some_fixed) and not same_bits(got, rgb)
        assert acc.save() == blob and summary_fields(mon.estimate(want_map=False)[1]) == summary_fields(before)
    d = sum(slices)
    assert acc.samples == d
    rgb, rgb8 = acc.resolve()
    one, one8, _ = scene.render(w, h, d, **kw)
    assert same_bits(rgb, one) and np.array_equal(rgb8, one8)
    acc.close()


def test_accum_denoise_is_the_composition_of_the_public_calls(rt, scene):
    check_composition(rt, scene, 36, 20, (3, 5, 8))


def test_accum_denoise_on_an_hw7_frame(rt):
    s = rt.Scene(pin_cases.load_hw7("practice7_1"))
    check_composition(rt, s, 36, 20, (2, 2), some_fixed=False, integrator=rt.RT_INTEGRATOR_HW7)
    s.close()


def test_accum_denoise_takes_parameters_and_checks_the_size(rt, scene):
    w, h = 36, 20
    acc = scene.accumulator(w, h)
    acc.render(2)
    got, _, st = acc.denoise(iterations=2, sigma_depth=0.5)
    guides, _ = scene.render_guides(w, h)
    want, _, _ = scene.denoise(acc.resolve()[0], guides["normal"], guides["depth"], emission=guides["emission"], iterations=2, sigma_depth=0.5)
    assert same_bits(got, want) and st.launches == 3
    p = rt.make_denoise_params(w, h)
    out = np.zeros((h, w, 3), F)
    assert rt.lib.rt_accum_denoise(acc._h, None, C.byref(p), out.ctypes.data, None, None) == 0   # the accumulator's own size is fine
    p = rt.make_denoise_params(w, 0)
    assert rt.lib.rt_accum_denoise(acc._h, None, C.byref(p), out.ctypes.data, None, None) == 0   # 0 = the accumulator's, per field
    for bad in ((w + 1, h), (w, h - 1), (0, h + 1), (-w, h)):
        p = rt.make_denoise_params(*bad)
        assert rt.lib.rt_accum_denoise(acc._h, None, C.byref(p), out.ctypes.data, None, None) == rt.RT_ERR_INVALID_ARG
        assert b"width and height must be 0 or the accumulator's" in rt.lib.rt_last_error()
    acc.close()


def test_refusals_that_need_a_device(rt, scene):
    w, h = 36, 20

    def refused(acc, code, text, monitor=None):
        with pytest.raises(rt.RtError) as e:
            acc.denoise(monitor=monitor)
        assert e.value.code == code and "rt_accum_denoise: " in str(e.value) and text in str(e.value), str(e.value)

    acc = scene.accumulator(w, h)
    refused(acc, rt.RT_ERR_INVALID_ARG, "no samples yet")
    acc.render(2)
    mon = acc.noise_monitor()
    refused(acc, rt.RT_ERR_INVALID_ARG, "0 batches", mon)
    acc.render(1)
    mon.update()
    refused(acc, rt.RT_ERR_INVALID_ARG, "1 batches", mon)
    other = scene.accumulator(w, h)
    other.render(1)
    foreign = other.noise_monitor()
    for _ in range(2):
        other.render(1)
        foreign.update()
    refused(acc, rt.RT_ERR_INVALID_ARG, "another accumulator", foreign)
    blob = acc.save()
    acc.load(blob)                      # a load ends the batches: the monitor's map no longer belongs to the state
    acc.render(1)
    refused(acc, rt.RT_ERR_INVALID_ARG, "rt_noise_reset", mon)
    acc.denoise()                       # and none of the refusals has broken anything
    sharded = scene.accumulator(w, h, shard_index=0, shard_count=2, tile=8)
    sharded.render(1)
    refused(sharded, rt.RT_ERR_UNSUPPORTED, "sharded")
    for a in (acc, other, sharded):
        a.close()
    s6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    acc6 = s6.accumulator(w, h, integrator=rt.RT_INTEGRATOR_HW6)
    acc6.render(1)
    refused(acc6, rt.RT_ERR_UNSUPPORTED, "hw8 / hw7")
    # rt_denoise itself is an image filter: any scene will do
    pl = synthetic(h, w)
    got, _, _ = s6.denoise(pl["rgb"], pl["normal"], pl["depth"])
    assert same_bits(got, dm.denoise(pl["rgb"], pl["normal"], pl["depth"])[0])
    s6.close()

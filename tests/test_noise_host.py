"""Noise monitor, host side (no GPU): rt_noise_* / rt_multi_noise_* are declared, exported and bound; null handles and a wrong
struct_size are errors, not crashes; and the estimator itself (tests/noise_model.py, the numpy restatement of the kernels' arithmetic)
is unbiased on streams whose variance is known."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noise_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = ["rt_noise_create", "rt_noise_update", "rt_noise_reset", "rt_noise_batches", "rt_noise_estimate", "rt_noise_destroy",
         "rt_multi_noise_create", "rt_multi_noise_update", "rt_multi_noise_reset", "rt_multi_noise_batches", "rt_multi_noise_estimate",
         "rt_multi_noise_destroy"]
RT_ERR_INVALID_ARG = -1


def test_noise_symbols_are_declared_exported_and_bound(rt):
    header = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s*(rt_(?:multi_)?noise_[a-z0-9_]+)\(", header, re.M))
    assert declared == set(NOISE)
    for name in NOISE:
        assert name in rt.ABI_SYMBOLS and hasattr(rt.lib, name), name
    assert "typedef struct rt_noise_summary {" in header
    assert rt.lib.rt_abi_version() == 6 and "#define RTAMD_ABI_VERSION 6" in header
    assert C.sizeof(rt.rt_render_params) == 64 and C.sizeof(rt.rt_stats) == 96
    # the ctypes mirror of the struct: 4 + 3 * 4 + 2 * 8 + 4 * 8 bytes, fields in the header's order
    fields = re.search(r"typedef struct rt_noise_summary \{(.*?)\} rt_noise_summary;", header, re.S).group(1)
    names = re.findall(r"^\s*(?:uint32_t|int32_t|uint64_t|double)\s+([a-z_]+);", fields, re.M)
    assert names == [f[0] for f in rt.rt_noise_summary._fields_] and C.sizeof(rt.rt_noise_summary) == 64
    for cls, acc in ((rt.NoiseMonitor, rt.Accumulator), (rt.MultiNoiseMonitor, rt.MultiAccumulator)):
        for method in ("update", "reset", "estimate", "close"):
            assert callable(getattr(cls, method))
        assert isinstance(cls.batches, property) and callable(acc.noise_monitor)


@pytest.mark.parametrize("family", ["rt_noise", "rt_multi_noise"])
def test_null_handles_and_struct_size_are_invalid_arguments(rt, family):
    fn = lambda name: getattr(rt.lib, family + name)
    msg = lambda: rt.lib.rt_last_error()
    out = C.c_void_p()
    summary = rt.rt_noise_summary()
    summary.struct_size = C.sizeof(rt.rt_noise_summary)
    assert fn("_create")(None, C.byref(out)) == RT_ERR_INVALID_ARG and not out
    assert msg().startswith(family.encode() + b"_create:")
    for name in ("_update", "_reset", "_batches"):
        assert fn(name)(None) == RT_ERR_INVALID_ARG
        assert msg().startswith(family.encode() + name.encode() + b":"), msg()
    assert fn("_estimate")(None, 0, None, C.byref(summary)) == RT_ERR_INVALID_ARG
    assert msg().startswith(family.encode() + b"_estimate:")
    assert fn("_estimate")(None, 0, None, None) == RT_ERR_INVALID_ARG
    fn("_destroy")(None)  # like free(NULL)


@pytest.mark.parametrize("family", ["rt_noise", "rt_multi_noise"])
def test_wrong_struct_size_is_an_invalid_argument(rt, family):
    """The summary's struct_size is looked at before anything else, so ABI skew is reported whatever the handle is."""
    estimate = getattr(rt.lib, family + "_estimate")
    for size in (0, 56, 72):
        summary = rt.rt_noise_summary()
        summary.struct_size = size
        rt.lib.rt_load_gltf(b"/nonexistent.gltf", 8, C.byref(C.c_void_p()))  # leaves some other message behind
        assert estimate(None, 0, None, C.byref(summary)) == RT_ERR_INVALID_ARG
        msg = rt.lib.rt_last_error()
        assert msg.startswith(family.encode() + b"_estimate:") and b"struct_size" in msg, msg
    summary.struct_size = C.sizeof(rt.rt_noise_summary)
    assert estimate(None, 0, None, C.byref(summary)) == RT_ERR_INVALID_ARG and b"null argument" in rt.lib.rt_last_error()


SLICINGS = [[8] * 8, [16] * 4, [1, 3, 5, 7, 9, 39]]


@pytest.mark.parametrize("slices", SLICINGS, ids=lambda s: "-".join(map(str, s)))
def test_model_is_unbiased_on_normal_streams(slices):
    """4,096 pixels of i.i.d. normal samples with one sigma, accumulated in float32 like the renderer's sums: the mean over the pixels of
    se^2 is sigma^2 / d within six standard deviations of a scaled chi-square mean, 6 * sqrt(2 / ((B - 1) * 4096)), relatively."""
    rng = np.random.default_rng(17)
    pixels, sigma, mean, d = 4096, 0.75, 2.0, sum(slices)
    assert d == 64
    samples = rng.normal(mean, sigma, (d, 64, 64, 3)).astype(np.float32)
    samples[..., 1] = samples[..., 0]
    samples[..., 2] = samples[..., 0]   # grey: Y of a sample is the sample, up to the weights' rounding (they add up to 1)
    sums = np.zeros((64, 64, 3), np.float32)
    mon = noise_model.Monitor(sums, 0)
    done = 0
    for n in slices:
        for k in range(done, done + n):
            sums = sums + samples[k]
        done += n
        mon.update(sums, done)
    se, se2, lum, finite = mon.estimate()
    assert finite.all() and se.dtype == np.float32 and mon.batches == len(slices) and mon.observed == d
    ratio = float(se2.astype(np.float64).mean()) / (sigma ** 2 / d)
    bound = 6 * np.sqrt(2 / ((len(slices) - 1) * pixels))
    print(f"slicing {slices}: mean se^2 / (sigma^2 / d) = {ratio:.4f}, bound +-{bound:.4f}")
    assert abs(ratio - 1) <= bound
    s = mon.summary()
    assert s["pixels"] == pixels and s["nonfinite_pixels"] == 0 and abs(s["mean_luminance"] - mean) < 0.01
    assert abs(s["rms_error"] ** 2 / (sigma ** 2 / d) - 1) <= bound


def test_model_late_start_and_unequal_batches_agree_with_plain_variance():
    """West's update against the textbook weighted variance of the batch means in float64, on a monitor attached after 10 samples."""
    rng = np.random.default_rng(3)
    slices = [2, 7, 1, 12, 5]
    samples = rng.gamma(2.0, 1.0, (10 + sum(slices), 16, 16, 3)).astype(np.float32)
    sums = samples[:10].sum(axis=0, dtype=np.float32)
    mon = noise_model.Monitor(sums, 10)
    done, means = 10, []
    for n in slices:
        before = noise_model.luminance(sums).astype(np.float64)
        for k in range(done, done + n):
            sums = sums + samples[k]
        done += n
        mon.update(sums, done)
        means.append((noise_model.luminance(sums).astype(np.float64) - before) / n)
    w = np.asarray(slices, np.float64)[:, None, None]
    means = np.asarray(means)
    grand = (w * means).sum(axis=0) / w.sum()
    m2 = (w * (means - grand) ** 2).sum(axis=0)
    assert mon.samples == done and mon.observed == sum(slices)
    assert np.allclose(mon.m2, m2, rtol=2e-3, atol=1e-6)   # float32 sums of ~40 against float64: differences of sums lose a few digits
    se, se2, _, _ = mon.estimate()
    assert np.allclose(se2, m2 / (len(slices) - 1) / done, rtol=2e-3, atol=1e-8)


def test_constant_stream_has_no_noise():
    sums = np.zeros((16, 24, 3), np.float32)
    mon = noise_model.Monitor(sums, 0)
    done = 0
    for n in (4, 4, 8, 16):
        done += n
        mon.update(np.full((16, 24, 3), 0.5 * done, np.float32), done)   # 0.5 per sample: every partial sum is exact
    se, se2, lum, finite = mon.estimate()
    assert finite.all() and not mon.m2.any() and not se.any()
    s = mon.summary()
    assert s["noise"] == 0 and s["rms_error"] == 0 and s["worst_tile_noise"] == 0 and s["pixels"] == 16 * 24
    assert abs(s["mean_luminance"] - 0.5) < 1e-6


def test_nonfinite_pixels_are_counted_and_left_out():
    rng = np.random.default_rng(1)
    samples = rng.random((12, 8, 16, 3)).astype(np.float32)
    samples[:, 2, 3, 0] = np.nan
    samples[5, 4, 9, 1] = np.inf
    sums = np.zeros((8, 16, 3), np.float32)
    mon = noise_model.Monitor(sums, 0)
    for k in range(0, 12, 4):
        sums = sums + samples[k:k + 4].sum(axis=0, dtype=np.float32)
        mon.update(sums, k + 4)
    se, _, _, finite = mon.estimate()
    assert not finite[2, 3] and not finite[4, 9] and finite.sum() == 8 * 16 - 2
    assert not np.isfinite(se[2, 3]) and not np.isfinite(se[4, 9])
    s = mon.summary()
    assert s["pixels"] == 8 * 16 - 2 and s["nonfinite_pixels"] == 2
    assert all(np.isfinite(s[k]) for k in ("mean_luminance", "rms_error", "noise", "worst_tile_noise")) and s["noise"] > 0

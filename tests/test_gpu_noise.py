"""Noise monitor of a resumable render (rt_noise_*): the per-pixel standard error is bit for bit what tests/noise_model.py computes from
the checkpoints' sums, the figures of the frame agree with the model's float64 sums to the rounding of a 64-term float32 sum, the
monitor only reads the accumulator, and every refusal is an RT_ERR_INVALID_ARG that leaves the statistics as they were."""
import ctypes as C

import numpy as np
import pytest

import noise_model
import pin_cases

pytestmark = pytest.mark.gpu
TILE_SUM = 64 * 2.0 ** -24   # worst case of adding 64 non-negative float32 terms in any order, relative; the rest is float64 on both sides
INT_FIELDS = ("batches", "samples_observed", "samples_total", "pixels", "nonfinite_pixels")
DOUBLE_FIELDS = ("mean_luminance", "rms_error", "noise", "worst_tile_noise")


def _same_map(a, b):
    """Bit for bit, a NaN equal to a NaN whatever its payload."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def _check_summary(got, want, what=""):
    for f in INT_FIELDS:
        assert getattr(got, f) == want[f], (what, f, getattr(got, f), want[f])
    for f in DOUBLE_FIELDS:
        g, w = getattr(got, f), want[f]
        print(f"{what} {f}: kernel {g!r} model {w!r} relative difference {abs(g - w) / abs(w) if w else abs(g):.3e} (bound {TILE_SUM:.3e})")
        assert np.isfinite(g) and abs(g - w) <= TILE_SUM * abs(w), (what, f, g, w)


def _watch(acc, mon, model, w, h, slices, what=""):
    """Advance `acc` by the slices, the monitor and the model side by side; after every slice from the second on map and summary agree."""
    for n in slices:
        acc.render(n)
        mon.update()
        model.update(noise_model.blob_sums(acc.save(), w, h), acc.samples)
        assert mon.batches == model.batches
        if mon.batches >= 2:
            se, s = mon.estimate()
            want, _, _, _ = model.estimate()
            assert se.dtype == np.float32 and _same_map(se, want), (what, n, int((se != want).sum()))
            _check_summary(s, model.summary(), f"{what} after {acc.samples} samples:")
    return se, s


CASES = {
    "hw8": (pin_cases.load_sphere, 36, 20, [3, 5, 8, 16], {}, None),     # border sub-tiles, 960 slots: not a multiple of 256
    "hw7": (lambda: pin_cases.load_hw7("practice7_1"), 48, 48, [2, 2, 4], dict(integrator=7), None),
    "hw6": (lambda: pin_cases.load_hw6("practice6_1"), 40, 24, [1, 2, 3], dict(integrator=6), None),
    "rounds": (pin_cases.load_sphere, 36, 20, [3, 5, 8, 16], {}, "wavefront"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_map_is_the_models_bit_for_bit(rt, monkeypatch, name):
    load, w, h, slices, kw, kernel = CASES[name]
    if kernel:
        monkeypatch.setenv("RTAMD_KERNEL", kernel)
    scene = rt.Scene(load())
    acc = scene.accumulator(w, h, **kw)
    mon = acc.noise_monitor()
    assert mon.batches == 0
    model = noise_model.Monitor(noise_model.blob_sums(acc.save(), w, h), 0)
    st = acc.render(slices[0])
    assert st.pipeline == (rt.RT_PIPELINE_ROUNDS if kernel else rt.RT_PIPELINE_PERSISTENT)
    mon.update()
    model.update(noise_model.blob_sums(acc.save(), w, h), acc.samples)
    se, s = _watch(acc, mon, model, w, h, slices[1:], name)
    assert s.batches == len(slices) and s.samples_observed == s.samples_total == sum(slices) and s.pixels == w * h and s.nonfinite_pixels == 0
    assert s.noise > 0 and s.worst_tile_noise >= s.noise and se.max() > 0
    # the summary alone, and the same bits a second time
    none, s2 = mon.estimate(want_map=False)
    assert none is None and all(getattr(s2, f) == getattr(s, f) for f in INT_FIELDS + DOUBLE_FIELDS)
    scene.close()   # closes the accumulator, which closes its monitor first
    assert not mon._h and not acc._h


def test_the_monitor_only_reads(rt, sphere_scene):
    w, h = 36, 20
    scene = rt.Scene(sphere_scene)
    plain = scene.accumulator(w, h)
    acc = scene.accumulator(w, h)
    mon = acc.noise_monitor()
    d = 0
    for n in (3, 5, 8):
        plain.render(n)
        acc.render(n)
        mon.update()
        if mon.batches >= 2:
            mon.estimate()
        d += n
        rgb, rgb8 = acc.resolve()
        one, one8, _ = scene.render(w, h, d)
        assert np.array_equal(rgb, one) and np.array_equal(rgb8, one8), d
    assert acc.save() == plain.save()
    scene.close()


def test_late_monitor_matches_the_model_and_reset_starts_afresh(rt, sphere_scene):
    w, h = 36, 20
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(w, h)
    acc.render(8)
    mon, twin = acc.noise_monitor(), acc.noise_monitor()
    model = noise_model.Monitor(noise_model.blob_sums(acc.save(), w, h), 8)
    for n in (4, 4, 4):
        acc.render(n)
        twin.update()
        mon.update()
        model.update(noise_model.blob_sums(acc.save(), w, h), acc.samples)
    se, s = mon.estimate()
    assert _same_map(se, model.estimate()[0])
    _check_summary(s, model.summary(), "attached after 8 samples:")
    assert s.samples_total == 20 and s.samples_observed == 12 and s.batches == 3
    se_twin, s_twin = twin.estimate()
    assert _same_map(se, se_twin) and all(getattr(s, f) == getattr(s_twin, f) for f in INT_FIELDS + DOUBLE_FIELDS)
    # reset, then two slices: a fresh monitor over those two slices
    mon.reset()
    assert mon.batches == 0 and twin.batches == 3
    fresh = acc.noise_monitor()
    for n in (5, 3):
        acc.render(n)
        mon.update()
        fresh.update()
    se, s = mon.estimate()
    se_fresh, s_fresh = fresh.estimate()
    assert s.batches == 2 and s.samples_observed == 8 and s.samples_total == 28
    assert _same_map(se, se_fresh) and all(getattr(s, f) == getattr(s_fresh, f) for f in INT_FIELDS + DOUBLE_FIELDS)
    scene.close()


def test_sharded(rt, sphere_scene):
    w, h, tile, shards, slices = 44, 28, 16, 3, [2, 3, 4]
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(w, h)
    mon = acc.noise_monitor()
    model = noise_model.Monitor(noise_model.blob_sums(acc.save(), w, h), 0)
    whole, s_whole = _watch(acc, mon, model, w, h, slices, "44x28 unsharded")
    tiles_x, tiles_y = (w + tile - 1) // tile, (h + tile - 1) // tile
    full = np.full((h, w), -1, np.float32)
    pixels = 0
    for r in range(shards):
        sacc = scene.accumulator(w, h, shard_index=r, shard_count=shards, tile=tile)
        smon = sacc.noise_monitor()
        for n in slices:
            sacc.render(n)
            smon.update()
        se, s = smon.estimate()
        mine = list(range(r, tiles_x * tiles_y, shards))
        assert se.shape == (len(mine) * tile * tile,)
        se = se.reshape(len(mine), tile, tile)
        for st, t in enumerate(mine):   # unshard, one channel: tile t of the frame is this shard's tile st
            x0, y0 = (t % tiles_x) * tile, (t // tiles_x) * tile
            tw, th = min(tile, w - x0), min(tile, h - y0)
            full[y0:y0 + th, x0:x0 + tw] = se[st, :th, :tw]
            pad = np.ones((tile, tile), bool)
            pad[:th, :tw] = False
            assert not se[st][pad].any()   # the padding of border tiles is zeroed
        pixels += s.pixels
        assert s.batches == 3 and s.samples_total == 9 and s.nonfinite_pixels == 0
    assert _same_map(full, whole) and pixels == w * h == s_whole.pixels
    scene.close()


def _nan_inf_scene(rt):
    """The scene of test_nan_and_inf_sums_go_through_the_state (tests/test_gpu_accum.py): a background with a NaN and an inf component
    behind two triangles."""
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
    return rt.SceneData(tris.reshape(n, 9), np.zeros((n, 6), np.float32), np.repeat(nrm[:, None, :], 3, axis=1).reshape(n, 9),
                        np.tile(np.array([1, 0, 0, 1], np.float32), (n, 3, 1)).reshape(n, 12), np.asarray([0, 1], np.uint32), mats, camera=cam,
                        bg=(float("nan"), float("inf"), 0.2))


def test_nan_and_inf_sums_are_counted_and_left_out(rt):
    w, h = 40, 24
    scene = rt.Scene(_nan_inf_scene(rt))
    acc = scene.accumulator(w, h)
    mon = acc.noise_monitor()
    model = noise_model.Monitor(noise_model.blob_sums(acc.save(), w, h), 0)
    se, s = _watch(acc, mon, model, w, h, [3, 2, 3], "NaN / inf background")
    _, _, _, finite = model.estimate()
    assert 0 < s.nonfinite_pixels < w * h and s.pixels + s.nonfinite_pixels == w * h
    assert np.array_equal(np.isfinite(se), finite) and not np.isfinite(se[~finite]).any()
    assert all(np.isfinite(getattr(s, f)) for f in DOUBLE_FIELDS)
    scene.close()


def test_errors(rt, sphere_scene):
    w, h = 36, 20
    scene = rt.Scene(sphere_scene)
    acc = scene.accumulator(w, h)
    mon = acc.noise_monitor()

    def refused(call, word):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID_ARG and word in str(e.value), str(e.value)

    refused(mon.update, "no samples")
    refused(mon.estimate, "0 batches")
    acc.render(4)
    mon.update()
    refused(mon.update, "no samples")
    refused(mon.estimate, "1 batches")
    assert mon.batches == 1
    acc.render(4)
    mon.update()
    blob = acc.save()
    good, s_good = mon.estimate()
    summary = rt.rt_noise_summary()
    summary.struct_size = C.sizeof(rt.rt_noise_summary)
    for flags in (rt.RT_FLAG_COUNTERS, rt.RT_FLAG_OUT_DEVICE | rt.RT_FLAG_SAMPLE_SEEDS, 1 << 31):
        assert rt.lib.rt_noise_estimate(mon._h, flags, None, C.byref(summary)) == rt.RT_ERR_INVALID_ARG
        assert rt.lib.rt_last_error().startswith(b"rt_noise_estimate: flags")
    summary.struct_size -= 8
    assert rt.lib.rt_noise_estimate(mon._h, 0, None, C.byref(summary)) == rt.RT_ERR_INVALID_ARG
    assert rt.lib.rt_last_error().startswith(b"rt_noise_estimate: struct_size")
    # a load replaces the state: the batches do not continue until a reset
    acc.render(4)
    acc.load(blob)
    assert acc.samples == 8
    refused(mon.update, "rt_accum_load")
    refused(mon.estimate, "rt_accum_load")
    acc.render(4)
    refused(mon.update, "rt_accum_load")
    mon.reset()
    assert mon.batches == 0
    refused(mon.update, "no samples")
    for n in (2, 2):
        acc.render(n)
        mon.update()
    se, s = mon.estimate()
    assert s.batches == 2 and s.samples_observed == 4 and s.samples_total == 16 and se.shape == good.shape
    scene.close()


DEVICE_MAP = """
import importlib, sys
import numpy as np
import torch
dev = torch.full(({h}, {w}), -1.0, dtype=torch.float32, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
rt = importlib.import_module("raytracing-course-hw_amd")
scene = rt.Scene(rt.load_gltf({gltf!r}))
acc = scene.accumulator({w}, {h})
mon = acc.noise_monitor()
for n in (3, 5, 8):
    acc.render(n)
    mon.update()
host, s_host = mon.estimate()
s_dev = mon.estimate_device(dev.data_ptr())
got = dev.cpu().numpy()
assert host.max() > 0 and np.array_equal(got, host), int((got != host).sum())
assert all(getattr(s_dev, f) == getattr(s_host, f) for f, _ in rt.rt_noise_summary._fields_[1:])
scene.close()
print("DEVICE MAP EQUAL")
"""


def test_map_into_device_memory():
    """RT_FLAG_OUT_DEVICE: the map written into a torch tensor on the scene's GPU is the host map.  In a process of its own, where torch
    opens the GPU before the library does (the order bench.py keeps)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gltf = os.path.join(root, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
    r = subprocess.run([sys.executable, "-c", DEVICE_MAP.format(w=36, h=20, root=root, gltf=gltf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE MAP EQUAL" in r.stdout, r.stdout + r.stderr

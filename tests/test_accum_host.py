"""Resumable renders, host side (no GPU): the rt_accum_* entry points are exported and declared, the size of a checkpoint follows
the frame's pixel slots, and null handles are errors, not crashes."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCUM = ["rt_accum_create", "rt_accum_render", "rt_accum_samples", "rt_accum_resolve", "rt_accum_state_bytes", "rt_accum_save",
         "rt_accum_load", "rt_accum_destroy"]
HEADER_MAX = 256       # the fixed header of a checkpoint (128 bytes today)
RT_ERR_INVALID_ARG = -1


def test_accum_symbols_are_exported_and_declared(rt):
    header = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    declared = set(re.findall(r"^(?:int|void|size_t)\s*(rt_accum_[a-z0-9_]+)\(", header, re.M))
    assert declared == set(ACCUM)
    for name in ACCUM:
        assert name in rt.ABI_SYMBOLS and hasattr(rt.lib, name), name
    assert rt.lib.rt_abi_version() == 6
    assert "#define RTAMD_ABI_VERSION 6" in header
    assert C.sizeof(rt.rt_render_params) == 64 and C.sizeof(rt.rt_stats) == 96


def _slots(w, h, tile, shard_index, shard_count):
    """Pixel slots of a shard: 64 per 8x8 sub-tile of its tiles (unsharded: the tiles are the 8x8 sub-tiles themselves)."""
    if shard_count <= 1:
        return ((w + 7) // 8) * ((h + 7) // 8) * 64
    tiles = ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
    return len(range(shard_index, tiles, shard_count)) * tile * tile


def test_state_bytes_follow_the_pixel_slots(rt):
    p = rt.make_params(1920, 1080, 0)
    n = rt.lib.rt_accum_state_bytes(C.byref(p))
    slots = _slots(1920, 1080, 32, 0, 1)
    assert 20 * 1920 * 1080 <= n <= 32 * slots + HEADER_MAX
    header = n % slots   # per-slot bytes are a whole number and the header is shorter than one byte per slot: the remainder
    per_slot = (n - header) // slots
    assert 20 <= per_slot <= 32 and 0 < header <= HEADER_MAX and header + per_slot * slots == n
    # `samples` is ignored, the integrators of the glTF scenes all have a state of the same shape
    for integ in (rt.RT_INTEGRATOR_HW6, rt.RT_INTEGRATOR_HW7, rt.RT_INTEGRATOR_HW8):
        assert rt.lib.rt_accum_state_bytes(C.byref(rt.make_params(1920, 1080, 77, integrator=integ))) == n
    # a shard's state covers its own tiles only (border tiles padded to whole tiles)
    total = 0
    for r in range(3):
        ps = rt.make_params(100, 70, 0, shard_index=r, shard_count=3, tile=32)
        ns = rt.lib.rt_accum_state_bytes(C.byref(ps))
        assert ns == header + per_slot * _slots(100, 70, 32, r, 3)
        total += ns - header
    assert total == per_slot * 4 * 3 * 32 * 32


@pytest.mark.parametrize("change", [dict(width=0), dict(height=-3), dict(struct_size=12), dict(reserved=1), dict(integrator=3), dict(integrator=99),
                                    dict(shard_count=2, shard_index=2), dict(shard_count=2, tile_w=12), dict(ray_depth=17)])
def test_state_bytes_of_invalid_params_is_zero_with_a_message(rt, change):
    p = rt.make_params(64, 48, 0)
    for k, v in change.items():
        setattr(p, k, v)
    rt.lib.rt_load_gltf(b"/nonexistent.gltf", 8, C.byref(C.c_void_p()))  # leaves some other message behind
    before = rt.lib.rt_last_error()
    assert rt.lib.rt_accum_state_bytes(C.byref(p)) == 0
    msg = rt.lib.rt_last_error()
    assert msg != before and msg.startswith(b"rt_accum_state_bytes:")
    assert rt.lib.rt_accum_state_bytes(None) == 0


def test_null_handles_are_invalid_arguments(rt):
    p = rt.make_params(64, 48, 0)
    out = C.c_void_p()
    st = rt.rt_stats()
    buf = C.create_string_buffer(64)
    assert rt.lib.rt_accum_create(None, C.byref(p), C.byref(out)) == RT_ERR_INVALID_ARG and not out
    assert b"rt_accum_create" in rt.lib.rt_last_error()
    assert rt.lib.rt_accum_render(None, 4, C.byref(st)) == RT_ERR_INVALID_ARG
    assert rt.lib.rt_accum_render(None, 4, None) == RT_ERR_INVALID_ARG
    assert rt.lib.rt_accum_samples(None) == RT_ERR_INVALID_ARG
    assert rt.lib.rt_accum_resolve(None, 0, None, None) == RT_ERR_INVALID_ARG
    assert rt.lib.rt_accum_save(None, buf, 64) == RT_ERR_INVALID_ARG
    assert rt.lib.rt_accum_load(None, buf.raw, 64) == RT_ERR_INVALID_ARG
    assert b"rt_accum_load" in rt.lib.rt_last_error()
    rt.lib.rt_accum_destroy(None)  # like free(NULL)
    assert rt.RT_ERR_INVALID_ARG == RT_ERR_INVALID_ARG and rt.RT_ERR_UNSUPPORTED == -4 and rt.RT_ERR_LIMIT == -7

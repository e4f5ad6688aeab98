"""Sharded renders of the three per-pixel pipelines no other test renders sharded: hw3 and hw4 (on the shared shell, for_each_pixel) and the hw8
megakernel (its own copy of that loop; both write through store_pixel).  A 44x28 frame in 16x16 tiles has a partial tile in every one of three shards
(44 is no multiple of 8, 28 none of 16): the shards put together must be the whole frame, floats and bytes, and whatever a shard buffer holds outside
the image must be black."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes", "txt")
W, H, SPP, TILE, SHARDS = 44, 28, 2, 16, 3


def _outside_image(k):
    """Mask over a shard buffer's pixels, (tiles, TILE, TILE): True where the pixel lies outside the image.  Shard k owns the tiles
    k, k + SHARDS, ... of the row-major tile grid, stored one after the other."""
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    gt = np.arange(k, tiles_x * tiles_y, SHARDS)
    y = (gt // tiles_x)[:, None, None] * TILE + np.arange(TILE)[None, :, None]
    x = (gt % tiles_x)[:, None, None] * TILE + np.arange(TILE)[None, None, :]
    return (x >= W) | (y >= H)


@pytest.mark.parametrize("case", ["hw3", "hw4", "mega"])
def test_three_shards_make_the_whole_frame_and_pad_with_black(rt, sphere_scene, monkeypatch, case):
    if case == "mega":
        monkeypatch.setenv("RTAMD_KERNEL", "mega")
        sd, kw = sphere_scene, {}
    else:
        integrator, name = {"hw3": (rt.RT_INTEGRATOR_HW3, "hw3_mixed_materials"), "hw4": (rt.RT_INTEGRATOR_HW4, "hw4_box_and_ellipsoid_lights")}[case]
        sd, _, _, _, depth = rt.load_txt(os.path.join(TXT, name + ".txt"), integrator)
        kw = dict(integrator=integrator, ray_depth=depth)
    scene = rt.Scene(sd)
    rgb, rgb8, _ = scene.render(W, H, SPP, tile=TILE, **kw)
    assert rgb.max() > 0 and rgb8.max() > 0
    full, full8, padding = np.zeros_like(rgb), np.zeros_like(rgb8), 0
    for k in range(SHARDS):
        buf, buf8, _ = scene.render(W, H, SPP, tile=TILE, shard_index=k, shard_count=SHARDS, **kw)
        p = rt.make_params(W, H, SPP, tile=TILE, shard_index=k, shard_count=SHARDS, **kw)
        full += rt.unshard(p, buf)
        full8 += rt.unshard(p, buf8)
        outside = _outside_image(k)
        assert buf.size == buf8.size == outside.size * 3
        padding += int(outside.sum())
        assert not buf.reshape(-1, TILE, TILE, 3)[outside].any()
        assert not buf8.reshape(-1, TILE, TILE, 3)[outside].any()
    assert padding == 6 * TILE * TILE - W * H
    assert np.array_equal(full, rgb)
    assert np.array_equal(full8, rgb8)
    scene.close()

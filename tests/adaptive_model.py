"""The decision of an adaptive slice (include/rtamd.h: rt_adaptive_render; csrc/host/rt_adaptive_decide.h) restated in numpy over the
tile records the library returns (rt.ADAPTIVE_TILE_DTYPE, shape (rows, columns)): float64 throughout, sums in the frame's sub-tile
order, row-major, which is what the host code does in double."""
import math

import numpy as np

ACTIVE, CONVERGED, CAPPED, NO_ESTIMATE = 1, 2, 4, 8
DILATE = 1
SAMPLE_LIMIT = 1 << 25


def mean_luminance(tiles):
    """The frame's mean luminance as rt_noise_estimate adds it: over the sub-tiles with an estimate and at least one finite pixel."""
    pixels, lum = 0, 0.0
    for t in tiles.reshape(-1):
        if (int(t["flags"]) & NO_ESTIMATE) or int(t["pixels"]) == 0:
            continue
        pixels += int(t["pixels"])
        lum += float(np.float64(t["sum_luminance"]))
    return lum / pixels if pixels else 0.0


def tile_noise(tiles):
    """sqrt(mean se^2) per sub-tile, float64; NaN where there is no estimate or no finite pixel."""
    out = np.full(tiles.shape, np.nan)
    ok = ((tiles["flags"] & NO_ESTIMATE) == 0) & (tiles["pixels"] > 0)
    out[ok] = np.sqrt(tiles["sum_se2"][ok].astype(np.float64) / tiles["pixels"][ok].astype(np.float64))
    return out


def decide(tiles, target_noise, min_batches, max_samples, flags, n_samples):
    """New flags (uint32, tiles' shape) from the records, whose own `flags` are the last decision's.  target_noise is taken as the
    float32 the params struct holds."""
    rows, cols = tiles.shape
    min_batches = min_batches if min_batches else 4
    max_samples = max_samples if max_samples else SAMPLE_LIMIT - 1
    bound = float(np.float64(np.float32(target_noise))) * mean_luminance(tiles)
    out = np.zeros(tiles.shape, dtype=np.uint32)
    for y in range(rows):
        for x in range(cols):
            t = tiles[y, x]
            f = int(t["flags"]) & (CONVERGED | NO_ESTIMATE)
            if not int(t["flags"]) & NO_ESTIMATE:
                if int(t["pixels"]) == 0:
                    f |= CONVERGED
                elif int(t["batches"]) >= min_batches and math.sqrt(float(np.float64(t["sum_se2"])) / int(t["pixels"])) <= bound:
                    f |= CONVERGED
            if int(t["samples"]) + n_samples > max_samples:
                f |= CAPPED
            out[y, x] = f
    done = (out & (CONVERGED | CAPPED)) != 0
    for y in range(rows):
        for x in range(cols):
            if out[y, x] & CAPPED:
                continue
            active = not out[y, x] & CONVERGED
            if not active and flags & DILATE:
                near = done[max(0, y - 1):y + 2, max(0, x - 1):x + 2].copy()
                near[min(y, 1), min(x, 1)] = True   # the sub-tile itself does not count
                active = not near.all()
            if active:
                out[y, x] |= ACTIVE
    return out

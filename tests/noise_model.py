"""The noise monitor's arithmetic (include/rtamd.h, rt_noise_*) restated in numpy: float32 with one rounding per operation, exactly the
operations of device/rt_noise.h in their order, so the per-pixel map can be compared bit for bit.  The per-sub-tile sums and the figures
of the frame are taken in float64 here (the kernel adds 64 float32 terms per sub-tile, the host adds the sub-tiles in double).

A model works on any array of pixels; `sums` are the accumulator's per-pixel sums (..., 3) as float32."""
import numpy as np

F = np.float32


def luminance(sums):
    s = np.asarray(sums, dtype=F)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * s[..., 0]) + (F(0.7152) * s[..., 1])) + (F(0.0722) * s[..., 2])


class Monitor:
    def __init__(self, sums, samples):
        self.reset(sums, samples)

    def reset(self, sums, samples):
        """create / reset: the sums as they are after `samples` samples per pixel."""
        self.y0 = luminance(sums)
        self.yp = self.y0.copy()
        self.m2 = np.zeros_like(self.y0)
        self.batches, self.observed, self.samples = 0, 0, int(samples)

    def update(self, sums, samples):
        """The samples between the last update and `samples` (the total per pixel now) are one batch."""
        n = int(samples) - self.samples
        assert n > 0
        yc = luminance(sums)
        with np.errstate(all="ignore"):
            mb = (yc - self.yp) / F(n)
            mu0 = mb if self.observed == 0 else (self.yp - self.y0) / F(self.observed)
            mu1 = (yc - self.y0) / F(self.observed + n)
            self.m2 = self.m2 + F(n) * ((mb - mu0) * (mb - mu1))
        assert self.m2.dtype == F
        self.yp = yc
        self.batches += 1
        self.observed += n
        self.samples = int(samples)

    def estimate(self):
        """(se, se2, mean luminance, finite) per pixel, float32; the picture has self.samples samples."""
        assert self.batches >= 2
        d = F(self.samples)
        with np.errstate(all="ignore"):
            s2 = np.where(self.m2 < 0, F(0), self.m2) / F(self.batches - 1)   # a NaN stays a NaN
            se2 = (s2 / d).astype(F)
            se = np.sqrt(se2)
            lum = self.yp / d
        finite = np.isfinite(self.yp) & np.isfinite(se2)
        return se, se2, lum, finite

    def summary(self):
        """The fields of rt_noise_summary for a (H, W) frame: sums per 8x8 sub-tile in float64, then over the sub-tiles row-major."""
        se, se2, lum, finite = self.estimate()
        h, w = se.shape
        tot_se2 = tot_lum = worst = 0.0
        pixels = 0
        for ty in range(0, h, 8):
            for tx in range(0, w, 8):
                f = finite[ty:ty + 8, tx:tx + 8]
                if not f.any():
                    continue
                t_se2 = float(se2[ty:ty + 8, tx:tx + 8][f].astype(np.float64).sum())
                tot_se2 += t_se2
                tot_lum += float(lum[ty:ty + 8, tx:tx + 8][f].astype(np.float64).sum())
                pixels += int(f.sum())
                worst = max(worst, t_se2 / int(f.sum()))
        mean = tot_lum / pixels if pixels else 0.0
        rms = float(np.sqrt(tot_se2 / pixels)) if pixels else 0.0
        return dict(batches=self.batches, samples_observed=self.observed, samples_total=self.samples, pixels=pixels,
                    nonfinite_pixels=int((~finite).sum()), mean_luminance=mean, rms_error=rms,
                    noise=rms / mean if mean != 0 else 0.0, worst_tile_noise=float(np.sqrt(worst)) / mean if mean != 0 else 0.0)


def blob_sums(blob, width, height):
    """Per-pixel sums (H, W, 3) float32 of an UNSHARDED checkpoint: a 128-byte header, then 16 bytes {r, g, b, x} per pixel slot; the slot
    of (x, y) is ((y >> 3) * ceil(W / 8) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)."""
    sub_w, sub_h = (width + 7) // 8, (height + 7) // 8
    slots = sub_w * sub_h * 64
    words = np.frombuffer(blob, np.float32, slots * 4, 128).reshape(slots, 4)
    y, x = np.mgrid[0:height, 0:width]
    return words[((y >> 3) * sub_w + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7), :3].copy()

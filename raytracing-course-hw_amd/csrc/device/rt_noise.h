// Noise monitor of a resumable render (include/rtamd.h: rt_noise_*): batch means over the slices of an rt_accum.  A pixel's samples
// come in order from its one engine, so the sums of consecutive slices are disjoint batches of one stream; how the batch means scatter
// gives the per-sample variance of the pixel's luminance and from it the standard error of the picture after d samples.  The three
// kernels only READ the rt_accum's state (the {sum r, g, b, engine} words accum_enter reads); what they keep is three floats per pixel
// slot, in three arrays so that a wave reads and writes whole contiguous lines:
//   y0  luminance of the sum when the monitor was created or reset,
//   yp  luminance of the sum at the last update,
//   m2  West's weighted sum of squares of the batch means so far (weights = samples per batch).
// All arithmetic is float32 with one rounding per operation (the build's -ffp-contract=off), written so that tests/noise_model.py
// restates it in numpy bit for bit.  Padding slots (outside the image) take part in nothing.
#pragma once
#include "rt_device.h"

namespace rtamd {

// What the estimate kernel leaves per 8x8 sub-tile (64 consecutive slots = one wave): sums over its finite pixels inside the image.
struct NoiseTile {
    float sum_se2;        // sum of se^2 = s2 / d
    float sum_luminance;  // sum of Y(sum) / d
    uint32_t pixels;      // how many pixels those sums are over
    uint32_t nonfinite;   // pixels inside the image whose luminance sum or estimate is NaN / inf (in neither sum)
};

struct NoiseView {
    const uint32_t *accum;  // the rt_accum's state
    float *y0, *yp, *m2;    // n_pixslots each
    // update: the batch is the n samples drawn since the last update, N the samples of the batches before it
    float n, N, N1;         // (float)n, (float)N, (float)(N + n)
    uint32_t first;         // N == 0
    // estimate: B batches, the picture has d samples
    float dof, d;           // (float)(B - 1), (float)d
    float *out_se;          // nullable: one float per pixel in the layout of rt_accum_resolve, one channel
    NoiseTile *tiles;       // n_pixslots / 64
};

namespace dev {

// Y of the slot's sum, Rec. 709 weights, added left to right.
RT_DEV float noise_luminance(const uint32_t *accum, uint32_t p) {
    const uint4 a = reinterpret_cast<const uint4 *>(accum)[p];
    return ((0.2126f * __uint_as_float(a.x)) + (0.7152f * __uint_as_float(a.y))) + (0.0722f * __uint_as_float(a.z));
}
RT_DEV bool noise_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Sum over the 64 lanes of a wave in a fixed order (a butterfly: every lane adds the same pairs, so every lane ends with the same bits,
// in every launch and on every shard layout: a sub-tile is the same 64 pixels in the same lanes wherever it lies).
RT_DEV float noise_wave_sum(float v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

#ifndef RT_NOISE_FUNCTIONS_ONLY // set by rt_adaptive.h, which wants the three functions above in rtamd_api.hip without a second copy of the kernels
// create / reset: y0 = yp = Y(sum), m2 = 0
__global__ __launch_bounds__(256) void noise_snapshot_kernel(RenderView R, NoiseView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const float yc = noise_luminance(V.accum, p);
        V.y0[p] = yc; V.yp[p] = yc; V.m2[p] = 0.f;
    }
}

// One more batch of n samples: West's weighted incremental variance of the batch means.  With mu0 / mu1 the mean per sample before / after
// the batch, m2 grows by n * (mb - mu0) * (mb - mu1), which is never negative in exact arithmetic.
__global__ __launch_bounds__(256) void noise_update_kernel(RenderView R, NoiseView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const float yc = noise_luminance(V.accum, p);
        const float y0 = V.y0[p], yp = V.yp[p];
        const float mb = (yc - yp) / V.n;
        const float mu0 = V.first ? mb : (yp - y0) / V.N;
        const float mu1 = (yc - y0) / V.N1;
        V.m2[p] = V.m2[p] + V.n * ((mb - mu0) * (mb - mu1));
        V.yp[p] = yc;
    }
}

// The estimate: s2 = max(m2, 0) / (B - 1) (a NaN m2 stays NaN), se^2 = s2 / d, se = sqrt(se^2), mean luminance = Y(sum) / d; the map and the
// sub-tile's four values.  n_pixslots is a multiple of 64 and blocks are 256 threads, so a wave is in or out of the loop as a whole and its
// lanes are the 64 pixels of sub-tile p >> 6.  The state of the monitor and of the rt_accum is only read.
__global__ __launch_bounds__(256) void noise_estimate_kernel(RenderView R, NoiseView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        float se2 = 0.f, lum = 0.f, se = 0.f;
        bool finite = false;
        if (inside) {
            const float yc = noise_luminance(V.accum, p);
            const float m2 = V.m2[p];
            const float s2 = (m2 < 0.f ? 0.f : m2) / V.dof;
            se2 = s2 / V.d;
            se = sqrtf(se2);
            lum = yc / V.d;
            finite = noise_finite(yc) && noise_finite(se2);
        }
        if (V.out_se && (inside || R.shard_count > 1)) V.out_se[out_index] = se; // the padding of a border tile in the compact layout: 0
        const float sum_se2 = noise_wave_sum(finite ? se2 : 0.f);
        const float sum_lum = noise_wave_sum(finite ? lum : 0.f);
        const uint32_t n_finite = (uint32_t)__popcll(__ballot(finite));
        const uint32_t n_bad = (uint32_t)__popcll(__ballot(inside && !finite));
        if ((threadIdx.x & 63u) == 0u) {
            NoiseTile t;
            t.sum_se2 = sum_se2; t.sum_luminance = sum_lum; t.pixels = n_finite; t.nonfinite = n_bad;
            V.tiles[p >> 6] = t;
        }
    }
}

#endif // RT_NOISE_FUNCTIONS_ONLY

} // namespace dev
} // namespace rtamd

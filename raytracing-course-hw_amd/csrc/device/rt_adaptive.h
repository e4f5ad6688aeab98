// Adaptive sampling (include/rtamd.h: rt_adaptive_*): the flat kernels around the persistent hw8 kernel's pixel source (rt_path_source.h,
// src_mode 4).  A slice draws samples for the ACTIVE 8x8 sub-tiles of a frame only: their state is gathered into a compact strip, the
// persistent kernel runs a slice of a resumable render over the strip, the state is scattered back.  The frame is unsharded, so its
// tiles are the 8x8 sub-tiles themselves, row-major over ceil(W/8) x ceil(H/8), 64 pixel slots each: sub-tile t owns slots 64 t .. 64 t + 63
// in the state's two arrays (accum_enter / accum_leave of rt_wavefront.h), strip sub-tile s stands for sub-tile list[s].
//
//   ad_gather_kernel    one lane per strip slot: the state words {sum, engine}, {saved, has_saved} from frame slot to strip slot, and the
//                       slot's pixel x | y << 16 (slot_to_pixel on the real geometry, here and not in the persistent kernel).  Beyond the
//                       list: engine word 0, which starts no path, and the pixel word of a slot outside the image
//   ad_scatter_kernel   the reverse, for the list's slots only
//   ad_resolve_kernel   accum_resolve_kernel with inv_samples read per sub-tile; a sub-tile without samples writes zeros
//   ad_update_kernel    noise_update_kernel's expressions in their order, n, N, N1 and first read per sub-tile, over the list only: a frozen
//                       sub-tile's statistics do not move
//   ad_estimate_kernel  noise_estimate_kernel's expressions in their order, dof and d read per sub-tile, over the whole frame; a sub-tile
//                       with fewer than two batches (dof < 1) gets se = 0 in the map and an entry of zeros marked AD_NO_ESTIMATE: nothing
//                       is divided by zero
// The last two run one wave per sub-tile (blocks of 256 = four sub-tiles) and add with noise_wave_sum: no float atomics, the same bits in
// every run.  All arithmetic is float32 with one rounding per operation (-ffp-contract=off), as rt_noise.h.
#pragma once
#define RT_NOISE_FUNCTIONS_ONLY // noise_luminance, noise_finite, noise_wave_sum; the monitor's kernels stay rtamd_noise.hip's alone
#include "rt_noise.h"
#include "rt_types_adaptive.h"
#include "rt_wavefront.h"

namespace rtamd {

static_assert(sizeof(AdTile) == sizeof(NoiseTile) && sizeof(AdTile) == 16, "an AdTile is a NoiseTile, field for field");
#define AD_PIXEL_OUTSIDE 0xffffffffu

namespace dev {

__global__ __launch_bounds__(256) void ad_gather_kernel(RenderView R, AdaptiveView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.strip_slots; i += gridDim.x * 256u) {
        const uint32_t s = i >> 6;
        const uint32_t p = s < V.n_list ? 64u * V.list[s] + (i & 63u) : V.n_pixslots;
        uint4 a = make_uint4(0u, 0u, 0u, 0u);
        uint2 b = make_uint2(0u, 0u);
        uint32_t xy = AD_PIXEL_OUTSIDE;
        if (p < V.n_pixslots) {
            a = reinterpret_cast<const uint4 *>(V.state)[p];
            b = reinterpret_cast<const uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[p];
            int x, y; bool inside; size_t out_index;
            slot_to_pixel(R, p, x, y, inside, out_index);
            if (inside) xy = (uint32_t)x | ((uint32_t)y << 16);
        }
        reinterpret_cast<uint4 *>(V.strip)[i] = a;
        reinterpret_cast<uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i] = b;
        V.pixels[i] = xy;
    }
}

__global__ __launch_bounds__(256) void ad_scatter_kernel(RenderView R, AdaptiveView V) {
    const uint32_t n = V.n_list * 64u < V.strip_slots ? V.n_list * 64u : V.strip_slots;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t p = 64u * V.list[i >> 6] + (i & 63u);
        if (p >= V.n_pixslots) continue;
        reinterpret_cast<uint4 *>(V.state)[p] = reinterpret_cast<const uint4 *>(V.strip)[i];
        reinterpret_cast<uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[p] = reinterpret_cast<const uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i];
    }
}

// pixel = inv_samples[sub-tile] * sum and the tonemap, exactly as accum_resolve_kernel; the state is only read
__global__ __launch_bounds__(256) void ad_resolve_kernel(RenderView R, AdaptiveView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const float inv = V.inv_samples[p >> 6];
        F3 px = f3(0.f, 0.f, 0.f);
        uint8_t b0 = 0, b1 = 0, b2 = 0;
        if (inv != 0.f) {
            Rng rng; F3 sum;
            accum_enter(R, p, rng, sum);
            px = inv * sum;                                          // scene.cpp:176
            b0 = tonemap1(px.x); b1 = tonemap1(px.y); b2 = tonemap1(px.z); // sceneio.cpp:393-395
        }
        if (R.out_rgb) { R.out_rgb[3 * out_index] = px.x; R.out_rgb[3 * out_index + 1] = px.y; R.out_rgb[3 * out_index + 2] = px.z; }
        if (R.out_rgb8) { R.out_rgb8[3 * out_index] = b0; R.out_rgb8[3 * out_index + 1] = b1; R.out_rgb8[3 * out_index + 2] = b2; }
    }
}

__global__ __launch_bounds__(256) void ad_update_kernel(RenderView R, AdaptiveView V) {
    const uint32_t n = V.n_list * 64u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t t = V.list[i >> 6], p = 64u * t + (i & 63u);
        if (p >= R.n_pixslots) continue;
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const AdTileArgs A = V.args[t];
        const float yc = noise_luminance(V.state, p);
        const float y0 = V.y0[p], yp = V.yp[p];
        const float mb = (yc - yp) / A.n;
        const float mu0 = A.first ? mb : (yp - y0) / A.N;
        const float mu1 = (yc - y0) / A.N1;
        V.m2[p] = V.m2[p] + A.n * ((mb - mu0) * (mb - mu1));
        V.yp[p] = yc;
    }
}

// n_pixslots is a multiple of 64 and blocks are 256 threads: a wave is in or out of the loop as a whole, its lanes are sub-tile p >> 6
__global__ __launch_bounds__(256) void ad_estimate_kernel(RenderView R, AdaptiveView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        const AdTileArgs A = V.args[p >> 6];
        const bool estimate = A.dof >= 1.f;                          // two batches or more
        float se2 = 0.f, lum = 0.f, se = 0.f;
        bool finite = false;
        if (inside && estimate) {
            const float yc = noise_luminance(V.state, p);
            const float m2 = V.m2[p];
            const float s2 = (m2 < 0.f ? 0.f : m2) / A.dof;
            se2 = s2 / A.d;
            se = sqrtf(se2);
            lum = yc / A.d;
            finite = noise_finite(yc) && noise_finite(se2);
        }
        if (V.out_se && inside) V.out_se[out_index] = se;
        const float sum_se2 = noise_wave_sum(finite ? se2 : 0.f);
        const float sum_lum = noise_wave_sum(finite ? lum : 0.f);
        const uint32_t n_finite = (uint32_t)__popcll(__ballot(finite));
        const uint32_t n_bad = (uint32_t)__popcll(__ballot(inside && !finite));
        if ((threadIdx.x & 63u) == 0u) {
            AdTile t;
            t.sum_se2 = sum_se2; t.sum_luminance = sum_lum; t.pixels = n_finite; t.nonfinite = estimate ? n_bad : AD_NO_ESTIMATE;
            V.tiles[p >> 6] = t;
        }
    }
}

} // namespace dev
} // namespace rtamd

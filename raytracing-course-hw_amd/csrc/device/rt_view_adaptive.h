// Adaptive sampling for view sets (include/rtamd.h: rt_view_adaptive_*): the flat kernels around the persistent hw8 kernel's view source
// (rt_path_source.h, src_mode 5).  A slice draws samples for the ACTIVE 8x8 sub-tiles of ALL views in one strip: strip sub-tile s stands
// for the word list[s] = G = view * tiles + sub-tile, whatever mix of views the list holds.  The view source reads the view once per
// 64-slot group and the pixel per slot, so the strip is src_pixels' layout as vw_gather_kernel (rt_views.h) writes it; nothing in the
// persistent kernel changes.  Layout of the state: rt_types_view_adaptive.h.
//
//   va_gather_kernel    one lane per strip slot: the state words {sum, engine}, {saved, has_saved} from the view's block to the strip, the
//                       slot's pixel x | y << 16 (slot_to_pixel on the view's geometry; the word of a slot outside the image for padding,
//                       whose engine word is the 0 accum_seed_kernel left) and per 64-slot group the view index behind the pixel words.
//                       Beyond the list: engine word 0, which starts no path.  The divisions by the sub-tiles of a view are here
//   va_scatter_kernel   the reverse, state words only, for the list's slots
//   va_update_kernel    ad_update_kernel's expressions in their order (rt_adaptive.h), n, N, N1 and first read per (view, sub-tile), over
//                       the list only: a frozen sub-tile's statistics do not move
//   va_estimate_kernel  ad_estimate_kernel's expressions in their order, dof and d read per (view, sub-tile), over sub-tiles first ..
//                       first + count - 1: all sub-tiles of all views without a map after a slice, one view's with a map for
//                       rt_view_adaptive_noise
//   va_resolve_kernel   ad_resolve_kernel on one view's block, inv_samples read per sub-tile
// Update and estimate run one wave per sub-tile (blocks of 256 = four sub-tiles) and add with noise_wave_sum: no float atomics, the same
// bits in every run.  All arithmetic is float32 with one rounding per operation (-ffp-contract=off), as rt_noise.h.
#pragma once
#include "rt_adaptive.h" // noise_luminance, noise_finite, noise_wave_sum (rt_noise.h, functions only); slot_to_pixel, accum_enter, tonemap1
#include "rt_types_view_adaptive.h"

namespace rtamd {

#define VA_PIXEL_OUTSIDE 0xffffffffu

namespace dev {

// the word G -> the view and the pixel slot `lane` of the sub-tile in that view's block
RT_DEV void va_slot(const ViewAdaptiveView &V, uint32_t G, uint32_t lane, uint32_t &view, uint32_t &p) {
    view = G / V.tiles;
    p = 64u * (G - view * V.tiles) + lane;
}

__global__ __launch_bounds__(256) void va_gather_kernel(RenderView R, ViewAdaptiveView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.strip_slots; i += gridDim.x * 256u) {
        const uint32_t s = i >> 6;
        uint4 a = make_uint4(0u, 0u, 0u, 0u);
        uint2 b = make_uint2(0u, 0u);
        uint32_t xy = VA_PIXEL_OUTSIDE, view = 0u;
        if (s < V.n_list) {
            uint32_t p;
            va_slot(V, V.list[s], i & 63u, view, p);
            const uint32_t *block = V.state + 6 * (size_t)view * V.vslots;
            a = reinterpret_cast<const uint4 *>(block)[p];
            b = reinterpret_cast<const uint2 *>(block + 4 * (size_t)V.vslots)[p];
            int x, y; bool inside; size_t out_index;
            slot_to_pixel(R, p, x, y, inside, out_index);
            if (inside) xy = (uint32_t)x | ((uint32_t)y << 16);
        }
        reinterpret_cast<uint4 *>(V.strip)[i] = a;
        reinterpret_cast<uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i] = b;
        V.pixels[i] = xy;
        if ((i & 63u) == 0u) V.pixels[V.strip_slots + s] = view;
    }
}

__global__ __launch_bounds__(256) void va_scatter_kernel(RenderView R, ViewAdaptiveView V) {
    const uint32_t n = V.n_list * 64u < V.strip_slots ? V.n_list * 64u : V.strip_slots;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint32_t view, p;
        va_slot(V, V.list[i >> 6], i & 63u, view, p);
        uint32_t *block = V.state + 6 * (size_t)view * V.vslots;
        reinterpret_cast<uint4 *>(block)[p] = reinterpret_cast<const uint4 *>(V.strip)[i];
        reinterpret_cast<uint2 *>(block + 4 * (size_t)V.vslots)[p] = reinterpret_cast<const uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i];
    }
}

__global__ __launch_bounds__(256) void va_update_kernel(RenderView R, ViewAdaptiveView V) {
    const uint32_t n = V.n_list * 64u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t G = V.list[i >> 6];
        uint32_t view, p;
        va_slot(V, G, i & 63u, view, p);
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const AdTileArgs A = V.args[G];
        float *y0p = V.planes + 3 * (size_t)view * V.vslots, *ypp = y0p + V.vslots, *m2p = ypp + V.vslots;
        const float yc = noise_luminance(V.state + 6 * (size_t)view * V.vslots, p);
        const float y0 = y0p[p], yp = ypp[p];
        const float mb = (yc - yp) / A.n;
        const float mu0 = A.first ? mb : (yp - y0) / A.N;
        const float mu1 = (yc - y0) / A.N1;
        m2p[p] = m2p[p] + A.n * ((mb - mu0) * (mb - mu1));
        ypp[p] = yc;
    }
}

// count * 64 lanes in blocks of 256: a wave is in or out of the loop as a whole, its lanes are one sub-tile
__global__ __launch_bounds__(256) void va_estimate_kernel(RenderView R, ViewAdaptiveView V) {
    const uint32_t n = V.count * 64u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t G = V.first + (i >> 6);
        uint32_t view, p;
        va_slot(V, G, i & 63u, view, p);
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        const AdTileArgs A = V.args[G];
        const bool estimate = A.dof >= 1.f;                          // two batches or more
        float se2 = 0.f, lum = 0.f, se = 0.f;
        bool finite = false;
        if (inside && estimate) {
            const float yc = noise_luminance(V.state + 6 * (size_t)view * V.vslots, p);
            const float m2 = V.planes[3 * (size_t)view * V.vslots + 2 * (size_t)V.vslots + p];
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
            V.entries[G] = t;
        }
    }
}

// pixel = inv_samples[sub-tile] * sum and the tonemap, exactly as ad_resolve_kernel; R.accum is the view's block, which is only read
__global__ __launch_bounds__(256) void va_resolve_kernel(RenderView R, ViewAdaptiveView V) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < R.n_pixslots; p += gridDim.x * 256u) {
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        if (!inside) continue;
        const float inv = V.inv_samples[V.first + (p >> 6)];
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

} // namespace dev
} // namespace rtamd

// Adaptive sampling (include/rtamd.h: rt_adaptive_*): what the flat kernels of rt_adaptive.h see, and what the host side
// (rtamd_adaptive.hip) asks of the translation unit that holds them (rtamd_api.hip: every __global__ keeps one definition there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include "rt_types.h"

struct rt_scene;

namespace rtamd {

// What ad_estimate_kernel leaves per 8x8 sub-tile: rt_noise.h's NoiseTile, field for field.  A sub-tile with fewer than two batches has
// no estimate: zeros, and AD_NO_ESTIMATE in `nonfinite`.
struct AdTile { float sum_se2, sum_luminance; uint32_t pixels, nonfinite; };
#define AD_NO_ESTIMATE 0xffffffffu

// The noise monitor's per-launch numbers (rt_noise.h NoiseView), here per sub-tile.
struct AdTileArgs {
    float n, N, N1;        // update: (float)n, (float)N, (float)(N + n) of the slice being added
    uint32_t first;        // update: N == 0
    float dof, d;          // estimate: (float)(B - 1), (float)d AFTER the slice; dof < 1: no estimate
};

struct AdaptiveView {
    uint32_t *state;           // the frame's state, rt_accum's layout: n_pixslots x {sum.xyz, Rng::x}, then n_pixslots x {saved, has_saved}
    uint32_t n_pixslots;       // 64 per sub-tile of the frame
    uint32_t *strip;           // the strip's state in the same layout over strip_slots
    uint32_t strip_slots;      // 64 per sub-tile of the chunk
    uint32_t *pixels;          // strip_slots x (x | y << 16): RenderView::src_pixels
    const uint32_t *list;      // n_list sub-tiles of the frame: strip sub-tile s stands for list[s]
    uint32_t n_list;
    float *y0, *yp, *m2;       // the monitor's planes, n_pixslots each
    const AdTileArgs *args;    // n_pixslots / 64
    const float *inv_samples;  // n_pixslots / 64: (float)(1.0 / d_s), 0 for d_s = 0
    float *out_se;             // nullable: W*H
    AdTile *tiles;             // n_pixslots / 64
};

// The launches, on `stream`; each returns the number of launches.  R: the real frame's geometry.
uint32_t adaptive_launch_gather(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream);
uint32_t adaptive_launch_scatter(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream);
uint32_t adaptive_launch_resolve(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream);
uint32_t adaptive_launch_update(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream);
uint32_t adaptive_launch_estimate(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream);
// A fresh state for the frame R (accum_seed_kernel) and the frame's tan_fov_x as the renders evaluate it.
void adaptive_launch_seed(const rt_scene *scene, const RenderView &R, hipStream_t stream);
float adaptive_tan_fov_x(const rt_scene *scene, int32_t width, int32_t height);

// The chunk loop of the query layer (rtamd_query.hip: chunks) over a list of `items` with no caller arrays: body(first, m) per chunk,
// one synchronisation after each.  source_chunk_slots: the slots of one path-source chunk (RTAMD_QUERY_CHUNK lowers it).
size_t source_chunk_slots();
int source_chunks(size_t items, size_t chunk_items, hipStream_t stream, const std::function<int(size_t first, size_t m)> &body);

} // namespace rtamd

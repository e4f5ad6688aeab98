// Adaptive sampling for view sets (include/rtamd.h: rt_view_adaptive_*): what the flat kernels of rt_view_adaptive.h see, and what the
// host side (rtamd_view_adaptive.hip) asks of the translation unit that holds them (rtamd_api.hip: every __global__ keeps one definition
// there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_types.h"
#include "rt_types_adaptive.h" // AdTile, AdTileArgs

struct rt_scene;

namespace rtamd {

// The state of an adaptive view set: per view one block in rt_accum's layout over the view's pixel slots, as a view set keeps it
// (rt_types_views.h), and one block of the noise monitor's planes y0, yp, m2 (vslots floats each, in this order).  Sub-tile t of view v
// is the word G = v * tiles + t: the entries, the arguments and the list of a slice are indexed by it, view-major.
struct ViewAdaptiveView {
    uint32_t *state;           // n_views x 6 vslots words
    float *planes;             // n_views x 3 vslots floats
    uint32_t vslots, tiles;    // pixel slots and 8x8 sub-tiles of one view (vslots = 64 tiles)
    uint32_t *strip;           // the chunk's state in rt_accum's layout over strip_slots
    uint32_t strip_slots;      // 64 per sub-tile of the chunk
    uint32_t *pixels;          // strip_slots x (x | y << 16), then strip_slots / 64 x view index: RenderView::src_pixels
    const uint32_t *list;      // n_list words G, ascending: strip sub-tile s stands for list[s]
    uint32_t n_list;
    uint32_t first, count;     // estimate: sub-tiles G = first .. first + count - 1; resolve: first = the view's first G
    const AdTileArgs *args;    // n_views x tiles
    const float *inv_samples;  // n_views x tiles: (float)(1.0 / d), 0 for d = 0; written for the view being resolved
    float *out_se;             // nullable: W*H of the ONE view the estimate runs over
    AdTile *entries;           // n_views x tiles
};

// The launches, on `stream`; each returns the number of launches.  R: the geometry of one view's frame.
uint32_t view_adaptive_launch_gather(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream);
uint32_t view_adaptive_launch_scatter(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream);
uint32_t view_adaptive_launch_update(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream);
uint32_t view_adaptive_launch_estimate(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream);
uint32_t view_adaptive_launch_resolve(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream);

} // namespace rtamd

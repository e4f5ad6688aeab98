// A batch of cameras over one scene (include/rtamd.h: rt_views_*): what the flat kernels of rt_views.h see, and what the host side
// (rtamd_views.hip) asks of the translation unit that holds them (rtamd_api.hip: every __global__ keeps one definition there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_types.h"

struct rt_scene;

namespace rtamd {

// The state of a view set: one block per view, each rt_accum's layout over the view's pixel slots (vslots x {sum.xyz, Rng::x}, then
// vslots x {saved, has_saved}; 64 slots per 8x8 sub-tile, row-major over ceil(W/8) x ceil(H/8)), so that the kernels of a resumable
// render seed and resolve one view's block as they stand.  A slice runs over the sub-tiles of the ACTIVE views in list order: sub-tile T
// of that sequence is sub-tile T % tiles of view list[T / tiles].
struct ViewsView {
    uint32_t *state;           // n_views x 6 vslots words
    uint32_t vslots, tiles;    // pixel slots and 8x8 sub-tiles of one view (vslots = 64 tiles)
    uint32_t *strip;           // the chunk's state in rt_accum's layout over strip_slots
    uint32_t strip_slots;      // 64 per sub-tile of the chunk
    uint32_t *pixels;          // strip_slots x (x | y << 16), then strip_slots / 64 x view index: RenderView::src_pixels
    const uint32_t *list;      // the active views, ascending
    uint32_t first_tile;       // the chunk's first sub-tile in the sequence
};

// The launches, on `stream`; each returns the number of launches.  R: the geometry of one view's frame.
uint32_t views_launch_gather(const rt_scene *scene, const RenderView &R, const ViewsView &V, hipStream_t stream);
uint32_t views_launch_scatter(const rt_scene *scene, const RenderView &R, const ViewsView &V, hipStream_t stream);
// One view's block: a fresh state (accum_seed_kernel), and its picture (accum_resolve_kernel); R.accum is the block.
void views_launch_seed(const rt_scene *scene, const RenderView &R, hipStream_t stream);
void views_launch_resolve(const rt_scene *scene, const RenderView &R, hipStream_t stream);

} // namespace rtamd

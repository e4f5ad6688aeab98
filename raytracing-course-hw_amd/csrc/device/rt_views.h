// A batch of cameras over one scene (include/rtamd.h: rt_views_*): the flat kernels around the persistent hw8 kernel's view source
// (rt_path_source.h, src_mode 5).  A slice draws samples for the ACTIVE views of a set: the state of their 8x8 sub-tiles is gathered into
// a compact strip, the persistent kernel runs a slice of a resumable render over the strip, the state is scattered back.  Layout and
// the order of the strip: rt_types_views.h.
//
//   vw_gather_kernel    one lane per strip slot: the state words {sum, engine}, {saved, has_saved} from the view's block to the strip, the
//                       slot's pixel x | y << 16 (slot_to_pixel on the view's geometry, here and not in the persistent kernel; the word
//                       of a slot outside the image for padding, whose engine word is the 0 accum_seed_kernel left), and per 64-slot
//                       group the view index behind the pixel words.  The divisions by the sub-tiles of a view are here too
//   vw_scatter_kernel   the reverse, state words only
// Seeding and resolving a view are rt_accum's kernels on the view's block (accum_seed_kernel, accum_resolve_kernel of rt_wavefront.h):
// a view IS a resumable render with a camera of its own.  One lane per slot, no atomics.
#pragma once
#include "rt_types_views.h"
#include "rt_wavefront.h"

namespace rtamd {

#define VW_PIXEL_OUTSIDE 0xffffffffu

namespace dev {

// strip slot i -> the view behind it and the slot in that view's block
RT_DEV void vw_slot(const ViewsView &V, uint32_t i, uint32_t &view, uint32_t &p) {
    const uint32_t T = V.first_tile + (i >> 6), a = T / V.tiles;
    view = V.list[a];
    p = 64u * (T - a * V.tiles) + (i & 63u);
}

__global__ __launch_bounds__(256) void vw_gather_kernel(RenderView R, ViewsView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.strip_slots; i += gridDim.x * 256u) {
        uint32_t view, p;
        vw_slot(V, i, view, p);
        const uint32_t *block = V.state + 6 * (size_t)view * V.vslots;
        reinterpret_cast<uint4 *>(V.strip)[i] = reinterpret_cast<const uint4 *>(block)[p];
        reinterpret_cast<uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i] = reinterpret_cast<const uint2 *>(block + 4 * (size_t)V.vslots)[p];
        int x, y; bool inside; size_t out_index;
        slot_to_pixel(R, p, x, y, inside, out_index);
        V.pixels[i] = inside ? (uint32_t)x | ((uint32_t)y << 16) : VW_PIXEL_OUTSIDE;
        if ((i & 63u) == 0u) V.pixels[V.strip_slots + (i >> 6)] = view;
    }
}

__global__ __launch_bounds__(256) void vw_scatter_kernel(RenderView R, ViewsView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.strip_slots; i += gridDim.x * 256u) {
        uint32_t view, p;
        vw_slot(V, i, view, p);
        uint32_t *block = V.state + 6 * (size_t)view * V.vslots;
        reinterpret_cast<uint4 *>(block)[p] = reinterpret_cast<const uint4 *>(V.strip)[i];
        reinterpret_cast<uint2 *>(block + 4 * (size_t)V.vslots)[p] = reinterpret_cast<const uint2 *>(V.strip + 4 * (size_t)V.strip_slots)[i];
    }
}

} // namespace dev
} // namespace rtamd

// The planning step of an adaptive slice over a view set (include/rtamd.h: rt_view_adaptive_render, rt_view_adaptive_render_tiles): the
// decision per view and the ascending list of words G = view * tiles + sub-tile that the slice draws for; the monitor's numbers per
// (view, sub-tile) are adaptive_slice_args' (rt_adaptive_decide.h) over all words.  Host functions with no GPU call in them, shared by
// rtamd_view_adaptive.hip and the test hook rtt_view_adaptive_plan (test_hooks.hip); tests/test_view_adaptive_host.py restates them in
// numpy on tests/adaptive_model.py.
#pragma once
#include <cstdint>
#include <vector>
#include "rt_adaptive_decide.h"

namespace rtamd {

// adaptive_decide per view, each over its own table (sub_w * sub_h entries, view-major in `tiles`) with its own mean luminance; dilation
// looks at the neighbours inside the view only.  A view whose view_mask byte is 0 (NULL mask: none is) keeps the flags it has.
inline void view_adaptive_decide(const rt_adaptive_tile *tiles, const rt_adaptive_params &p, int32_t sub_w, int32_t sub_h, int32_t n_views, int32_t n_samples,
                                 const uint8_t *view_mask, uint32_t *flags) {
    const size_t per_view = (size_t)sub_w * (size_t)sub_h;
    for (int32_t v = 0; v < n_views; v++) {
        const rt_adaptive_tile *table = tiles + (size_t)v * per_view;
        uint32_t *out = flags + (size_t)v * per_view;
        if (view_mask && !view_mask[v]) for (size_t t = 0; t < per_view; t++) out[t] = table[t].flags;
        else adaptive_decide(table, p, sub_w, sub_h, n_samples, out);
    }
}

// The list of the policy: the ACTIVE sub-tiles of the views that take part, by `flags` of view_adaptive_decide.
inline void view_adaptive_list_policy(const uint32_t *flags, size_t per_view, int32_t n_views, const uint8_t *view_mask, std::vector<uint32_t> &list) {
    list.clear();
    for (int32_t v = 0; v < n_views; v++) {
        if (view_mask && !view_mask[v]) continue;
        for (size_t t = 0; t < per_view; t++)
            if (flags[(size_t)v * per_view + t] & RT_ADAPTIVE_ACTIVE) list.push_back((uint32_t)((size_t)v * per_view + t));
    }
}

// The list of the mechanism: one byte per (view, sub-tile), view-major.
inline void view_adaptive_list_tiles(const uint8_t *tile_mask, size_t n, std::vector<uint32_t> &list) {
    list.clear();
    for (size_t G = 0; G < n; G++) if (tile_mask[G]) list.push_back((uint32_t)G);
}

} // namespace rtamd

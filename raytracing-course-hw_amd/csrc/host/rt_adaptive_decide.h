// The decision of an adaptive slice (include/rtamd.h: rt_adaptive_render): which 8x8 sub-tiles of the frame go on drawing samples.
// One host function with no GPU call in it, shared by rtamd_adaptive.hip and the test hook rtt_adaptive_decide (test_hooks.hip);
// tests/adaptive_model.py restates it in numpy.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../../include/rtamd.h"

namespace rtamd {

#define ADAPTIVE_SAMPLE_LIMIT (1 << 25) // the path records' sample index (wf_pack): a sub-tile's count stays below it

inline int32_t adaptive_min_batches(const rt_adaptive_params &p) { return p.min_batches ? p.min_batches : 4; }
inline int32_t adaptive_max_samples(const rt_adaptive_params &p) { return p.max_samples ? p.max_samples : ADAPTIVE_SAMPLE_LIMIT - 1; }

// tiles: sub_w * sub_h entries, row-major, whose flags are those of the last decision (CONVERGED is sticky, NO_ESTIMATE says whether
// the entry's sums mean anything); n_samples: the length of the slice the decision is for (the cap).  flags: the new flags.
inline void adaptive_decide(const rt_adaptive_tile *tiles, const rt_adaptive_params &p, int32_t sub_w, int32_t sub_h, int32_t n_samples, uint32_t *flags) {
    const size_t n = (size_t)sub_w * (size_t)sub_h;
    const int32_t min_batches = adaptive_min_batches(p), max_samples = adaptive_max_samples(p);
    uint64_t pixels = 0;
    double lum = 0;
    for (size_t i = 0; i < n; i++) { // the frame's mean luminance, as noise_summarise adds it
        const rt_adaptive_tile &t = tiles[i];
        if ((t.flags & RT_ADAPTIVE_NO_ESTIMATE) || !t.pixels) continue;
        pixels += t.pixels;
        lum += (double)t.sum_luminance;
    }
    const double L = pixels ? lum / (double)pixels : 0.0;
    for (size_t i = 0; i < n; i++) {
        const rt_adaptive_tile &t = tiles[i];
        uint32_t f = t.flags & (RT_ADAPTIVE_CONVERGED | RT_ADAPTIVE_NO_ESTIMATE);
        if (!(t.flags & RT_ADAPTIVE_NO_ESTIMATE)) {
            if (!t.pixels) f |= RT_ADAPTIVE_CONVERGED;
            else if (t.batches >= min_batches && std::sqrt((double)t.sum_se2 / (double)t.pixels) <= (double)p.target_noise * L) f |= RT_ADAPTIVE_CONVERGED;
        }
        if ((int64_t)t.samples + (int64_t)n_samples > (int64_t)max_samples) f |= RT_ADAPTIVE_CAPPED;
        flags[i] = f;
    }
    const bool dilate = (p.flags & RT_ADAPTIVE_DILATE) != 0;
    for (int32_t y = 0; y < sub_h; y++)
        for (int32_t x = 0; x < sub_w; x++) {
            uint32_t &f = flags[(size_t)y * sub_w + x];
            if (f & RT_ADAPTIVE_CAPPED) continue;
            bool active = !(f & RT_ADAPTIVE_CONVERGED);
            for (int32_t dy = -1; dilate && !active && dy <= 1; dy++)
                for (int32_t dx = -1; !active && dx <= 1; dx++) {
                    const int32_t nx = x + dx, ny = y + dy;
                    if ((dx || dy) && nx >= 0 && ny >= 0 && nx < sub_w && ny < sub_h)
                        active = !(flags[(size_t)ny * sub_w + nx] & (RT_ADAPTIVE_CONVERGED | RT_ADAPTIVE_CAPPED));
                }
            if (active) f |= RT_ADAPTIVE_ACTIVE;
        }
}

} // namespace rtamd

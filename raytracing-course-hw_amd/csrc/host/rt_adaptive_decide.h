// The decision of an adaptive slice (include/rtamd.h: rt_adaptive_render): which 8x8 sub-tiles of the frame go on drawing samples.
// One host function with no GPU call in it, shared by rtamd_adaptive.hip and the test hook rtt_adaptive_decide (test_hooks.hip);
// tests/adaptive_model.py restates it in numpy.  Below it, the host bookkeeping of a sub-tile that rt_adaptive and rt_view_adaptive
// (rtamd_view_adaptive.hip, per view and sub-tile) must do alike for their results to be the same bits: the refusals of the
// parameters, the monitor's numbers of a slice, the counts, the estimate's entry, the frame figures.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "../../../include/rtamd.h"
#include "../device/rt_types_adaptive.h" // AdTile, AD_NO_ESTIMATE

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

// What rt_adaptive_create and rt_view_adaptive_create refuse in an rt_adaptive_params whose struct_size and reserved word are in order:
// empty when it is usable, else the field and what is wrong with it (RT_ERR_INVALID_ARG).
inline std::string adaptive_params_refusal(const rt_adaptive_params &p) {
    if (!(p.target_noise > 0.f) || !std::isfinite(p.target_noise)) return "adaptive.target_noise must be positive and finite";
    if (p.min_batches < 0 || p.min_batches == 1) return "adaptive.min_batches must be at least 2 (0 = 4): the scatter of batch means needs 2";
    if (p.max_samples < 0) return "adaptive.max_samples must not be negative (0 = the sample-index limit)";
    if (p.flags & ~RT_ADAPTIVE_DILATE) return "adaptive.flags other than RT_ADAPTIVE_DILATE";
    return std::string();
}

// The monitor's numbers for a slice of n_samples over the sub-tiles of `list`, for each of n sub-tiles: the update's from before the slice,
// the estimate's from after it.  observed: N of the monitor per sub-tile.
inline void adaptive_slice_args(const rt_adaptive_tile *tiles, const int32_t *observed, size_t n, int32_t n_samples, const std::vector<uint32_t> &list,
                                std::vector<AdTileArgs> &args) {
    std::vector<bool> drawn(n, false);
    for (uint32_t t : list) drawn[t] = true;
    args.resize(n);
    for (size_t t = 0; t < n; t++) {
        const rt_adaptive_tile &T = tiles[t];
        const int32_t N = observed[t], d = drawn[t] ? n_samples : 0;
        AdTileArgs &A = args[t];
        A.n = (float)n_samples; A.N = (float)N; A.N1 = (float)(N + n_samples); A.first = N == 0;
        A.dof = (float)(T.batches + (drawn[t] ? 1 : 0) - 1); A.d = (float)(T.samples + d);
    }
}

// A sub-tile that a slice of n_samples drew for: one batch more.
inline void adaptive_count_slice(rt_adaptive_tile &T, int32_t &observed, int32_t n_samples) {
    T.samples += n_samples; T.batches += 1; observed += n_samples;
}

// The estimate kernel's entry of a sub-tile into its record: the sums, and NO_ESTIMATE by the mark the kernel leaves in `nonfinite`.
inline void adaptive_take_estimate(rt_adaptive_tile &T, const AdTile &e) {
    const bool none = e.nonfinite == AD_NO_ESTIMATE;
    T.sum_se2 = e.sum_se2; T.sum_luminance = e.sum_luminance; T.pixels = e.pixels; T.nonfinite = none ? 0u : e.nonfinite;
    T.flags = (T.flags & ~RT_ADAPTIVE_NO_ESTIMATE) | (none ? RT_ADAPTIVE_NO_ESTIMATE : 0u);
}

// Converged and capped sub-tiles and the smallest and largest count over n records: the stats of a slice.
inline void adaptive_tile_counts(const rt_adaptive_tile *tiles, size_t n, uint32_t &converged, uint32_t &capped, int32_t &min_samples, int32_t &max_samples) {
    int32_t lo = 0x7fffffff, hi = 0;
    for (size_t t = 0; t < n; t++) {
        if (tiles[t].flags & RT_ADAPTIVE_CONVERGED) converged++;
        if (tiles[t].flags & RT_ADAPTIVE_CAPPED) capped++;
        if (tiles[t].samples < lo) lo = tiles[t].samples;
        if (tiles[t].samples > hi) hi = tiles[t].samples;
    }
    min_samples = n ? lo : 0; max_samples = hi;
}

// Pixels of sub-tile t (row-major over sub_w columns) that lie inside a width x height image.
inline uint32_t adaptive_tile_pixels(uint32_t t, int32_t sub_w, int32_t width, int32_t height) {
    const int32_t gx = (int32_t)(t % (uint32_t)sub_w), gy = (int32_t)(t / (uint32_t)sub_w);
    const int32_t w = width - 8 * gx < 8 ? width - 8 * gx : 8, h = height - 8 * gy < 8 ? height - 8 * gy : 8;
    return (uint32_t)(w * h);
}

// The largest batches, observed samples and samples over n sub-tiles: what rt_adaptive_noise reports for them.
inline void adaptive_largest(const rt_adaptive_tile *tiles, const int32_t *observed, size_t n, int32_t &batches, int32_t &seen, int32_t &total) {
    batches = seen = total = 0;
    for (size_t t = 0; t < n; t++) {
        if (tiles[t].batches > batches) batches = tiles[t].batches;
        if (observed[t] > seen) seen = observed[t];
        if (tiles[t].samples > total) total = tiles[t].samples;
    }
}

// The frame figures of n sub-tiles' entries: noise_summarise's sums (rtamd_noise.hip), over the sub-tiles that have an estimate, in the
// frame's order.  batches, samples_observed and samples_total are the caller's.
inline void adaptive_summarise(const rt_adaptive_tile *tiles, size_t n, rt_noise_summary *s) {
    uint64_t pixels = 0, nonfinite = 0;
    double se2 = 0, lum = 0, worst = 0;
    for (size_t i = 0; i < n; i++) {
        const rt_adaptive_tile &t = tiles[i];
        if (t.flags & RT_ADAPTIVE_NO_ESTIMATE) continue;
        nonfinite += t.nonfinite;
        if (!t.pixels) continue;
        pixels += t.pixels;
        se2 += (double)t.sum_se2;
        lum += (double)t.sum_luminance;
        const double mean = (double)t.sum_se2 / (double)t.pixels;
        if (mean > worst) worst = mean;
    }
    s->pixels = pixels; s->nonfinite_pixels = nonfinite;
    s->mean_luminance = pixels ? lum / (double)pixels : 0.0;
    s->rms_error = pixels ? std::sqrt(se2 / (double)pixels) : 0.0;
    s->noise = s->mean_luminance != 0.0 ? s->rms_error / s->mean_luminance : 0.0;
    s->worst_tile_noise = s->mean_luminance != 0.0 ? std::sqrt(worst) / s->mean_luminance : 0.0;
}

} // namespace rtamd

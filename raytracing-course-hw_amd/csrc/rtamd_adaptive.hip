// Adaptive sampling through the C-ABI (include/rtamd.h: rt_adaptive_*), host side only: the object and its state, the refusals, the
// slice (gather, the persistent kernel's pixel source, scatter, update, estimate) over the query layer's chunk loop, and the decision
// (host/rt_adaptive_decide.h).  No kernel and no kernel header here: the kernels (device/rt_adaptive.h, device/rt_path_source.h) live in
// rtamd_api.hip and are launched through adaptive_launch_* and source_render.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "host/rt_scene.h"
#include "host/rt_adaptive_decide.h"
#include "device/rt_types_query.h"
#include "device/rt_types_adaptive.h"

using namespace rtamd;

static_assert(sizeof(rt_adaptive_tile) == 32 && sizeof(rt_adaptive_params) == 24, "the adaptive records as include/rtamd.h lays them out");

struct rt_adaptive {
    rt_scene *scene = nullptr;
    rt_render_params params{};          // as given to rt_adaptive_create
    rt_adaptive_params adaptive{};
    RenderView view{};                  // the real frame: geometry, n_pixslots, tan_fov_x
    int32_t sub_w = 0, sub_h = 0;
    uint32_t n_tiles = 0;
    uint32_t *d_state = nullptr;        // 24 bytes per pixel slot, rt_accum's layout
    float *d_stats = nullptr;           // y0, yp, m2: n_pixslots floats each
    AdTile *d_tiles = nullptr;          // n_tiles
    AdTileArgs *d_args = nullptr;       // n_tiles
    float *d_inv = nullptr;             // n_tiles
    uint32_t *d_list = nullptr;         // n_tiles
    uint32_t *d_strip = nullptr;        // one chunk's strip: 24 bytes per slot, then its pixel words
    size_t strip_cap = 0;               // slots
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the gather and the scatter of a chunk
    std::vector<rt_adaptive_tile> tiles; // samples, batches, the last estimate's entry, flags
    std::vector<int32_t> observed;      // N of the monitor, per sub-tile
    std::string broken;
    ~rt_adaptive() {
        for (void *p : {(void *)d_state, (void *)d_stats, (void *)d_tiles, (void *)d_args, (void *)d_inv, (void *)d_list, (void *)d_strip})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

AdaptiveView adaptive_view(const rt_adaptive *a) {
    AdaptiveView V{};
    const size_t slots = a->view.n_pixslots;
    V.state = a->d_state; V.n_pixslots = a->view.n_pixslots;
    V.y0 = a->d_stats; V.yp = a->d_stats + slots; V.m2 = a->d_stats + 2 * slots;
    V.args = a->d_args; V.inv_samples = a->d_inv; V.tiles = a->d_tiles; V.list = a->d_list;
    return V;
}

int usable(const rt_adaptive *a, const std::string &who) {
    if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "an earlier slice failed and left the state half advanced (" + a->broken + ")");
    return RT_OK;
}

void decide(rt_adaptive *a, int32_t n_samples) {
    std::vector<uint32_t> flags(a->n_tiles);
    adaptive_decide(a->tiles.data(), a->adaptive, a->sub_w, a->sub_h, n_samples, flags.data());
    for (uint32_t t = 0; t < a->n_tiles; t++) a->tiles[t].flags = flags[t];
}

// What a slice over `list` refuses before anything is launched.
int check_slice(const rt_adaptive *a, int32_t n_samples, const std::vector<uint32_t> &list, const std::string &who) {
    if (n_samples <= 0) return fail(RT_ERR_INVALID_ARG, who + "n_samples must be positive");
    if (n_samples >= ADAPTIVE_SAMPLE_LIMIT) return fail(RT_ERR_LIMIT, who + "n_samples does not fit the path records' sample index (below " + std::to_string(ADAPTIVE_SAMPLE_LIMIT) + ")");
    for (uint32_t t : list)
        if ((int64_t)a->tiles[t].samples + n_samples >= (int64_t)ADAPTIVE_SAMPLE_LIMIT)
            return fail(RT_ERR_LIMIT, who + "sub-tile " + std::to_string(t) + ": " + std::to_string(a->tiles[t].samples) + " + " + std::to_string(n_samples) +
                                          " samples per pixel do not fit the path records' sample index (below " + std::to_string(ADAPTIVE_SAMPLE_LIMIT) + ")");
    if (list.empty()) return RT_OK;
    return source_check(a->scene, (uint32_t)std::min((size_t)list.size() * 64u, source_chunk_slots()), a->view.ray_depth, n_samples, who);
}

// One slice of n_samples for the sub-tiles of `list` (ascending), then the update over the list and the estimate over the frame.
int slice(rt_adaptive *a, int32_t n_samples, const std::vector<uint32_t> &list, rt_adaptive_stats &st, const std::string &who) {
    rt_scene *scene = a->scene;
    hipStream_t stream = (hipStream_t)a->params.stream;
    st.active_tiles = (uint32_t)list.size();
    if (list.empty()) return RT_OK;
    std::vector<AdTileArgs> args;
    adaptive_slice_args(a->tiles.data(), a->observed.data(), a->n_tiles, n_samples, list, args);
    std::vector<bool> drawn(a->n_tiles, false);
    for (uint32_t t : list) drawn[t] = true;
    HIP_CHECK(hipMemcpyAsync(a->d_args, args.data(), args.size() * sizeof(AdTileArgs), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(a->d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    const size_t chunk_tiles = std::max<size_t>(1u, source_chunk_slots() / 64u);
    const size_t cap = std::min(list.size(), chunk_tiles) * 64u;
    if (a->strip_cap < cap) {
        if (a->d_strip) (void)hipFree(a->d_strip);
        a->d_strip = nullptr; a->strip_cap = 0;
        HIP_CHECK(hipMalloc((void **)&a->d_strip, cap * 28u));
        a->strip_cap = cap;
    }
    const int rc = source_chunks(list.size(), chunk_tiles, stream, [&](size_t first, size_t m) -> int {
        AdaptiveView V = adaptive_view(a);
        V.list = a->d_list + first; V.n_list = (uint32_t)m;
        V.strip = a->d_strip; V.strip_slots = (uint32_t)m * 64u; V.pixels = a->d_strip + 6 * (size_t)V.strip_slots;
        HIP_CHECK(hipEventRecord(a->ev[0], stream));
        st.launches += adaptive_launch_gather(scene, a->view, V, stream);
        HIP_CHECK(hipEventRecord(a->ev[1], stream));
        SourceChunk C{};
        C.mode = 4u; C.n = V.strip_slots; C.streams = 1u;
        C.ray_depth = a->view.ray_depth; C.samples = n_samples; C.state = V.strip;
        C.pixels = V.pixels; C.frame_w = a->view.width; C.frame_h = a->view.height;
        SourceResult res{};
        if (const int rc = source_render(scene, C, stream, res, who)) return rc;
        HIP_CHECK(hipEventRecord(a->ev[2], stream));
        st.launches += res.launches + adaptive_launch_scatter(scene, a->view, V, stream);
        HIP_CHECK(hipEventRecord(a->ev[3], stream));
        HIP_CHECK(hipEventSynchronize(a->ev[3]));
        float g = 0.f, s = 0.f;
        HIP_CHECK(hipEventElapsedTime(&g, a->ev[0], a->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&s, a->ev[2], a->ev[3]));
        st.gather_ms += g; st.scatter_ms += s; st.kernel_ms += res.kernel_ms;
        st.exact_walks += res.exact_walks; st.reference_exact = res.reference_exact;
        return RT_OK;
    });
    if (rc != RT_OK) return rc;
    AdaptiveView V = adaptive_view(a);
    V.n_list = (uint32_t)list.size();
    st.launches += adaptive_launch_update(scene, a->view, V, stream);
    st.launches += adaptive_launch_estimate(scene, a->view, V, stream);
    std::vector<AdTile> est(a->n_tiles);
    HIP_CHECK(hipMemcpyAsync(est.data(), a->d_tiles, est.size() * sizeof(AdTile), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint32_t t = 0; t < a->n_tiles; t++) {
        if (drawn[t]) {
            adaptive_count_slice(a->tiles[t], a->observed[t], n_samples);
            st.samples += (uint64_t)adaptive_tile_pixels(t, a->sub_w, a->view.width, a->view.height) * (uint64_t)n_samples;
        }
        adaptive_take_estimate(a->tiles[t], est[t]);
    }
    return RT_OK;
}

// rt_adaptive_render (mask == null: the policy) and rt_adaptive_render_tiles
int render(rt_adaptive *a, int32_t n_samples, const uint8_t *mask, rt_adaptive_stats *stats, const std::string &who) {
    if (stats && stats->struct_size != sizeof(rt_adaptive_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        const double t0 = now_ms();
        std::vector<uint32_t> list;
        if (mask) {
            for (uint32_t t = 0; t < a->n_tiles; t++) if (mask[t]) list.push_back(t);
        } else if (n_samples > 0) { // the cap depends on this call's slice length; CONVERGED is sticky and the entries are the last estimate's
            std::vector<uint32_t> flags(a->n_tiles);
            adaptive_decide(a->tiles.data(), a->adaptive, a->sub_w, a->sub_h, n_samples, flags.data());
            for (uint32_t t = 0; t < a->n_tiles; t++) if (flags[t] & RT_ADAPTIVE_ACTIVE) list.push_back(t);
        }
        if (const int rc = check_slice(a, n_samples, list, who)) return rc;
        HIP_CHECK(hipSetDevice(a->scene->device));
        rt_adaptive_stats st{};
        st.struct_size = sizeof(rt_adaptive_stats);
        st.reference_exact = a->scene->view.exact_boxes == 1u ? 1u : 0u;
        const int rc = guarded(who, [&]() -> int { return slice(a, n_samples, list, st, who); });
        if (rc != RT_OK) { a->broken = rt_last_error(); return rc; } // the slice failed under way (a refusal or a HIP error): the state is half advanced
        if (!mask) decide(a, n_samples);
        adaptive_tile_counts(a->tiles.data(), a->tiles.size(), st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples);
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

} // namespace

extern "C" {

int rt_adaptive_create(rt_scene *scene, const rt_render_params *p, const rt_adaptive_params *ap, rt_adaptive **out) {
    const std::string who = "rt_adaptive_create: ";
    if (!scene || !p || !ap || !out) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    *out = nullptr;
    return guarded(who, [&]() -> int {
        if (p->struct_size != sizeof(rt_render_params)) return fail(RT_ERR_INVALID_ARG, who + "params.struct_size mismatch (ABI skew)");
        if (ap->struct_size != sizeof(rt_adaptive_params)) return fail(RT_ERR_INVALID_ARG, who + "adaptive.struct_size mismatch (ABI skew)");
        if (p->reserved != 0 || ap->reserved != 0) return fail(RT_ERR_INVALID_ARG, who + "reserved must be 0");
        if (const std::string why = adaptive_params_refusal(*ap); !why.empty()) return fail(RT_ERR_INVALID_ARG, who + why);
        if (p->integrator != RT_INTEGRATOR_HW8 || scene->flavor != RT_INTEGRATOR_HW8)
            return fail(RT_ERR_UNSUPPORTED, who + "adaptive sampling runs the persistent hw8 kernel: RT_INTEGRATOR_HW8 on a scene created for it only (integrator " +
                                            std::to_string(p->integrator) + ", scene prepared for " + std::to_string(scene->flavor) + "); there is no fallback");
        if (p->shard_count > 1) return fail(RT_ERR_UNSUPPORTED, who + "shard_count > 1: an adaptive frame is unsharded (rt_multi_* is out of scope)");
        if (p->sample_streams > 1) return fail(RT_ERR_UNSUPPORTED, who + "throughput mode (sample_streams > 1) has no resumable state");
        if (p->flags != 0) return fail(RT_ERR_UNSUPPORTED, who + "render flags other than 0 do not apply to an adaptive render (the outputs are named at rt_adaptive_resolve)");
        std::unique_ptr<rt_adaptive> a(new rt_adaptive);
        rt_render_params q = *p;
        q.samples = 1; // ignored here
        std::string err;
        if (!resolve_tiles(&q, a->view, err)) return fail(RT_ERR_INVALID_ARG, who + err);
        if (a->view.width > 65535 || a->view.height > 65535) return fail(RT_ERR_LIMIT, who + "width and height must stay below 65,536 (a slot's pixel is one packed word)");
        const uint64_t n_tiles = (uint64_t)a->view.tiles_x * (uint64_t)a->view.tiles_y;
        if (n_tiles * 64u >= 0x40000000ull) return fail(RT_ERR_LIMIT, who + "too many pixel slots");
        a->scene = scene; a->params = *p; a->params.samples = 0; a->adaptive = *ap;
        a->sub_w = a->view.tiles_x; a->sub_h = a->view.tiles_y; a->n_tiles = (uint32_t)n_tiles;
        a->view.n_pixslots = a->n_tiles * 64u;
        a->view.tan_fov_x = adaptive_tan_fov_x(scene, a->view.width, a->view.height);
        if (const int rc = source_check(scene, (uint32_t)std::min((size_t)a->view.n_pixslots, source_chunk_slots()), a->view.ray_depth, 1, who)) return rc;
        HIP_CHECK(hipSetDevice(scene->device));
        hipStream_t stream = (hipStream_t)p->stream;
        const size_t slots = a->view.n_pixslots;
        HIP_CHECK(hipMalloc((void **)&a->d_state, slots * 24u));
        HIP_CHECK(hipMalloc((void **)&a->d_stats, 3 * slots * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&a->d_tiles, a->n_tiles * sizeof(AdTile)));
        HIP_CHECK(hipMalloc((void **)&a->d_args, a->n_tiles * sizeof(AdTileArgs)));
        HIP_CHECK(hipMalloc((void **)&a->d_inv, a->n_tiles * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&a->d_list, a->n_tiles * sizeof(uint32_t)));
        for (hipEvent_t &e : a->ev) HIP_CHECK(hipEventCreate(&e));
        // a fresh state; the monitor's snapshot of it is y0 = yp = Y(0) = 0, m2 = 0
        HIP_CHECK(hipMemsetAsync(a->d_stats, 0, 3 * slots * sizeof(float), stream));
        RenderView R = a->view;
        R.accum = a->d_state;
        adaptive_launch_seed(scene, R, stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        rt_adaptive_tile fresh{};
        fresh.flags = RT_ADAPTIVE_ACTIVE | RT_ADAPTIVE_NO_ESTIMATE;
        a->tiles.assign(a->n_tiles, fresh);
        a->observed.assign(a->n_tiles, 0);
        *out = a.release();
        return RT_OK;
    });
}

void rt_adaptive_destroy(rt_adaptive *a) {
    if (a) (void)hipSetDevice(a->scene->device);
    delete a;
}

int rt_adaptive_render(rt_adaptive *a, int32_t n_samples, rt_adaptive_stats *stats) {
    return render(a, n_samples, nullptr, stats, "rt_adaptive_render: ");
}

int rt_adaptive_render_tiles(rt_adaptive *a, int32_t n_samples, const uint8_t *mask, rt_adaptive_stats *stats) {
    if (a && !mask) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_render_tiles: null argument (mask)");
    return render(a, n_samples, mask, stats, "rt_adaptive_render_tiles: ");
}

int rt_adaptive_tiles(rt_adaptive *a, rt_adaptive_tile *out) {
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_tiles: null argument");
    return guarded("rt_adaptive_tiles: ", [&]() -> int {
        if (const int rc = usable(a, "rt_adaptive_tiles: ")) return rc;
        memcpy(out, a->tiles.data(), a->tiles.size() * sizeof(rt_adaptive_tile));
        return RT_OK;
    });
}

int rt_adaptive_sample_map(rt_adaptive *a, int32_t *out) {
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_sample_map: null argument");
    return guarded("rt_adaptive_sample_map: ", [&]() -> int {
        if (const int rc = usable(a, "rt_adaptive_sample_map: ")) return rc;
        const int32_t W = a->view.width, H = a->view.height;
        for (int32_t y = 0; y < H; y++)
            for (int32_t x = 0; x < W; x++) out[(size_t)y * W + x] = a->tiles[(size_t)(y >> 3) * a->sub_w + (x >> 3)].samples;
        return RT_OK;
    });
}

int rt_adaptive_resolve(rt_adaptive *a, uint32_t flags, float *out_rgb, uint8_t *out_rgb8) {
    const std::string who = "rt_adaptive_resolve: ";
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_FLAG_OUT_DEVICE");
        if (!out_rgb && !out_rgb8) return RT_OK;
        HIP_CHECK(hipSetDevice(a->scene->device));
        hipStream_t stream = (hipStream_t)a->params.stream;
        std::vector<float> inv(a->n_tiles);
        for (uint32_t t = 0; t < a->n_tiles; t++) inv[t] = a->tiles[t].samples > 0 ? (float)(1.0 / a->tiles[t].samples) : 0.f; // scene.cpp:176, as rt_render(samples = d) evaluates it
        HIP_CHECK(hipMemcpyAsync(a->d_inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        RenderView R = a->view;
        const size_t elems = (size_t)R.width * R.height * 3;
        StagedOut rgb(out_rgb, flags, elems, sizeof(float)), rgb8(out_rgb8, flags, elems, 1);
        R.out_rgb = (float *)rgb.dev; R.out_rgb8 = (uint8_t *)rgb8.dev;
        R.accum = a->d_state;
        adaptive_launch_resolve(a->scene, R, adaptive_view(a), stream);
        rgb.copy_back(stream);
        rgb8.copy_back(stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        return RT_OK;
    });
}

int rt_adaptive_noise(rt_adaptive *a, uint32_t flags, float *out_se, rt_noise_summary *summary) {
    const std::string who = "rt_adaptive_noise: ";
    if (summary && summary->struct_size != sizeof(rt_noise_summary)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_FLAG_OUT_DEVICE");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        int32_t batches = 0, observed = 0, total = 0;
        adaptive_largest(a->tiles.data(), a->observed.data(), a->n_tiles, batches, observed, total);
        if (batches < 2) return fail(RT_ERR_INVALID_ARG, who + "no sub-tile has 2 batches yet (" + std::to_string(batches) + " at most): the scatter of batch means needs at least 2");
        if (out_se) { // the map: the estimate once more, with the numbers of the state as it stands
            HIP_CHECK(hipSetDevice(a->scene->device));
            hipStream_t stream = (hipStream_t)a->params.stream;
            std::vector<AdTileArgs> args(a->n_tiles);
            for (uint32_t t = 0; t < a->n_tiles; t++) { args[t] = AdTileArgs{}; args[t].dof = (float)(a->tiles[t].batches - 1); args[t].d = (float)a->tiles[t].samples; }
            HIP_CHECK(hipMemcpyAsync(a->d_args, args.data(), args.size() * sizeof(AdTileArgs), hipMemcpyHostToDevice, stream));
            StagedOut se(out_se, flags, (size_t)a->view.width * a->view.height, sizeof(float));
            AdaptiveView V = adaptive_view(a);
            V.out_se = (float *)se.dev;
            adaptive_launch_estimate(a->scene, a->view, V, stream);
            se.copy_back(stream);
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        if (summary) {
            summary->batches = batches; summary->samples_observed = observed; summary->samples_total = total;
            adaptive_summarise(a->tiles.data(), a->tiles.size(), summary);
        }
        return RT_OK;
    });
}

} // extern "C"

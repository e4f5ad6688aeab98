// Adaptive sampling for view sets through the C-ABI (include/rtamd.h: rt_view_adaptive_*), host side only: the object and its state, the
// refusals, the slice (gather, the persistent kernel's view source, scatter per chunk; then one update and one estimate for the whole
// set) over the query layer's chunk loop, and the decision per view (host/rt_view_adaptive_plan.h).  No kernel and no kernel header
// here: the kernels (device/rt_view_adaptive.h, device/rt_path_source.h) live in rtamd_api.hip and are launched through
// view_adaptive_launch_* and source_render.  The scene is only read: a view's camera lives in the set's own record array.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "host/rt_scene.h"
#include "host/rt_views_camera.h"
#include "host/rt_view_adaptive_plan.h"
#include "device/rt_types_query.h"
#include "device/rt_types_views.h" // views_launch_seed: a view's block is seeded as a view set's
#include "device/rt_types_view_adaptive.h"

using namespace rtamd;

static_assert(sizeof(rt_view_adaptive_stats) == 96, "the stats record as include/rtamd.h lays it out");

struct rt_view_adaptive {
    rt_scene *scene = nullptr;
    hipStream_t stream = nullptr;
    rt_adaptive_params adaptive{};
    RenderView view{};                  // one view's frame: geometry, n_pixslots, ray_depth
    int32_t sub_w = 0, sub_h = 0, n_views = 0;
    uint32_t tiles = 0;                 // 8x8 sub-tiles of a view
    size_t n = 0;                       // n_views * tiles: the words G
    uint32_t *d_state = nullptr;        // n_views blocks of 24 bytes per pixel slot (rt_types_views.h)
    float *d_planes = nullptr;          // n_views blocks of y0, yp, m2
    ViewCamera *d_cameras = nullptr;    // n_views
    AdTile *d_entries = nullptr;        // n
    AdTileArgs *d_args = nullptr;       // n
    float *d_inv = nullptr;             // n
    uint32_t *d_list = nullptr;         // n
    uint32_t *d_strip = nullptr;        // one chunk's strip: 24 bytes per slot, its pixel words, a view word per 64 slots
    size_t strip_cap = 0;               // slots
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // around gather, scatter and the two noise launches
    std::vector<rt_adaptive_tile> entries; // n: samples, batches, the last estimate's entry, flags
    std::vector<int32_t> observed;      // n: N of the monitor
    std::string broken;
    ~rt_view_adaptive() {
        for (void *p : {(void *)d_state, (void *)d_planes, (void *)d_cameras, (void *)d_entries, (void *)d_args, (void *)d_inv, (void *)d_list, (void *)d_strip})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

ViewAdaptiveView device_view(const rt_view_adaptive *a) {
    ViewAdaptiveView V{};
    V.state = a->d_state; V.planes = a->d_planes; V.vslots = a->view.n_pixslots; V.tiles = a->tiles;
    V.list = a->d_list; V.args = a->d_args; V.inv_samples = a->d_inv; V.entries = a->d_entries;
    return V;
}

int usable(const rt_view_adaptive *a, const std::string &who) {
    if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "an earlier slice failed and left the state half advanced (" + a->broken + ")");
    return RT_OK;
}

int check_view(const rt_view_adaptive *a, int32_t view, const std::string &who) {
    if (view < 0 || view >= a->n_views) return fail(RT_ERR_INVALID_ARG, who + "view (" + std::to_string(view) + ") is no view of the set's " + std::to_string(a->n_views));
    return RT_OK;
}

int check_cameras(const rt_camera *cameras, int32_t first, int32_t n, const std::string &who) {
    const std::string why = views_cameras_check(cameras, first, n);
    return why.empty() ? RT_OK : fail(RT_ERR_INVALID_ARG, who + why);
}

// Views first .. first + n - 1 get `cameras` and a fresh state: sums 0, engines reseeded, planes 0, every sub-tile ACTIVE | NO_ESTIMATE.
void reset_views(rt_view_adaptive *a, int32_t first, int32_t n, const rt_camera *cameras) {
    const size_t slots = a->view.n_pixslots;
    std::vector<ViewCamera> rec((size_t)n);
    for (int32_t i = 0; i < n; i++) rec[(size_t)i] = views_camera_record(cameras[i], a->view.width, a->view.height);
    HIP_CHECK(hipMemcpyAsync(a->d_cameras + first, rec.data(), rec.size() * sizeof(ViewCamera), hipMemcpyHostToDevice, a->stream));
    HIP_CHECK(hipMemsetAsync(a->d_planes + 3 * (size_t)first * slots, 0, 3 * (size_t)n * slots * sizeof(float), a->stream)); // y0 = yp = Y(0) = 0, m2 = 0
    rt_adaptive_tile fresh{};
    fresh.flags = RT_ADAPTIVE_ACTIVE | RT_ADAPTIVE_NO_ESTIMATE;
    for (int32_t i = first; i < first + n; i++) {
        RenderView R = a->view;
        R.accum = a->d_state + 6 * (size_t)i * slots;
        views_launch_seed(a->scene, R, a->stream);
        std::fill_n(a->entries.begin() + (size_t)i * a->tiles, a->tiles, fresh);
        std::fill_n(a->observed.begin() + (size_t)i * a->tiles, a->tiles, 0);
    }
    HIP_CHECK(hipStreamSynchronize(a->stream)); // `rec` is pageable memory of this call
}

// The stored flags of the views that take part become those of the decision for a slice of n_samples.
void decide(rt_view_adaptive *a, int32_t n_samples, const uint8_t *view_mask) {
    std::vector<uint32_t> flags(a->n);
    view_adaptive_decide(a->entries.data(), a->adaptive, a->sub_w, a->sub_h, a->n_views, n_samples, view_mask, flags.data());
    for (size_t G = 0; G < a->n; G++) a->entries[G].flags = flags[G];
}

// What a slice over `list` refuses before anything is launched.
int check_slice(const rt_view_adaptive *a, int32_t n_samples, const std::vector<uint32_t> &list, const std::string &who) {
    if (n_samples <= 0) return fail(RT_ERR_INVALID_ARG, who + "n_samples must be positive");
    if (n_samples >= ADAPTIVE_SAMPLE_LIMIT) return fail(RT_ERR_LIMIT, who + "n_samples does not fit the path records' sample index (below " + std::to_string(ADAPTIVE_SAMPLE_LIMIT) + ")");
    for (uint32_t G : list)
        if ((int64_t)a->entries[G].samples + n_samples >= (int64_t)ADAPTIVE_SAMPLE_LIMIT)
            return fail(RT_ERR_LIMIT, who + "n_samples: view " + std::to_string(G / a->tiles) + " sub-tile " + std::to_string(G % a->tiles) + ": " + std::to_string(a->entries[G].samples) +
                                          " + " + std::to_string(n_samples) + " samples per pixel do not fit the path records' sample index (below " + std::to_string(ADAPTIVE_SAMPLE_LIMIT) + ")");
    if (list.empty()) return RT_OK;
    return source_check(a->scene, (uint32_t)std::min((size_t)list.size() * 64u, source_chunk_slots()), a->view.ray_depth, n_samples, who);
}

// One slice of n_samples for the sub-tiles of `list` (ascending words G), then one update over the list and one estimate over the set.
int slice(rt_view_adaptive *a, int32_t n_samples, const std::vector<uint32_t> &list, rt_view_adaptive_stats &st, const std::string &who) {
    rt_scene *scene = a->scene;
    hipStream_t stream = a->stream;
    st.active_tiles = (uint32_t)list.size();
    if (list.empty()) return RT_OK;
    std::vector<AdTileArgs> args;
    adaptive_slice_args(a->entries.data(), a->observed.data(), a->n, n_samples, list, args);
    HIP_CHECK(hipMemcpyAsync(a->d_args, args.data(), args.size() * sizeof(AdTileArgs), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(a->d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    const size_t chunk_tiles = std::max<size_t>(1u, source_chunk_slots() / 64u);
    const size_t cap = std::min(list.size(), chunk_tiles) * 64u;
    if (a->strip_cap < cap) {
        if (a->d_strip) (void)hipFree(a->d_strip);
        a->d_strip = nullptr; a->strip_cap = 0;
        HIP_CHECK(hipMalloc((void **)&a->d_strip, cap * 28u + cap / 64u * 4u));
        a->strip_cap = cap;
    }
    const int rc = source_chunks(list.size(), chunk_tiles, stream, [&](size_t first, size_t m) -> int {
        ViewAdaptiveView V = device_view(a);
        V.list = a->d_list + first; V.n_list = (uint32_t)m;
        V.strip = a->d_strip; V.strip_slots = (uint32_t)m * 64u; V.pixels = a->d_strip + 6 * (size_t)V.strip_slots;
        HIP_CHECK(hipEventRecord(a->ev[0], stream));
        st.launches += view_adaptive_launch_gather(scene, a->view, V, stream);
        HIP_CHECK(hipEventRecord(a->ev[1], stream));
        SourceChunk C{};
        C.mode = 5u; C.n = V.strip_slots; C.streams = 1u;
        C.ray_depth = a->view.ray_depth; C.samples = n_samples; C.state = V.strip;
        C.pixels = V.pixels; C.frame_w = a->view.width; C.frame_h = a->view.height; C.cameras = a->d_cameras;
        SourceResult res{};
        if (const int rc = source_render(scene, C, stream, res, who)) return rc;
        HIP_CHECK(hipEventRecord(a->ev[2], stream));
        st.launches += res.launches + view_adaptive_launch_scatter(scene, a->view, V, stream);
        HIP_CHECK(hipEventRecord(a->ev[3], stream));
        HIP_CHECK(hipEventSynchronize(a->ev[3]));
        float g = 0.f, s = 0.f;
        HIP_CHECK(hipEventElapsedTime(&g, a->ev[0], a->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&s, a->ev[2], a->ev[3]));
        st.gather_ms += g; st.scatter_ms += s; st.kernel_ms += res.kernel_ms;
        st.exact_walks += res.exact_walks; st.reference_exact = res.reference_exact;
        return RT_OK;
    });
    if (rc != RT_OK) { (void)hipStreamSynchronize(stream); return rc; } // `args` and `list` are pageable memory of this call
    ViewAdaptiveView V = device_view(a);
    V.n_list = (uint32_t)list.size();
    V.first = 0u; V.count = (uint32_t)a->n;
    HIP_CHECK(hipEventRecord(a->ev[4], stream));
    st.launches += view_adaptive_launch_update(scene, a->view, V, stream);
    st.launches += view_adaptive_launch_estimate(scene, a->view, V, stream);
    HIP_CHECK(hipEventRecord(a->ev[5], stream));
    std::vector<AdTile> est(a->n);
    HIP_CHECK(hipMemcpyAsync(est.data(), a->d_entries, est.size() * sizeof(AdTile), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    float noise = 0.f;
    HIP_CHECK(hipEventElapsedTime(&noise, a->ev[4], a->ev[5]));
    st.noise_ms += noise;
    std::vector<bool> view_drew((size_t)a->n_views, false);
    for (uint32_t G : list) {
        adaptive_count_slice(a->entries[G], a->observed[G], n_samples);
        st.samples += (uint64_t)adaptive_tile_pixels(G % a->tiles, a->sub_w, a->view.width, a->view.height) * (uint64_t)n_samples;
        view_drew[G / a->tiles] = true;
    }
    for (int32_t v = 0; v < a->n_views; v++) {
        if (!view_drew[(size_t)v]) continue; // a view that drew nothing has the state it had: its entries are left as they were
        st.active_views++;
        for (size_t G = (size_t)v * a->tiles; G < (size_t)(v + 1) * a->tiles; G++) adaptive_take_estimate(a->entries[G], est[G]);
    }
    return RT_OK;
}

// rt_view_adaptive_render (tile_mask == null: the policy, over the views of view_mask) and rt_view_adaptive_render_tiles
int render(rt_view_adaptive *a, int32_t n_samples, const uint8_t *view_mask, const uint8_t *tile_mask, rt_view_adaptive_stats *stats, const std::string &who) {
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        const double t0 = now_ms();
        std::vector<uint32_t> list;
        if (tile_mask) view_adaptive_list_tiles(tile_mask, a->n, list);
        else if (n_samples > 0) { // the cap depends on this call's slice length; CONVERGED is sticky and the entries are the last estimate's
            std::vector<uint32_t> flags(a->n);
            view_adaptive_decide(a->entries.data(), a->adaptive, a->sub_w, a->sub_h, a->n_views, n_samples, view_mask, flags.data());
            view_adaptive_list_policy(flags.data(), a->tiles, a->n_views, view_mask, list);
        }
        if (const int rc = check_slice(a, n_samples, list, who)) return rc;
        HIP_CHECK(hipSetDevice(a->scene->device));
        rt_view_adaptive_stats st{};
        st.struct_size = sizeof(rt_view_adaptive_stats);
        st.reference_exact = a->scene->view.exact_boxes == 1u ? 1u : 0u;
        const int rc = guarded(who, [&]() -> int { return slice(a, n_samples, list, st, who); });
        if (rc != RT_OK) { a->broken = rt_last_error(); return rc; } // the slice failed under way (a refusal or a HIP error): the state is half advanced
        if (!tile_mask) decide(a, n_samples, view_mask);
        adaptive_tile_counts(a->entries.data(), a->n, st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples);
        st.total_ms = now_ms() - t0;
        *stats = st;
        return RT_OK;
    });
}

} // namespace

extern "C" {

int rt_view_adaptive_create(rt_scene *scene, const rt_views_params *p, const rt_adaptive_params *ap, const rt_camera *cameras, rt_view_adaptive **out) {
    const std::string who = "rt_view_adaptive_create: ";
    if (p && p->struct_size != sizeof(rt_views_params)) return fail(RT_ERR_INVALID_ARG, who + "params.struct_size mismatch (ABI skew)");
    if (ap && ap->struct_size != sizeof(rt_adaptive_params)) return fail(RT_ERR_INVALID_ARG, who + "adaptive.struct_size mismatch (ABI skew)");
    if (!scene || !p || !ap || !cameras || !out) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    *out = nullptr;
    return guarded(who, [&]() -> int {
        if (p->flags != 0) return fail(RT_ERR_INVALID_ARG, who + "params.flags must be 0");
        if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(RT_ERR_INVALID_ARG, who + "params.reserved must be 0");
        if (ap->reserved != 0) return fail(RT_ERR_INVALID_ARG, who + "adaptive.reserved must be 0");
        if (const std::string why = adaptive_params_refusal(*ap); !why.empty()) return fail(RT_ERR_INVALID_ARG, who + why);
        if (p->n_views < 1) return fail(RT_ERR_INVALID_ARG, who + "params.n_views must be at least 1");
        if (p->width < 1 || p->height < 1) return fail(RT_ERR_INVALID_ARG, who + "params.width and params.height must be at least 1");
        if (p->width > 65535 || p->height > 65535) return fail(RT_ERR_LIMIT, who + "params.width and params.height must stay below 65,536 (a slot's pixel is one packed word)");
        if (p->ray_depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "params.ray_depth above RT_MAX_DEPTH (16)");
        const uint64_t tiles = (uint64_t)((p->width + 7) / 8) * (uint64_t)((p->height + 7) / 8); // 64 pixel slots each
        if (tiles * 64u * (uint64_t)p->n_views >= 0x80000000ull)
            return fail(RT_ERR_LIMIT, who + "params.n_views: " + std::to_string(p->n_views) + " views of " + std::to_string(tiles * 64u) + " pixel slots each do not stay below 2^31 slots");
        std::unique_ptr<rt_view_adaptive> a(new rt_view_adaptive);
        rt_render_params q{};
        q.struct_size = sizeof q; q.width = p->width; q.height = p->height; q.samples = 1; q.ray_depth = p->ray_depth; q.integrator = RT_INTEGRATOR_HW8;
        std::string err;
        if (!resolve_tiles(&q, a->view, err)) return fail(RT_ERR_INVALID_ARG, who + err);
        if (scene->flavor != RT_INTEGRATOR_HW8)
            return fail(RT_ERR_UNSUPPORTED, who + "an adaptive view set runs the persistent hw8 kernel: a scene created for RT_INTEGRATOR_HW8 only (scene prepared for " +
                                            std::to_string(scene->flavor) + "); there is no fallback");
        if (const int rc = check_cameras(cameras, 0, p->n_views, who)) return rc;
        a->scene = scene; a->stream = (hipStream_t)p->stream; a->n_views = p->n_views; a->adaptive = *ap;
        a->sub_w = a->view.tiles_x; a->sub_h = a->view.tiles_y;
        a->tiles = (uint32_t)tiles; a->n = (size_t)tiles * (size_t)p->n_views;
        a->view.n_pixslots = a->tiles * 64u;
        if (const int rc = source_check(scene, (uint32_t)std::min(a->n * 64u, source_chunk_slots()), a->view.ray_depth, 1, who)) return rc;
        HIP_CHECK(hipSetDevice(scene->device));
        const size_t slots = (size_t)a->view.n_pixslots * (size_t)p->n_views;
        HIP_CHECK(hipMalloc((void **)&a->d_state, slots * 24u));
        HIP_CHECK(hipMalloc((void **)&a->d_planes, slots * 3u * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&a->d_cameras, (size_t)p->n_views * sizeof(ViewCamera)));
        HIP_CHECK(hipMalloc((void **)&a->d_entries, a->n * sizeof(AdTile)));
        HIP_CHECK(hipMalloc((void **)&a->d_args, a->n * sizeof(AdTileArgs)));
        HIP_CHECK(hipMalloc((void **)&a->d_inv, a->n * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&a->d_list, a->n * sizeof(uint32_t)));
        for (hipEvent_t &e : a->ev) HIP_CHECK(hipEventCreate(&e));
        a->entries.assign(a->n, rt_adaptive_tile{});
        a->observed.assign(a->n, 0);
        reset_views(a.get(), 0, p->n_views, cameras);
        *out = a.release();
        return RT_OK;
    });
}

void rt_view_adaptive_destroy(rt_view_adaptive *a) {
    if (a) (void)hipSetDevice(a->scene->device);
    delete a;
}

int rt_view_adaptive_set_cameras(rt_view_adaptive *a, int32_t first, int32_t n, const rt_camera *cameras) {
    const std::string who = "rt_view_adaptive_set_cameras: ";
    if (!a || !cameras) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (first < 0 || first >= a->n_views) return fail(RT_ERR_INVALID_ARG, who + "first (" + std::to_string(first) + ") is no view of the set's " + std::to_string(a->n_views));
        if (n < 1 || n > a->n_views - first) return fail(RT_ERR_INVALID_ARG, who + "n (" + std::to_string(n) + ") must be 1 .. " + std::to_string(a->n_views - first) + " from view " + std::to_string(first));
        if (const int rc = check_cameras(cameras, first, n, who)) return rc;
        HIP_CHECK(hipSetDevice(a->scene->device));
        const int rc = guarded(who, [&]() -> int { reset_views(a, first, n, cameras); return RT_OK; });
        if (rc != RT_OK) a->broken = rt_last_error();
        return rc;
    });
}

int rt_view_adaptive_render(rt_view_adaptive *a, int32_t n_samples, const uint8_t *view_mask, rt_view_adaptive_stats *stats) {
    const std::string who = "rt_view_adaptive_render: ";
    if (stats && stats->struct_size != sizeof(rt_view_adaptive_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (!a || !stats) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return render(a, n_samples, view_mask, nullptr, stats, who);
}

int rt_view_adaptive_render_tiles(rt_view_adaptive *a, int32_t n_samples, const uint8_t *tile_mask, rt_view_adaptive_stats *stats) {
    const std::string who = "rt_view_adaptive_render_tiles: ";
    if (stats && stats->struct_size != sizeof(rt_view_adaptive_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (!a || !stats) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (!tile_mask) return fail(RT_ERR_INVALID_ARG, who + "null argument (tile_mask)");
    return render(a, n_samples, nullptr, tile_mask, stats, who);
}

int rt_view_adaptive_tiles(rt_view_adaptive *a, int32_t view, rt_adaptive_tile *out) {
    const std::string who = "rt_view_adaptive_tiles: ";
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (const int rc = check_view(a, view, who)) return rc;
        memcpy(out, a->entries.data() + (size_t)view * a->tiles, a->tiles * sizeof(rt_adaptive_tile));
        return RT_OK;
    });
}

int rt_view_adaptive_sample_map(rt_view_adaptive *a, int32_t view, int32_t *out) {
    const std::string who = "rt_view_adaptive_sample_map: ";
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (const int rc = check_view(a, view, who)) return rc;
        const rt_adaptive_tile *table = a->entries.data() + (size_t)view * a->tiles;
        const int32_t W = a->view.width, H = a->view.height;
        for (int32_t y = 0; y < H; y++)
            for (int32_t x = 0; x < W; x++) out[(size_t)y * W + x] = table[(size_t)(y >> 3) * a->sub_w + (x >> 3)].samples;
        return RT_OK;
    });
}

int rt_view_adaptive_resolve(rt_view_adaptive *a, int32_t view, uint32_t flags, float *out_rgb, uint8_t *out_rgb8) {
    const std::string who = "rt_view_adaptive_resolve: ";
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_FLAG_OUT_DEVICE");
        if (const int rc = check_view(a, view, who)) return rc;
        if (!out_rgb && !out_rgb8) return RT_OK;
        HIP_CHECK(hipSetDevice(a->scene->device));
        const size_t first = (size_t)view * a->tiles;
        std::vector<float> inv(a->tiles);
        for (uint32_t t = 0; t < a->tiles; t++) inv[t] = a->entries[first + t].samples > 0 ? (float)(1.0 / a->entries[first + t].samples) : 0.f; // scene.cpp:176, as rt_render(samples = d) evaluates it
        HIP_CHECK(hipMemcpyAsync(a->d_inv + first, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice, a->stream));
        RenderView R = a->view;
        const size_t elems = (size_t)R.width * R.height * 3;
        StagedOut rgb(out_rgb, flags, elems, sizeof(float)), rgb8(out_rgb8, flags, elems, 1);
        R.out_rgb = (float *)rgb.dev; R.out_rgb8 = (uint8_t *)rgb8.dev;
        R.accum = a->d_state + 6 * (size_t)view * R.n_pixslots;
        ViewAdaptiveView V = device_view(a);
        V.first = (uint32_t)first;
        view_adaptive_launch_resolve(a->scene, R, V, a->stream);
        rgb.copy_back(a->stream);
        rgb8.copy_back(a->stream);
        HIP_CHECK(hipStreamSynchronize(a->stream));
        return RT_OK;
    });
}

int rt_view_adaptive_noise(rt_view_adaptive *a, int32_t view, uint32_t flags, float *out_se, rt_noise_summary *summary) {
    const std::string who = "rt_view_adaptive_noise: ";
    if (summary && summary->struct_size != sizeof(rt_noise_summary)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_FLAG_OUT_DEVICE");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(a, who)) return rc;
        if (const int rc = check_view(a, view, who)) return rc;
        const size_t first = (size_t)view * a->tiles;
        const rt_adaptive_tile *table = a->entries.data() + first;
        int32_t batches = 0, observed = 0, total = 0;
        adaptive_largest(table, a->observed.data() + first, a->tiles, batches, observed, total);
        if (batches < 2) return fail(RT_ERR_INVALID_ARG, who + "view " + std::to_string(view) + ": no sub-tile has 2 batches yet (" + std::to_string(batches) + " at most): the scatter of batch means needs at least 2");
        if (out_se) { // the map: the estimate once more over this view, with the numbers of the state as it stands.  It overwrites the view's
                      // part of d_args (dof and d only) and rewrites its part of d_entries with the bits it holds: neither outlives a call,
                      // every slice uploads all of d_args and reads d_entries only behind its own estimate
            HIP_CHECK(hipSetDevice(a->scene->device));
            std::vector<AdTileArgs> args(a->tiles);
            for (uint32_t t = 0; t < a->tiles; t++) { args[t] = AdTileArgs{}; args[t].dof = (float)(table[t].batches - 1); args[t].d = (float)table[t].samples; }
            HIP_CHECK(hipMemcpyAsync(a->d_args + first, args.data(), args.size() * sizeof(AdTileArgs), hipMemcpyHostToDevice, a->stream));
            StagedOut se(out_se, flags, (size_t)a->view.width * a->view.height, sizeof(float));
            ViewAdaptiveView V = device_view(a);
            V.first = (uint32_t)first; V.count = a->tiles; V.out_se = (float *)se.dev;
            view_adaptive_launch_estimate(a->scene, a->view, V, a->stream);
            se.copy_back(a->stream);
            HIP_CHECK(hipStreamSynchronize(a->stream));
        }
        if (summary) {
            summary->batches = batches; summary->samples_observed = observed; summary->samples_total = total;
            adaptive_summarise(table, a->tiles, summary);
        }
        return RT_OK;
    });
}

} // extern "C"

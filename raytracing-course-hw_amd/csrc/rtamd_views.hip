// A batch of cameras over one live scene through the C-ABI (include/rtamd.h: rt_views_*), host side only: the object and its state, the
// refusals, and the slice (gather, the persistent kernel's view source, scatter) over the query layer's chunk loop.  No kernel and no
// kernel header here: the kernels (device/rt_views.h, device/rt_path_source.h) live in rtamd_api.hip and are launched through
// views_launch_* and source_render.  The scene is only read: a view's camera lives in the set's own record array.
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
#include "device/rt_types_query.h"
#include "device/rt_types_adaptive.h" // source_chunks, source_chunk_slots
#include "device/rt_types_views.h"

using namespace rtamd;

static_assert(sizeof(rt_views_params) == 40 && sizeof(rt_views_stats) == 72, "the view set's records as include/rtamd.h lays them out");

#define VIEWS_SAMPLE_LIMIT (1 << 25) // the path records' sample index (wf_pack): a view's count stays below it

struct rt_views {
    rt_scene *scene = nullptr;
    hipStream_t stream = nullptr;
    RenderView view{};                  // one view's frame: geometry, n_pixslots, ray_depth
    uint32_t tiles = 0;                 // 8x8 sub-tiles of a view
    int32_t n_views = 0;
    uint32_t *d_state = nullptr;        // n_views blocks of 24 bytes per pixel slot (rt_types_views.h)
    ViewCamera *d_cameras = nullptr;    // n_views
    uint32_t *d_list = nullptr;         // n_views: the active views of a slice
    uint32_t *d_strip = nullptr;        // one chunk's strip: 24 bytes per slot, its pixel words, a view word per 64 slots
    size_t strip_cap = 0;               // slots
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the gather and the scatter of a chunk
    std::vector<int32_t> samples;       // per view
    std::string broken;
    ~rt_views() {
        for (void *p : {(void *)d_state, (void *)d_cameras, (void *)d_list, (void *)d_strip})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int usable(const rt_views *v, const std::string &who) {
    if (!v->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "an earlier slice failed and left the state half advanced (" + v->broken + ")");
    return RT_OK;
}

// The refusals of a camera array (host/rt_views_camera.h), before anything is touched; `first`: the view of cameras[0].
int check_cameras(const rt_camera *cameras, int32_t first, int32_t n, const std::string &who) {
    const std::string why = views_cameras_check(cameras, first, n);
    return why.empty() ? RT_OK : fail(RT_ERR_INVALID_ARG, who + why);
}

// Views first .. first + n - 1 get `cameras` and a fresh state: sum 0, engines reseeded, 0 samples.
void reset_views(rt_views *v, int32_t first, int32_t n, const rt_camera *cameras) {
    std::vector<ViewCamera> rec((size_t)n);
    for (int32_t i = 0; i < n; i++) rec[(size_t)i] = views_camera_record(cameras[i], v->view.width, v->view.height);
    HIP_CHECK(hipMemcpyAsync(v->d_cameras + first, rec.data(), rec.size() * sizeof(ViewCamera), hipMemcpyHostToDevice, v->stream));
    for (int32_t i = first; i < first + n; i++) {
        RenderView R = v->view;
        R.accum = v->d_state + 6 * (size_t)i * v->view.n_pixslots;
        views_launch_seed(v->scene, R, v->stream);
        v->samples[(size_t)i] = 0;
    }
    HIP_CHECK(hipStreamSynchronize(v->stream)); // `rec` is pageable memory of this call
}

// One slice of n_samples for the views of `list` (ascending).
int slice(rt_views *v, int32_t n_samples, const std::vector<uint32_t> &list, rt_views_stats &st, const std::string &who) {
    rt_scene *scene = v->scene;
    hipStream_t stream = v->stream;
    HIP_CHECK(hipMemcpyAsync(v->d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    const size_t n_tiles = list.size() * v->tiles;
    const size_t chunk_tiles = std::max<size_t>(1u, source_chunk_slots() / 64u);
    const size_t cap = std::min(n_tiles, chunk_tiles) * 64u;
    if (v->strip_cap < cap) {
        if (v->d_strip) (void)hipFree(v->d_strip);
        v->d_strip = nullptr; v->strip_cap = 0;
        HIP_CHECK(hipMalloc((void **)&v->d_strip, cap * 28u + cap / 64u * 4u));
        v->strip_cap = cap;
    }
    return source_chunks(n_tiles, chunk_tiles, stream, [&](size_t first, size_t m) -> int {
        ViewsView V{};
        V.state = v->d_state; V.vslots = v->view.n_pixslots; V.tiles = v->tiles;
        V.list = v->d_list; V.first_tile = (uint32_t)first;
        V.strip = v->d_strip; V.strip_slots = (uint32_t)m * 64u; V.pixels = v->d_strip + 6 * (size_t)V.strip_slots;
        HIP_CHECK(hipEventRecord(v->ev[0], stream));
        st.launches += views_launch_gather(scene, v->view, V, stream);
        HIP_CHECK(hipEventRecord(v->ev[1], stream));
        SourceChunk C{};
        C.mode = 5u; C.n = V.strip_slots; C.streams = 1u;
        C.ray_depth = v->view.ray_depth; C.samples = n_samples; C.state = V.strip;
        C.pixels = V.pixels; C.frame_w = v->view.width; C.frame_h = v->view.height; C.cameras = v->d_cameras;
        SourceResult res{};
        if (const int rc = source_render(scene, C, stream, res, who)) return rc;
        HIP_CHECK(hipEventRecord(v->ev[2], stream));
        st.launches += res.launches + views_launch_scatter(scene, v->view, V, stream);
        HIP_CHECK(hipEventRecord(v->ev[3], stream));
        HIP_CHECK(hipEventSynchronize(v->ev[3]));
        float g = 0.f, s = 0.f;
        HIP_CHECK(hipEventElapsedTime(&g, v->ev[0], v->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&s, v->ev[2], v->ev[3]));
        st.gather_ms += g; st.scatter_ms += s; st.kernel_ms += res.kernel_ms;
        st.exact_walks += res.exact_walks; st.reference_exact = res.reference_exact;
        return RT_OK;
    });
}

} // namespace

extern "C" {

int rt_views_create(rt_scene *scene, const rt_views_params *p, const rt_camera *cameras, rt_views **out) {
    const std::string who = "rt_views_create: ";
    if (p && p->struct_size != sizeof(rt_views_params)) return fail(RT_ERR_INVALID_ARG, who + "params.struct_size mismatch (ABI skew)");
    if (!scene || !p || !cameras || !out) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    *out = nullptr;
    return guarded(who, [&]() -> int {
        if (p->flags != 0) return fail(RT_ERR_INVALID_ARG, who + "params.flags must be 0");
        if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(RT_ERR_INVALID_ARG, who + "params.reserved must be 0");
        if (p->n_views < 1) return fail(RT_ERR_INVALID_ARG, who + "params.n_views must be at least 1");
        if (p->width < 1 || p->height < 1) return fail(RT_ERR_INVALID_ARG, who + "params.width and params.height must be at least 1");
        if (p->width > 65535 || p->height > 65535) return fail(RT_ERR_LIMIT, who + "params.width and params.height must stay below 65,536 (a slot's pixel is one packed word)");
        if (p->ray_depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "params.ray_depth above RT_MAX_DEPTH (16)");
        const uint64_t tiles = (uint64_t)((p->width + 7) / 8) * (uint64_t)((p->height + 7) / 8); // 64 pixel slots each
        if (tiles * 64u * (uint64_t)p->n_views >= 0x80000000ull)
            return fail(RT_ERR_LIMIT, who + "params.n_views: " + std::to_string(p->n_views) + " views of " + std::to_string(tiles * 64u) + " pixel slots each do not stay below 2^31 slots");
        std::unique_ptr<rt_views> v(new rt_views);
        rt_render_params q{};
        q.struct_size = sizeof q; q.width = p->width; q.height = p->height; q.samples = 1; q.ray_depth = p->ray_depth; q.integrator = RT_INTEGRATOR_HW8;
        std::string err;
        if (!resolve_tiles(&q, v->view, err)) return fail(RT_ERR_INVALID_ARG, who + err);
        if (scene->flavor != RT_INTEGRATOR_HW8)
            return fail(RT_ERR_UNSUPPORTED, who + "a view set runs the persistent hw8 kernel: a scene created for RT_INTEGRATOR_HW8 only (scene prepared for " +
                                            std::to_string(scene->flavor) + "); there is no fallback");
        if (const int rc = check_cameras(cameras, 0, p->n_views, who)) return rc;
        v->scene = scene; v->stream = (hipStream_t)p->stream; v->n_views = p->n_views;
        v->tiles = (uint32_t)tiles;
        v->view.n_pixslots = v->tiles * 64u;
        if (const int rc = source_check(scene, (uint32_t)std::min((size_t)v->view.n_pixslots * (size_t)p->n_views, source_chunk_slots()), v->view.ray_depth, 1, who)) return rc;
        HIP_CHECK(hipSetDevice(scene->device));
        HIP_CHECK(hipMalloc((void **)&v->d_state, (size_t)v->view.n_pixslots * (size_t)p->n_views * 24u));
        HIP_CHECK(hipMalloc((void **)&v->d_cameras, (size_t)p->n_views * sizeof(ViewCamera)));
        HIP_CHECK(hipMalloc((void **)&v->d_list, (size_t)p->n_views * sizeof(uint32_t)));
        for (hipEvent_t &e : v->ev) HIP_CHECK(hipEventCreate(&e));
        v->samples.assign((size_t)p->n_views, 0);
        reset_views(v.get(), 0, p->n_views, cameras);
        *out = v.release();
        return RT_OK;
    });
}

void rt_views_destroy(rt_views *v) {
    if (v) (void)hipSetDevice(v->scene->device);
    delete v;
}

int rt_views_set_cameras(rt_views *v, int32_t first, int32_t n, const rt_camera *cameras) {
    const std::string who = "rt_views_set_cameras: ";
    if (!v || !cameras) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(v, who)) return rc;
        if (first < 0 || first >= v->n_views) return fail(RT_ERR_INVALID_ARG, who + "first (" + std::to_string(first) + ") is no view of the set's " + std::to_string(v->n_views));
        if (n < 1 || n > v->n_views - first) return fail(RT_ERR_INVALID_ARG, who + "n (" + std::to_string(n) + ") must be 1 .. " + std::to_string(v->n_views - first) + " from view " + std::to_string(first));
        if (const int rc = check_cameras(cameras, first, n, who)) return rc;
        HIP_CHECK(hipSetDevice(v->scene->device));
        const int rc = guarded(who, [&]() -> int { reset_views(v, first, n, cameras); return RT_OK; });
        if (rc != RT_OK) v->broken = rt_last_error();
        return rc;
    });
}

int rt_views_samples(const rt_views *v, int32_t *out) {
    if (!v || !out) return fail(RT_ERR_INVALID_ARG, "rt_views_samples: null argument");
    memcpy(out, v->samples.data(), v->samples.size() * sizeof(int32_t));
    return RT_OK;
}

int rt_views_render(rt_views *v, int32_t n_samples, const uint8_t *mask, rt_views_stats *stats) {
    const std::string who = "rt_views_render: ";
    if (stats && stats->struct_size != sizeof(rt_views_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (!v || !stats) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(v, who)) return rc;
        const double t0 = now_ms();
        if (n_samples <= 0) return fail(RT_ERR_INVALID_ARG, who + "n_samples must be positive");
        std::vector<uint32_t> list;
        for (int32_t i = 0; i < v->n_views; i++) if (!mask || mask[i]) list.push_back((uint32_t)i);
        for (uint32_t i : list)
            if ((int64_t)v->samples[i] + n_samples >= (int64_t)VIEWS_SAMPLE_LIMIT)
                return fail(RT_ERR_LIMIT, who + "n_samples: view " + std::to_string(i) + ": " + std::to_string(v->samples[i]) + " + " + std::to_string(n_samples) +
                                          " samples per pixel do not fit the path records' sample index (below " + std::to_string(VIEWS_SAMPLE_LIMIT) + ")");
        rt_views_stats st{};
        st.struct_size = sizeof(rt_views_stats);
        st.reference_exact = v->scene->view.exact_boxes == 1u ? 1u : 0u;
        st.active_views = (uint32_t)list.size();
        if (!list.empty()) {
            const size_t slots = list.size() * (size_t)v->view.n_pixslots;
            if (const int rc = source_check(v->scene, (uint32_t)std::min(slots, source_chunk_slots()), v->view.ray_depth, n_samples, who)) return rc;
            HIP_CHECK(hipSetDevice(v->scene->device));
            const int rc = guarded(who, [&]() -> int { return slice(v, n_samples, list, st, who); });
            if (rc != RT_OK) { v->broken = rt_last_error(); return rc; } // the slice failed under way (a refusal or a HIP error): the state is half advanced
            for (uint32_t i : list) v->samples[i] += n_samples;
            st.samples = (uint64_t)list.size() * (uint64_t)v->view.width * (uint64_t)v->view.height * (uint64_t)n_samples;
        }
        st.min_samples = *std::min_element(v->samples.begin(), v->samples.end());
        st.max_samples = *std::max_element(v->samples.begin(), v->samples.end());
        st.total_ms = now_ms() - t0;
        *stats = st;
        return RT_OK;
    });
}

int rt_views_resolve(rt_views *v, int32_t view, uint32_t flags, float *out_rgb, uint8_t *out_rgb8) {
    const std::string who = "rt_views_resolve: ";
    if (!v) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    return guarded(who, [&]() -> int {
        if (const int rc = usable(v, who)) return rc;
        if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_FLAG_OUT_DEVICE");
        if (view < 0 || view >= v->n_views) return fail(RT_ERR_INVALID_ARG, who + "view (" + std::to_string(view) + ") is no view of the set's " + std::to_string(v->n_views));
        const int32_t d = v->samples[(size_t)view];
        if (d <= 0) return fail(RT_ERR_INVALID_ARG, who + "view " + std::to_string(view) + " has no samples yet (a picture needs at least one)");
        if (!out_rgb && !out_rgb8) return RT_OK;
        HIP_CHECK(hipSetDevice(v->scene->device));
        RenderView R = v->view;
        const size_t elems = (size_t)R.width * R.height * 3;
        StagedOut rgb(out_rgb, flags, elems, sizeof(float)), rgb8(out_rgb8, flags, elems, 1);
        R.out_rgb = (float *)rgb.dev; R.out_rgb8 = (uint8_t *)rgb8.dev;
        R.accum = v->d_state + 6 * (size_t)view * R.n_pixslots;
        R.samples = d;
        R.inv_samples = (float)(1.0 / d); // scene.cpp:176, as rt_render(samples = d) evaluates it
        views_launch_resolve(v->scene, R, v->stream);
        rgb.copy_back(v->stream);
        rgb8.copy_back(v->stream);
        HIP_CHECK(hipStreamSynchronize(v->stream));
        return RT_OK;
    });
}

} // extern "C"

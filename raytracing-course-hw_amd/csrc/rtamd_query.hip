// Batched ray queries through the C-ABI (include/rtamd.h: rt_query_closest, rt_query_light_pdf, rt_query_occluded), the first-hit layer over them
// (rt_query_surface, rt_query_environment, rt_camera_rays, rt_render_guides) and the bounce step (rt_query_scatter, rt_query_bsdf,
// rt_trace_paths, rt_rng_*) and its first caller, the baker (rt_bake_rays, rt_bake): argument checks, the chunking, the staging, the
// rounds and the statistics; and rt_render_paths / rt_render_bake, the same answers through the persistent render kernel
// (device/rt_path_source.h; the launches are rtamd_api.hip's frame driver, source_render).  No kernel and no kernel header here: the
// kernels (device/rt_query.h, device/rt_query_surface.h, device/rt_query_scatter.h, device/rt_bake.h) live in rtamd_api.hip,
// where every __global__ keeps one definition, and are launched through query_launch_* (device/rt_types_query.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rtamd.h"
#include "host/knobs.h"
#include "host/rt_scene.h"
#include "device/rt_types_query.h"

using namespace rtamd;

namespace {

static_assert(sizeof(rt_bake_point) == 24 && sizeof(rt_bake_params) == 32 && sizeof(rt_bake_stats) == 88, "the baker's records as include/rtamd.h lays them out");
static_assert(sizeof(rt_ray) == 24 && sizeof(rt_hit) == 64 && sizeof(rt_surface) == 64 && sizeof(rt_rng) == 16 && sizeof(rt_scatter) == 64,
              "rt_ray is 24 bytes, rt_rng 16, rt_hit, rt_surface and rt_scatter 64: the kernels read and write them as words");

// Rays per chunk: what the staging is sized for.  RTAMD_QUERY_CHUNK (testing) lowers it, so that a small call crosses chunk seams; it
// changes no answer, a ray's answer does not depend on its neighbours.
const size_t QUERY_CHUNK = 262144;
size_t query_chunk() { return std::min(QUERY_CHUNK, (size_t)std::max(64, env_positive("RTAMD_QUERY_CHUNK", (int)QUERY_CHUNK))); }

// The staging of one chunk, carved out of one allocation that the scene keeps: counters first, then the arrays in 256-byte steps.
// The two ray queries need the first eight parts; a surface query or a guide pass (STAGE_FIRST_HIT) grows the allocation by the next
// two, an occlusion query (STAGE_OCCLUSION) by the last two: a bound and an answer byte per ray.  The bounce step (STAGE_SCATTER) takes
// the first-hit layer's parts and four more: the engines, the rt_scatter records, the rays of the light walk and its answers.  The
// baker (STAGE_BAKE) takes the bounce step's parts and its per-slot state: the points, the first directions, `bake_floats` accumulator
// floats, the samples left, its counters and, with host arrays, the chunk's answer.
const size_t PLANE_FLOATS = 10; // albedo 3, normal 3, depth 1, emission 3
enum StageParts { STAGE_WALK, STAGE_FIRST_HIT, STAGE_OCCLUSION, STAGE_SCATTER, STAGE_BAKE };
struct QueryStage {
    uint32_t *ctr; unsigned long long *totals;
    float *rays; uint8_t *out; float4 *rec; uint32_t *q_fast, *q_exact, *ovf;
    uint8_t *surf; float *planes;
    float *tmax; uint8_t *occ;
    uint8_t *rng, *scat; float *walk_rays, *light_pdf;
    float *bake_points, *bake_dir0, *bake_acc, *bake_out; uint32_t *bake_left; unsigned long long *bake_ctr;
};
QueryStage query_stage(rt_scene *scene, StageParts parts, size_t bake_floats = 0, bool bake_out = false) {
    const bool bake = parts == STAGE_BAKE, scatter = parts == STAGE_SCATTER || bake, first_hit = parts == STAGE_FIRST_HIT || scatter, occlusion = parts == STAGE_OCCLUSION;
    const size_t C = QUERY_CHUNK, ovf_words = query_ovf_words(scene);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255u) & ~(size_t)255u; return here; };
    const size_t o_ctr = take(RQ_CTR_WORDS * 4), o_tot = take(RQ_TOTAL_WORDS * 8), o_rays = take(C * sizeof(rt_ray)), o_out = take(C * sizeof(rt_hit)),
                 o_rec = take(C * 16), o_fast = take(C * 4), o_exact = take(C * 4), o_ovf = take(ovf_words * 4);
    size_t o_surf = 0, o_planes = 0;
    if (first_hit) { o_surf = take(C * sizeof(rt_surface)); o_planes = take(C * PLANE_FLOATS * 4); }
    size_t o_tmax = 0, o_occ = 0;
    if (occlusion) { o_tmax = take(C * sizeof(float)); o_occ = take(C); }
    size_t o_rng = 0, o_scat = 0, o_walk = 0, o_lpdf = 0;
    if (scatter) { o_rng = take(C * sizeof(rt_rng)); o_scat = take(C * sizeof(rt_scatter)); o_walk = take(C * sizeof(rt_ray)); o_lpdf = take(C * sizeof(float)); }
    size_t o_bpts = 0, o_bdir = 0, o_bacc = 0, o_bleft = 0, o_bctr = 0, o_bout = 0;
    if (bake) {
        o_bpts = take(C * sizeof(rt_bake_point)); o_bdir = take(C * 12); o_bacc = take(C * bake_floats * 4); o_bleft = take(C * 4);
        o_bctr = take(RQ_BAKE_CTR_WORDS * 8); o_bout = take(bake_out ? C * bake_floats * 4 : 0);
    }
    grow(scene->query_stage, scene->query_stage_bytes, at);
    uint8_t *b = scene->query_stage;
    QueryStage s;
    s.ctr = (uint32_t *)(b + o_ctr); s.totals = (unsigned long long *)(b + o_tot);
    s.rays = (float *)(b + o_rays); s.out = b + o_out; s.rec = (float4 *)(b + o_rec);
    s.q_fast = (uint32_t *)(b + o_fast); s.q_exact = (uint32_t *)(b + o_exact);
    s.ovf = ovf_words ? (uint32_t *)(b + o_ovf) : nullptr;
    s.surf = first_hit ? b + o_surf : nullptr; s.planes = first_hit ? (float *)(b + o_planes) : nullptr;
    s.tmax = occlusion ? (float *)(b + o_tmax) : nullptr; s.occ = occlusion ? b + o_occ : nullptr;
    s.rng = scatter ? b + o_rng : nullptr; s.scat = scatter ? b + o_scat : nullptr;
    s.walk_rays = scatter ? (float *)(b + o_walk) : nullptr; s.light_pdf = scatter ? (float *)(b + o_lpdf) : nullptr;
    s.bake_points = bake ? (float *)(b + o_bpts) : nullptr; s.bake_dir0 = bake ? (float *)(b + o_bdir) : nullptr;
    s.bake_acc = bake ? (float *)(b + o_bacc) : nullptr; s.bake_left = bake ? (uint32_t *)(b + o_bleft) : nullptr;
    s.bake_ctr = bake ? (unsigned long long *)(b + o_bctr) : nullptr; s.bake_out = bake && bake_out ? (float *)(b + o_bout) : nullptr;
    return s;
}

// What every call here checks first.  `allowed`: the flags the function takes, `allowed_names` their names for the message.
int check_call(const rt_scene *scene, const rt_query_stats *stats, uint32_t flags, uint32_t allowed, const char *allowed_names, const std::string &who) {
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (flags & ~allowed) return fail(RT_ERR_INVALID_ARG, who + "flags other than " + allowed_names);
    if (scene->flavor != RT_INTEGRATOR_HW8) return fail(RT_ERR_UNSUPPORTED, who + "ray queries serve scenes created for hw8 / hw7 (this one was prepared for integrator " + std::to_string(scene->flavor) + ")");
    return RT_OK;
}

// One call over n items in chunks.  Per chunk: before(S, first, m, stream) queues the copies in, launch(...) the kernels (between the
// scene's two events) and returns their number, after(...) queues the copies out; the next chunk reuses the staging, so each ends with
// a synchronisation.  n == 0 launches nothing.
template <class Before, class Launch, class After>
int answer(rt_scene *scene, size_t n, rt_query_stats *stats, const std::string &who, StageParts parts, Before before, Launch launch, After after) {
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        rt_query_stats st{};
        st.struct_size = sizeof(rt_query_stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        st.rays = n;
        if (n) {
            HIP_CHECK(hipSetDevice(scene->device));
            hipStream_t stream = nullptr;
            const QueryStage S = query_stage(scene, parts);
            const size_t chunk = query_chunk();
            HIP_CHECK(hipMemsetAsync(S.totals, 0, RQ_TOTAL_WORDS * 8, stream));
            float ms_sum = 0.f;
            for (size_t first = 0; first < n; first += chunk) {
                const size_t m = std::min(chunk, n - first);
                before(S, first, m, stream);
                HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
                HIP_CHECK(hipEventRecord(scene->ev_start, stream));
                st.launches += launch(S, first, m, stream);
                HIP_CHECK(hipEventRecord(scene->ev_stop, stream));
                after(S, first, m, stream);
                HIP_CHECK(hipStreamSynchronize(stream)); // the next chunk reuses the staging
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop));
                ms_sum += ms;
            }
            unsigned long long totals[RQ_TOTAL_WORDS];
            HIP_CHECK(hipMemcpy(totals, S.totals, sizeof totals, hipMemcpyDeviceToHost));
            st.exact_walks = totals[RQ_TOTAL_EXACT] + totals[RQ_TOTAL_RIDE_EXACT]; st.invalid_rays = totals[RQ_TOTAL_INVALID];
            st.kernel_ms = ms_sum;
        }
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

// The closest-hit and light-pdf launches' view of a chunk of m rays at `rays`.
QueryView walk_view(const rt_scene *scene, const QueryStage &S, size_t m, uint32_t flags, const float *rays) {
    QueryView Q{};
    Q.n = (uint32_t)m;
    Q.reference_walk = (flags & RT_QUERY_REFERENCE_WALK) ? 1u : 0u;
    Q.origin_bound = scene->view.box_c2 * 1048576.f; // box_c2 = 2^-20 max|coordinate| of scene and camera
    Q.rec = S.rec; Q.q_fast = S.q_fast; Q.q_exact = S.q_exact; Q.ctr = S.ctr; Q.totals = S.totals; Q.ovf = S.ovf;
    Q.rays = rays;
    return Q;
}

// Both ray queries: `light` answers one float per ray, else one rt_hit.
int query(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, void *out, rt_query_stats *stats, bool light, const std::string &who) {
    if (const int rc = check_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK, "RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK", who)) return rc;
    if (light && scene->view.n_lights == 0) return fail(RT_ERR_INVALID_ARG, who + "the scene has no lights: there is no light pdf to ask for");
    if (n && (!rays || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && !light && ((uintptr_t)out & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_hit array must be 16-byte aligned");
    const size_t out_size = light ? sizeof(float) : sizeof(rt_hit);
    return answer(scene, n, stats, who, STAGE_WALK,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            QueryView Q = walk_view(scene, S, m, flags, on_device ? (const float *)(rays + first) : S.rays);
            uint8_t *dev_out = on_device ? (uint8_t *)out + first * out_size : S.out;
            if (light) Q.pdf = (float *)dev_out; else Q.hits = (uint4 *)dev_out;
            return light ? query_launch_light_pdf(scene, Q, stream) : query_launch_closest(scene, Q, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync((uint8_t *)out + first * out_size, S.out, m * out_size, hipMemcpyDeviceToHost, stream));
        });
}

// The material index of every LOAD-order triangle, made on the device from the shading records the first time a surface is asked for.
void ensure_materials(rt_scene *scene, hipStream_t stream) {
    if (scene->query_materials) return;
    OwnedDev table;
    HIP_CHECK(hipMalloc(&table.p, std::max<size_t>(scene->view.n_tris, 4u) * sizeof(uint32_t)));
    query_launch_material_table(scene, (uint32_t *)table.p, stream);
    scene->query_materials = (uint32_t *)table.release();
}

SurfaceView surface_view(const rt_scene *scene, const QueryStage &S, size_t m, const void *hits, void *out) {
    SurfaceView V{};
    V.hits = (const uint4 *)hits; V.out = (uint4 *)out;
    V.n = (uint32_t)m; V.n_tris = scene->view.n_tris;
    V.tri_material = scene->query_materials; V.totals = S.totals;
    return V;
}

// ---- the bounce step ------------------------------------------------------------------------------------------------------------------------
const uint32_t SCATTER_FLAGS = RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK;
const char *const SCATTER_FLAG_NAMES = "RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK";

// What rt_query_scatter, rt_query_bsdf and rt_trace_paths check before the scene: stats, flags, and the engines of a host array, so
// that no launch ever sees a state the engine cannot be in (device arrays: the sample kernel marks such a record invalid).
int check_scatter_call(const rt_query_stats *stats, uint32_t flags, const rt_rng *rng, size_t n, const std::string &who) {
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (flags & ~SCATTER_FLAGS) return fail(RT_ERR_INVALID_ARG, who + "flags other than " + SCATTER_FLAG_NAMES);
    if (rng && !(flags & RT_QUERY_DEVICE_POINTERS))
        for (size_t i = 0; i < n; i++)
            if (!rq_rng_valid(rng[i].x))
                return fail(RT_ERR_INVALID_ARG, who + "rng[" + std::to_string(i) + "].x = " + std::to_string(rng[i].x) + " is no state of the engine (1 .. 2147483646)");
    return RT_OK;
}

// A chunk's records as the kernels see them: the caller's device arrays from `first` on, or the staging.
struct ScatterArrays { const rt_ray *rays; const rt_hit *hits; const rt_surface *surfaces; rt_rng *rng; rt_scatter *out; };
ScatterView scatter_view(const QueryStage &S, size_t m, const ScatterArrays &A) {
    ScatterView V{};
    V.rays = (const float *)A.rays; V.hits = (const uint4 *)A.hits; V.surfaces = (const uint4 *)A.surfaces;
    V.rng = (uint4 *)A.rng; V.out = (uint4 *)A.out;
    V.walk_rays = S.walk_rays; V.light_pdf = S.light_pdf;
    V.n = (uint32_t)m; V.totals = S.totals;
    return V;
}

// The light walk over the rays a sample kernel left in the staging: its invalid rays are records that ride along, so its totals are the
// RIDE pair.  `rezero`: a walk before it in this chunk has used the chunk's counters.
uint32_t launch_ride_light_pdf(const rt_scene *scene, const QueryStage &S, size_t m, uint32_t flags, bool rezero, hipStream_t stream) {
    if (scene->view.n_lights == 0) return 0u;
    if (rezero) HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
    QueryView Q = walk_view(scene, S, m, flags, S.walk_rays);
    Q.pdf = S.light_pdf; Q.totals = S.totals + RQ_TOTAL_RIDE_EXACT;
    return query_launch_light_pdf(scene, Q, stream);
}

// The per-bounce stack of rt_trace_paths for `paths` paths of a chunk: 16 bytes of state, then 24 bytes per bounce.
uint8_t *path_stack(rt_scene *scene, size_t paths, int depth) {
    grow(scene->path_stack, scene->path_stack_bytes, paths * (16u + 24u * (size_t)depth));
    return scene->path_stack;
}

// One round of a chunk's m paths, for rt_trace_paths and rt_bake: closest hit, surface, scatter sample, light walk, scatter finish over
// the rays in the staging.  `later`: not the chunk's first round -- the counters have been used, and paths that have ended (or slots
// that are parked) ride along as invalid rays, so the closest-hit walk counts into the RIDE pair.
uint32_t launch_round(rt_scene *scene, const QueryStage &S, const ScatterView &V, size_t m, uint32_t flags, bool later, hipStream_t stream) {
    if (later) HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
    QueryView Q = walk_view(scene, S, m, flags, S.rays);
    Q.hits = (uint4 *)S.out;
    if (later) Q.totals = S.totals + RQ_TOTAL_RIDE_EXACT; // the caller's own invalid rays were counted in the first round
    uint32_t launches = query_launch_closest(scene, Q, stream);
    launches += query_launch_surface(scene, surface_view(scene, S, m, S.out, S.surf), stream);
    launches += query_launch_scatter_sample(scene, V, stream);
    launches += launch_ride_light_pdf(scene, S, m, flags, true, stream);
    return launches + query_launch_scatter_finish(scene, V, stream);
}

// What rt_bake_rays and rt_bake refuse alike.
const uint32_t BAKE_RAYS_FLAGS = RT_QUERY_DEVICE_POINTERS;
const uint32_t BAKE_FLAGS = RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK | RT_BAKE_LOCKSTEP;
int check_bake_mode(int32_t mode, const std::string &who, const char *field) {
    if (mode != RT_BAKE_IRRADIANCE && mode != RT_BAKE_SH9)
        return fail(RT_ERR_INVALID_ARG, who + field + " = " + std::to_string(mode) + " is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9");
    return RT_OK;
}
int check_bake_engines(const rt_rng *rng, size_t n, const std::string &who) {
    for (size_t i = 0; i < n; i++)
        if (!rq_rng_valid(rng[i].x))
            return fail(RT_ERR_INVALID_ARG, who + "rng[" + std::to_string(i) + "].x = " + std::to_string(rng[i].x) + " is no state of the engine (1 .. 2147483646)");
    return RT_OK;
}


// ---- rt_render_paths / rt_render_bake: the caller's paths through the persistent kernel (device/rt_path_source.h) ----------------------------
// Slots per chunk: the pixel slots of a 1080p frame, so the persistent kernel's path records (256 bytes per slot at depth 6) never grow
// beyond what rt_render of that frame allocates, and workload A of profiles/r30_render_paths.txt is one launch.  RTAMD_QUERY_CHUNK
// lowers it as it does for the composed calls.
const size_t SOURCE_CHUNK = 2073600;
size_t source_chunk() { return std::min(SOURCE_CHUNK, (size_t)std::max(64, env_positive("RTAMD_QUERY_CHUNK", (int)SOURCE_CHUNK))); }

// One call: `items` rays (K = 1) or points of K slots each.  `in`: the rays or the points, 24 bytes an item.
struct SourceCall {
    uint32_t mode; size_t K; int32_t depth, samples; float scale; // samples: per slot
    const void *in; rt_rng *rng; float *out; bool on_device;
};
struct SourceTotals { double kernel_ms = 0; uint32_t launches = 0, reference_exact = 0; uint64_t exact_walks = 0, no_path = 0; };

int source_run(rt_scene *scene, const SourceCall &c, size_t items, const std::string &who, SourceTotals &T) {
    HIP_CHECK(hipSetDevice(scene->device));
    hipStream_t stream = nullptr;
    const size_t chunk_items = source_chunk() / c.K; // whole points: the stream sum never crosses a seam (the chunk's minimum of 64 covers K <= 64)
    const size_t cap_items = std::min(items, chunk_items), cap = (cap_items * c.K + 63u) & ~(size_t)63u;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255u) & ~(size_t)255u; return here; };
    const size_t o_state = take(cap * 24u), o_in = take(c.on_device ? 0 : cap_items * 24u), o_rng = take(c.on_device ? 0 : cap * sizeof(rt_rng)),
                 o_out = take(c.on_device ? 0 : cap_items * 12u);
    grow(scene->source_stage, scene->source_stage_bytes, at);
    uint8_t *b = scene->source_stage;
    for (size_t first = 0; first < items; first += chunk_items) {
        const size_t m_items = std::min(chunk_items, items - first), m = m_items * c.K;
        const uint8_t *in = (const uint8_t *)c.in + first * 24u;
        rt_rng *rng = c.rng + first * c.K;
        float *out = c.out + first * 3u;
        if (!c.on_device) {
            HIP_CHECK(hipMemcpyAsync(b + o_in, in, m_items * 24u, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(b + o_rng, rng, m * sizeof(rt_rng), hipMemcpyHostToDevice, stream));
        }
        SourceView V{};
        V.state = (uint32_t *)(b + o_state); V.n_pixslots = (uint32_t)((m + 63u) & ~(size_t)63u); V.n = (uint32_t)m; V.mode = c.mode;
        V.rng = (uint4 *)(c.on_device ? (uint8_t *)rng : b + o_rng);
        const float *records = (const float *)(c.on_device ? in : b + o_in);
        if (c.mode == 1u) V.rays = records; else V.points = records;
        V.streams = (uint32_t)c.K; V.scale = c.scale;
        V.out = c.on_device ? out : (float *)(b + o_out);
        T.launches += query_launch_source_pack(scene, V, stream);
        SourceChunk C{};
        C.mode = c.mode; C.n = V.n; C.streams = V.streams; C.rays = V.rays; C.points = V.points;
        C.ray_depth = c.depth; C.samples = c.samples; C.state = V.state;
        SourceResult res{};
        if (const int rc = source_render(scene, C, stream, res, who)) return rc;
        T.launches += res.launches + query_launch_source_unpack(scene, V, stream);
        if (!c.on_device) {
            HIP_CHECK(hipMemcpyAsync(out, b + o_out, m_items * 12u, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(rng, b + o_rng, m * sizeof(rt_rng), hipMemcpyDeviceToHost, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream)); // the next chunk reuses the state and the staging
        T.kernel_ms += res.kernel_ms; T.exact_walks += res.exact_walks; T.no_path += res.no_path; T.reference_exact = res.reference_exact;
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_query_closest(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, rt_hit *out, rt_query_stats *stats) {
    return query(scene, rays, n, flags, out, stats, false, "rt_query_closest: ");
}

int rt_query_light_pdf(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, float *out, rt_query_stats *stats) {
    return query(scene, rays, n, flags, out, stats, true, "rt_query_light_pdf: ");
}

int rt_query_occluded(rt_scene *scene, const rt_ray *rays, const float *tmax, size_t n, uint32_t flags, uint8_t *out, rt_query_stats *stats) {
    const std::string who = "rt_query_occluded: ";
    // what can be judged without the scene first, each refusal naming its argument; check_call repeats the first two and adds the scene's
    const uint32_t allowed = RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK;
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (flags & ~allowed) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK");
    if (n && !rays) return fail(RT_ERR_INVALID_ARG, who + "null argument (rays)");
    if (n && !out) return fail(RT_ERR_INVALID_ARG, who + "null argument (out)");
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument (scene)");
    if (const int rc = check_call(scene, stats, flags, allowed, "RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK", who)) return rc;
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && ((uintptr_t)tmax & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the tmax array must be 4-byte aligned");
    return answer(scene, n, stats, who, STAGE_OCCLUSION,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
            if (tmax) HIP_CHECK(hipMemcpyAsync(S.tmax, tmax + first, m * sizeof(float), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            QueryView Q = walk_view(scene, S, m, flags, on_device ? (const float *)(rays + first) : S.rays);
            Q.tmax = !tmax ? nullptr : on_device ? tmax + first : S.tmax;
            Q.occ = on_device ? out + first : S.occ;
            return query_launch_occluded(scene, Q, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(out + first, S.occ, m, hipMemcpyDeviceToHost, stream));
        });
}

int rt_query_surface(rt_scene *scene, const rt_hit *hits, size_t n, uint32_t flags, rt_surface *out, rt_query_stats *stats) {
    const std::string who = "rt_query_surface: ";
    if (const int rc = check_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (n && (!hits || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && (((uintptr_t)hits | (uintptr_t)out) & 15u))
        return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_hit and rt_surface arrays must be 16-byte aligned");
    return answer(scene, n, stats, who, STAGE_FIRST_HIT,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            ensure_materials(scene, stream);
            if (!on_device) HIP_CHECK(hipMemcpyAsync(S.out, hits + first, m * sizeof(rt_hit), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            return query_launch_surface(scene, on_device ? surface_view(scene, S, m, hits + first, out + first) : surface_view(scene, S, m, S.out, S.surf), stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(out + first, S.surf, m * sizeof(rt_surface), hipMemcpyDeviceToHost, stream));
        });
}

int rt_query_environment(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_query_environment: ";
    if (const int rc = check_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (n && (!rays || !out_rgb)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    return answer(scene, n, stats, who, STAGE_WALK, // the colours of a chunk are staged where a closest-hit query keeps its 16-byte records
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            EnvironmentView V{};
            V.rays = on_device ? (const float *)(rays + first) : S.rays;
            V.rgb = on_device ? out_rgb + 3 * first : (float *)S.rec;
            V.n = (uint32_t)m; V.totals = S.totals;
            return query_launch_environment(scene, V, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(out_rgb + 3 * first, S.rec, m * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        });
}

int rt_camera_rays(rt_scene *scene, int32_t width, int32_t height, const float *xy, size_t n, uint32_t flags, rt_ray *out) {
    const std::string who = "rt_camera_rays: ";
    if (const int rc = check_call(scene, nullptr, flags, RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, who + "width and height must be positive");
    if (n && (!xy || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (!on_device)
        for (size_t i = 0; i < 2 * n; i++)
            if (!std::isfinite(xy[i])) return fail(RT_ERR_INVALID_ARG, who + "xy holds a NaN or an infinity (point " + std::to_string(i / 2) + ")");
    return answer(scene, n, nullptr, who, STAGE_WALK, // the points of a chunk are staged where a closest-hit query keeps its 16-byte records
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(S.rec, xy + 2 * first, m * 2 * sizeof(float), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            CameraView V{};
            V.xy = on_device ? xy + 2 * first : (const float *)S.rec;
            V.rays = on_device ? (float *)(out + first) : S.rays;
            V.n = (uint32_t)m; V.width = width; V.height = height;
            return query_launch_camera_rays(scene, V, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (!on_device) HIP_CHECK(hipMemcpyAsync(out + first, S.rays, m * sizeof(rt_ray), hipMemcpyDeviceToHost, stream));
        });
}

int rt_render_guides(rt_scene *scene, int32_t width, int32_t height, uint32_t flags, float *albedo, float *normal, float *depth, float *emission,
                     rt_query_stats *stats) {
    const std::string who = "rt_render_guides: ";
    if (const int rc = check_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, who + "width and height must be positive");
    if ((int64_t)width * height >= 2147483647LL) return fail(RT_ERR_INVALID_ARG, who + "image too large (width * height must stay below 2^31-1)");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    // the planes of a chunk in the staging, in this order: {plane, floats per pixel, offset in floats per pixel of the chunk}
    struct Plane { float *p; size_t k, at; } planes[4] = {{albedo, 3, 0}, {normal, 3, 3}, {depth, 1, 6}, {emission, 3, 7}};
    return answer(scene, (size_t)width * height, stats, who, STAGE_FIRST_HIT,
        [&](const QueryStage &, size_t, size_t, hipStream_t stream) { ensure_materials(scene, stream); },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            CameraView C{};
            C.rays = S.rays; C.n = (uint32_t)m; C.first_pixel = (uint32_t)first; C.width = width; C.height = height;
            uint32_t launches = query_launch_camera_rays(scene, C, stream);
            QueryView Q = walk_view(scene, S, m, 0u, S.rays);
            Q.hits = (uint4 *)S.out;
            launches += query_launch_closest(scene, Q, stream);
            launches += query_launch_surface(scene, surface_view(scene, S, m, S.out, S.surf), stream);
            GuidesView G{};
            G.hits = (const uint4 *)S.out; G.surfaces = (const uint4 *)S.surf; G.rays = S.rays; G.n = (uint32_t)m;
            float **to[4] = {&G.albedo, &G.normal, &G.depth, &G.emission};
            for (int k = 0; k < 4; k++)
                if (planes[k].p) *to[k] = on_device ? planes[k].p + planes[k].k * first : S.planes + planes[k].at * QUERY_CHUNK;
            return launches + query_launch_guides(scene, G, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            for (const Plane &pl : planes)
                if (pl.p) HIP_CHECK(hipMemcpyAsync(pl.p + pl.k * first, S.planes + pl.at * QUERY_CHUNK, m * pl.k * sizeof(float), hipMemcpyDeviceToHost, stream));
        });
}

void rt_rng_seed(rt_rng *r, uint32_t seed) {
    if (!r) return;
    const uint32_t v = seed % 2147483647u;
    r->x = v == 0 ? 1u : v; r->saved = 0.f; r->has_saved = 0u; r->reserved = 0u;
}

float rt_rng_uniform(rt_rng *r) { // rng_next and rng_u01 of device/rt_device.h, on the host
    if (!r) return 0.f;
    r->x = (uint32_t)((uint64_t)r->x * 48271ull % 2147483647ull);
    const float v = (float)(r->x - 1u) * 4.656612873077392578125e-10f;
    return v >= 1.0f ? 0.99999994f : v;
}

int rt_query_scatter(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, rt_rng *rng, size_t n, uint32_t flags,
                     rt_scatter *out, rt_query_stats *stats) {
    const std::string who = "rt_query_scatter: ";
    if (n && (!rays || !hits || !surfaces || !rng || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (const int rc = check_scatter_call(stats, flags, rng, n, who)) return rc;
    if (const int rc = check_call(scene, stats, flags, SCATTER_FLAGS, SCATTER_FLAG_NAMES, who)) return rc;
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && (((uintptr_t)hits | (uintptr_t)surfaces | (uintptr_t)rng | (uintptr_t)out) & 15u))
        return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_hit, rt_surface, rt_rng and rt_scatter arrays must be 16-byte aligned");
    return answer(scene, n, stats, who, STAGE_SCATTER,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.out, hits + first, m * sizeof(rt_hit), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.surf, surfaces + first, m * sizeof(rt_surface), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.rng, rng + first, m * sizeof(rt_rng), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            const ScatterArrays A = on_device ? ScatterArrays{rays + first, hits + first, surfaces + first, rng + first, out + first}
                                              : ScatterArrays{(const rt_ray *)S.rays, (const rt_hit *)S.out, (const rt_surface *)S.surf, (rt_rng *)S.rng, (rt_scatter *)S.scat};
            const ScatterView V = scatter_view(S, m, A);
            uint32_t launches = query_launch_scatter_sample(scene, V, stream);
            launches += launch_ride_light_pdf(scene, S, m, flags, false, stream);
            return launches + query_launch_scatter_finish(scene, V, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(out + first, S.scat, m * sizeof(rt_scatter), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(rng + first, S.rng, m * sizeof(rt_rng), hipMemcpyDeviceToHost, stream));
        });
}

int rt_query_bsdf(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, const float *dirs, size_t n, uint32_t flags,
                  float *out_brdf, float *out_pdf, rt_query_stats *stats) {
    const std::string who = "rt_query_bsdf: ";
    if (n && (!rays || !hits || !surfaces || !dirs || !out_brdf || !out_pdf)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (const int rc = check_scatter_call(stats, flags, nullptr, n, who)) return rc;
    if (const int rc = check_call(scene, stats, flags, SCATTER_FLAGS, SCATTER_FLAG_NAMES, who)) return rc;
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && (((uintptr_t)hits | (uintptr_t)surfaces) & 15u))
        return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_hit and rt_surface arrays must be 16-byte aligned");
    if (n && on_device && (((uintptr_t)dirs | (uintptr_t)out_brdf | (uintptr_t)out_pdf) & 3u))
        return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS dirs, out_brdf and out_pdf must be 4-byte aligned");
    // host arrays: the directions and the two answers of a chunk are staged where a scatter keeps its records (3 + 3 + 1 floats per record)
    auto stage_dirs = [](const QueryStage &S) { return (float *)S.scat; };
    auto stage_brdf = [](const QueryStage &S) { return (float *)S.scat + 3 * QUERY_CHUNK; };
    auto stage_pdf = [](const QueryStage &S) { return (float *)S.scat + 6 * QUERY_CHUNK; };
    return answer(scene, n, stats, who, STAGE_SCATTER,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.out, hits + first, m * sizeof(rt_hit), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.surf, surfaces + first, m * sizeof(rt_surface), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(stage_dirs(S), dirs + 3 * first, m * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            const ScatterArrays A = on_device ? ScatterArrays{rays + first, hits + first, surfaces + first, nullptr, nullptr}
                                              : ScatterArrays{(const rt_ray *)S.rays, (const rt_hit *)S.out, (const rt_surface *)S.surf, nullptr, nullptr};
            ScatterView V = scatter_view(S, m, A);
            V.dirs = on_device ? dirs + 3 * first : stage_dirs(S);
            V.out_brdf = on_device ? out_brdf + 3 * first : stage_brdf(S);
            V.out_pdf = on_device ? out_pdf + first : stage_pdf(S);
            uint32_t launches = query_launch_bsdf_rays(scene, V, stream);
            launches += launch_ride_light_pdf(scene, S, m, flags, false, stream);
            return launches + query_launch_bsdf_finish(scene, V, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(out_brdf + 3 * first, stage_brdf(S), m * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(out_pdf + first, stage_pdf(S), m * sizeof(float), hipMemcpyDeviceToHost, stream));
        });
}

int rt_trace_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng, size_t n, int32_t ray_depth, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_trace_paths: ";
    if (n && (!rays || !rng || !out_rgb)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (const int rc = check_scatter_call(stats, flags, rng, n, who)) return rc;
    if (const int rc = check_call(scene, stats, flags, SCATTER_FLAGS, SCATTER_FLAG_NAMES, who)) return rc;
    const int depth = ray_depth > 0 ? ray_depth : 6;
    if (depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "ray_depth above " + std::to_string(RT_MAX_DEPTH));
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && ((uintptr_t)rng & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_rng array must be 16-byte aligned");
    if (n && on_device && (((uintptr_t)rays | (uintptr_t)out_rgb) & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS rays and out_rgb must be 4-byte aligned");
    const size_t paths = std::min(n, query_chunk());
    uint8_t *stack = nullptr;
    return answer(scene, n, stats, who, STAGE_SCATTER,
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            ensure_materials(scene, stream);
            stack = path_stack(scene, paths, depth);
            HIP_CHECK(hipMemsetAsync(stack, 0, paths * 16u, stream)); // tail 0, no bounce kept, not ended
            // the rays change from bounce to bounce: always a copy in the staging
            HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
            if (!on_device) HIP_CHECK(hipMemcpyAsync(S.rng, rng + first, m * sizeof(rt_rng), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            const ScatterView V = scatter_view(S, m, ScatterArrays{(const rt_ray *)S.rays, (const rt_hit *)S.out, (const rt_surface *)S.surf,
                                                                   on_device ? rng + first : (rt_rng *)S.rng, (rt_scatter *)S.scat});
            PathView P{};
            P.rays = S.rays; P.hits = V.hits; P.surfaces = V.surfaces; P.scatter = V.out;
            P.state = (float4 *)stack; P.stack = (float *)(stack + paths * 16u);
            P.rgb = on_device ? out_rgb + 3 * first : (float *)S.rec; // the colours of a chunk are staged where a closest-hit query keeps its records
            P.n = (uint32_t)m;
            uint32_t launches = 0;
            for (int b = 0; b < depth; b++) {
                launches += launch_round(scene, S, V, m, flags, b != 0, stream);
                P.last = b == depth - 1 ? 1u : 0u;
                launches += query_launch_path_advance(scene, P, stream);
            }
            return launches;
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(out_rgb + 3 * first, S.rec, m * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(rng + first, S.rng, m * sizeof(rt_rng), hipMemcpyDeviceToHost, stream));
        });
}

int rt_bake_rays(rt_scene *scene, const rt_bake_point *points, rt_rng *rng, size_t n, int32_t mode, uint32_t flags, rt_ray *out, rt_query_stats *stats) {
    const std::string who = "rt_bake_rays: ";
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (const int rc = check_bake_mode(mode, who, "mode")) return rc;
    if (flags & ~BAKE_RAYS_FLAGS) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_QUERY_DEVICE_POINTERS");
    if (n && (!points || !rng || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (!on_device)
        if (const int rc = check_bake_engines(rng, n, who)) return rc;
    if (const int rc = check_call(scene, stats, flags, BAKE_RAYS_FLAGS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (n && on_device && ((uintptr_t)rng & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_rng array must be 16-byte aligned");
    if (n && on_device && (((uintptr_t)points | (uintptr_t)out) & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS points and out must be 4-byte aligned");
    return answer(scene, n, stats, who, STAGE_BAKE, // the points of a chunk are staged with the baker's state
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(S.bake_points, points + first, m * sizeof(rt_bake_point), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(S.rng, rng + first, m * sizeof(rt_rng), hipMemcpyHostToDevice, stream));
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            BakeView B{};
            B.points = on_device ? (const float *)(points + first) : S.bake_points;
            B.rng = (uint4 *)(on_device ? rng + first : (rt_rng *)S.rng);
            B.rays = on_device ? (float *)(out + first) : S.rays;
            B.totals = S.totals; B.n = (uint32_t)m; B.streams = 1u; B.mode = mode;
            return query_launch_bake_rays(scene, B, stream);
        },
        [&](const QueryStage &S, size_t first, size_t m, hipStream_t stream) {
            if (on_device) return;
            HIP_CHECK(hipMemcpyAsync(out + first, S.rays, m * sizeof(rt_ray), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(rng + first, S.rng, m * sizeof(rt_rng), hipMemcpyDeviceToHost, stream));
        });
}

int rt_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params, rt_rng *rng, float *out, rt_bake_stats *stats) {
    const std::string who = "rt_bake: ";
    if (!params) return fail(RT_ERR_INVALID_ARG, who + "null argument (params)");
    if (params->struct_size != sizeof(rt_bake_params)) return fail(RT_ERR_INVALID_ARG, who + "params.struct_size mismatch (ABI skew)");
    if (stats && stats->struct_size != sizeof(rt_bake_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (const int rc = check_bake_mode(params->mode, who, "params.mode")) return rc;
    const uint32_t flags = params->flags;
    if (flags & ~BAKE_FLAGS) return fail(RT_ERR_INVALID_ARG, who + "params.flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK | RT_BAKE_LOCKSTEP");
    if (params->reserved[0] || params->reserved[1]) return fail(RT_ERR_INVALID_ARG, who + "params.reserved must be zero");
    if (params->streams < 0) return fail(RT_ERR_INVALID_ARG, who + "params.streams must not be negative");
    if (params->streams > 64) return fail(RT_ERR_LIMIT, who + "params.streams above 64");
    const size_t K = params->streams ? (size_t)params->streams : 1u;
    if (params->samples < 1) return fail(RT_ERR_INVALID_ARG, who + "params.samples must be at least 1");
    if ((size_t)params->samples % K) return fail(RT_ERR_INVALID_ARG, who + "params.samples = " + std::to_string(params->samples) + " is no multiple of params.streams = " + std::to_string(K));
    const int depth = params->ray_depth > 0 ? params->ray_depth : 6;
    if (depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "params.ray_depth above " + std::to_string(RT_MAX_DEPTH));
    if (n_points > (((size_t)1 << 31) - 1u) / K) return fail(RT_ERR_LIMIT, who + "n_points * params.streams must stay below 2^31");
    if (n_points && (!points || !rng || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0, lockstep = (flags & RT_BAKE_LOCKSTEP) != 0;
    if (!on_device)
        if (const int rc = check_bake_engines(rng, n_points * K, who)) return rc;
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument (scene)");
    if (const int rc = check_call(scene, nullptr, 0u, 0u, "", who)) return rc;
    if (n_points && on_device && ((uintptr_t)rng & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_rng array must be 16-byte aligned");
    if (n_points && on_device && (((uintptr_t)points | (uintptr_t)out) & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS points and out must be 4-byte aligned");
    const uint32_t walk_flags = flags & (RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK);
    const size_t floats = params->mode == RT_BAKE_SH9 ? 27u : 3u;
    const uint32_t q = (uint32_t)((size_t)params->samples / K);
    const double pi = 3.14159265358979323846;
    const float scale = params->mode == RT_BAKE_SH9 ? (float)(4.0 * pi / (double)params->samples) : (float)(pi / (double)params->samples);
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        rt_bake_stats st{};
        st.struct_size = sizeof(rt_bake_stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        st.points = n_points;
        if (n_points) {
            HIP_CHECK(hipSetDevice(scene->device));
            hipStream_t stream = nullptr;
            const QueryStage S = query_stage(scene, STAGE_BAKE, floats, !on_device);
            const size_t chunk_points = query_chunk() / K; // whole points: the stream sum never crosses a seam (the chunk's minimum of 64 covers K <= 64)
            const size_t slots_max = std::min(n_points, chunk_points) * K;
            ensure_materials(scene, stream);
            uint8_t *stack = path_stack(scene, slots_max, depth);
            HIP_CHECK(hipMemsetAsync(S.totals, 0, RQ_TOTAL_WORDS * 8, stream));
            float ms_sum = 0.f;
            auto mark = [&](bool stop) { // the scene's two events around a stretch of launches; add_ms reads them once the stream has been waited for
                HIP_CHECK(hipEventRecord(stop ? scene->ev_stop : scene->ev_start, stream));
            };
            auto add_ms = [&]() { float ms = 0.f; HIP_CHECK(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop)); ms_sum += ms; };
            for (size_t first = 0; first < n_points; first += chunk_points) {
                const size_t pts = std::min(chunk_points, n_points - first), m = pts * K;
                if (!on_device) {
                    HIP_CHECK(hipMemcpyAsync(S.bake_points, points + first, pts * sizeof(rt_bake_point), hipMemcpyHostToDevice, stream));
                    HIP_CHECK(hipMemcpyAsync(S.rng, rng + first * K, m * sizeof(rt_rng), hipMemcpyHostToDevice, stream));
                }
                HIP_CHECK(hipMemsetAsync(stack, 0, slots_max * 16u, stream)); // tail 0, no bounce kept, not ended
                HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
                HIP_CHECK(hipMemsetAsync(S.bake_ctr, 0, RQ_BAKE_CTR_WORDS * 8, stream));
                const ScatterView V = scatter_view(S, m, ScatterArrays{(const rt_ray *)S.rays, (const rt_hit *)S.out, (const rt_surface *)S.surf,
                                                                       on_device ? rng + first * K : (rt_rng *)S.rng, (rt_scatter *)S.scat});
                PathView P{};
                P.rays = S.rays; P.hits = V.hits; P.surfaces = V.surfaces; P.scatter = V.out;
                P.state = (float4 *)stack; P.stack = (float *)(stack + slots_max * 16u);
                P.n = (uint32_t)m;
                BakeView B{};
                B.points = on_device ? (const float *)(points + first) : S.bake_points;
                B.rng = V.rng; B.rays = S.rays; B.dir0 = params->mode == RT_BAKE_SH9 ? S.bake_dir0 : nullptr; B.acc = S.bake_acc; B.left = S.bake_left;
                B.out = on_device ? out + first * floats : S.bake_out;
                B.ctr = S.bake_ctr; B.totals = S.totals;
                B.n = (uint32_t)m; B.streams = (uint32_t)K; B.per_stream = q; B.depth = (uint32_t)depth; B.lockstep = lockstep ? 1u : 0u;
                B.mode = params->mode; B.floats = (uint32_t)floats; B.scale = scale;
                unsigned long long ctr[RQ_BAKE_CTR_WORDS] = {};
                auto poll = [&]() { HIP_CHECK(hipMemcpy(ctr, S.bake_ctr, sizeof ctr, hipMemcpyDeviceToHost)); add_ms(); }; // waits for the stream
                uint64_t rounds = 0;
                auto round = [&](bool last) {
                    st.launches += launch_round(scene, S, V, m, walk_flags, rounds != 0, stream);
                    B.last = last ? 1u : 0u;
                    st.launches += query_launch_bake_advance(scene, P, B, stream);
                    rounds++;
                };
                mark(false);
                st.launches += query_launch_bake_rays(scene, B, stream);
                if (lockstep) { // the plain composition: every slot starts sample j in the same round, every sample takes `depth` rounds
                    for (uint32_t j = 0; j < q; j++)
                        for (int b = 0; b < depth; b++) round(b == depth - 1);
                    mark(true);
                    poll();
                } else {        // regeneration: a round at a time, until every valid slot is parked
                    mark(true);
                    poll();
                    while (ctr[RQ_BAKE_CTR_PARKED] < ctr[RQ_BAKE_CTR_SLOTS]) {
                        mark(false);
                        round(false);
                        mark(true);
                        poll();
                    }
                }
                BakeView R = B;
                R.n = (uint32_t)(pts * floats);
                mark(false);
                st.launches += query_launch_bake_resolve(scene, R, stream);
                mark(true);
                if (!on_device) {
                    HIP_CHECK(hipMemcpyAsync(out + first * floats, S.bake_out, pts * floats * sizeof(float), hipMemcpyDeviceToHost, stream));
                    HIP_CHECK(hipMemcpyAsync(rng + first * K, S.rng, m * sizeof(rt_rng), hipMemcpyDeviceToHost, stream));
                }
                HIP_CHECK(hipStreamSynchronize(stream)); // the next chunk reuses the staging
                add_ms();
                st.invalid_points += ctr[RQ_BAKE_CTR_INVALID_POINTS];
                st.paths += ctr[RQ_BAKE_CTR_SLOTS] * q;
                st.live_ray_slots += ctr[RQ_BAKE_CTR_LIVE_RAY_SLOTS];
                st.rounds += rounds;
                st.ray_slots += rounds * m;
            }
            unsigned long long totals[RQ_TOTAL_WORDS];
            HIP_CHECK(hipMemcpy(totals, S.totals, sizeof totals, hipMemcpyDeviceToHost));
            st.exact_walks = totals[RQ_TOTAL_EXACT] + totals[RQ_TOTAL_RIDE_EXACT];
            st.kernel_ms = ms_sum;
        }
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

int rt_render_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng, size_t n, int32_t ray_depth, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_render_paths: ";
    if (n && (!rays || !rng || !out_rgb)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (flags & ~RT_QUERY_DEVICE_POINTERS) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_QUERY_DEVICE_POINTERS");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (!on_device)
        if (const int rc = check_bake_engines(rng, n, who)) return rc;
    const int depth = ray_depth > 0 ? ray_depth : 6;
    if (depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "ray_depth above " + std::to_string(RT_MAX_DEPTH));
    if (const int rc = check_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS", who)) return rc;
    if (n && on_device && ((uintptr_t)rng & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_rng array must be 16-byte aligned");
    if (n && on_device && (((uintptr_t)rays | (uintptr_t)out_rgb) & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS rays and out_rgb must be 4-byte aligned");
    if (const int rc = source_check(scene, (uint32_t)std::min(std::max<size_t>(n, 1u), source_chunk()), depth, 1, who)) return rc;
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        rt_query_stats st{};
        st.struct_size = sizeof(rt_query_stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        st.rays = n;
        if (n) {
            SourceTotals T;
            if (const int rc = source_run(scene, SourceCall{1u, 1u, depth, 1, 0.f, rays, rng, out_rgb, on_device}, n, who, T)) return rc;
            st.exact_walks = T.exact_walks; st.invalid_rays = T.no_path; st.kernel_ms = T.kernel_ms; st.launches = T.launches;
            st.reference_exact = T.reference_exact;
        }
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

int rt_render_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params, rt_rng *rng, float *out, rt_bake_stats *stats) {
    const std::string who = "rt_render_bake: ";
    if (!params) return fail(RT_ERR_INVALID_ARG, who + "null argument (params)");
    if (params->struct_size != sizeof(rt_bake_params)) return fail(RT_ERR_INVALID_ARG, who + "params.struct_size mismatch (ABI skew)");
    if (stats && stats->struct_size != sizeof(rt_bake_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats.struct_size mismatch (ABI skew)");
    if (const int rc = check_bake_mode(params->mode, who, "params.mode")) return rc;
    const uint32_t flags = params->flags;
    if (flags & ~RT_QUERY_DEVICE_POINTERS) return fail(RT_ERR_INVALID_ARG, who + "params.flags other than RT_QUERY_DEVICE_POINTERS");
    if (params->reserved[0] || params->reserved[1]) return fail(RT_ERR_INVALID_ARG, who + "params.reserved must be zero");
    if (params->streams < 0) return fail(RT_ERR_INVALID_ARG, who + "params.streams must not be negative");
    if (params->streams > 64) return fail(RT_ERR_LIMIT, who + "params.streams above 64");
    const size_t K = params->streams ? (size_t)params->streams : 1u;
    if (params->samples < 1) return fail(RT_ERR_INVALID_ARG, who + "params.samples must be at least 1");
    if ((size_t)params->samples % K) return fail(RT_ERR_INVALID_ARG, who + "params.samples = " + std::to_string(params->samples) + " is no multiple of params.streams = " + std::to_string(K));
    const int depth = params->ray_depth > 0 ? params->ray_depth : 6;
    if (depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + "params.ray_depth above " + std::to_string(RT_MAX_DEPTH));
    if (n_points > (((size_t)1 << 31) - 1u) / K) return fail(RT_ERR_LIMIT, who + "n_points * params.streams must stay below 2^31");
    const size_t q = (size_t)params->samples / K;
    if (q >= ((size_t)1 << 25)) return fail(RT_ERR_LIMIT, who + "params.samples / params.streams must stay below 2^25 (the path record's sample index)");
    if (params->mode == RT_BAKE_SH9)
        return fail(RT_ERR_UNSUPPORTED, who + "RT_BAKE_SH9 does not fit the persistent kernel's path record (27 accumulators and the first direction): rt_bake serves it");
    if (n_points && (!points || !rng || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (!on_device)
        if (const int rc = check_bake_engines(rng, n_points * K, who)) return rc;
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument (scene)");
    if (const int rc = check_call(scene, nullptr, 0u, 0u, "", who)) return rc;
    if (n_points && on_device && ((uintptr_t)rng & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_rng array must be 16-byte aligned");
    if (n_points && on_device && (((uintptr_t)points | (uintptr_t)out) & 3u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS points and out must be 4-byte aligned");
    if (const int rc = source_check(scene, (uint32_t)std::min(std::max<size_t>(n_points, 1u) * K, source_chunk()), depth, (int32_t)q, who)) return rc;
    const double pi = 3.14159265358979323846;
    const float scale = (float)(pi / (double)params->samples);
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        rt_bake_stats st{};
        st.struct_size = sizeof(rt_bake_stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        st.points = n_points;
        if (n_points) {
            SourceTotals T;
            if (const int rc = source_run(scene, SourceCall{2u, K, depth, (int32_t)q, scale, points, rng, out, on_device}, n_points, who, T)) return rc;
            st.invalid_points = T.no_path; st.paths = (n_points - T.no_path) * K * q; st.exact_walks = T.exact_walks;
            st.kernel_ms = T.kernel_ms; st.launches = T.launches; st.reference_exact = T.reference_exact;
        }
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

} // extern "C"

// Batched ray queries through the C-ABI (include/rtamd.h: rt_query_closest, rt_query_light_pdf, rt_query_occluded), the first-hit layer over them
// (rt_query_surface, rt_query_environment, rt_camera_rays, rt_render_guides) and the bounce step (rt_query_scatter, rt_query_bsdf,
// rt_trace_paths, rt_rng_*) and its first caller, the baker (rt_bake_rays, rt_bake); and rt_render_paths / rt_render_bake, the same
// answers through the persistent render kernel (device/rt_path_source.h; the launches are rtamd_api.hip's frame driver, source_render).
// Host side only, each thing once: the argument predicates, the staging map, the chunk loop over a call's declared arrays, the stats
// shell; then the entry points, which check in their own order, declare their arrays and build their views.  No kernel and no kernel
// header here: the kernels (device/rt_query.h, device/rt_query_surface.h, device/rt_query_scatter.h, device/rt_bake.h) live in
// rtamd_api.hip, where every __global__ keeps one definition, and are launched through query_launch_* (device/rt_types_query.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include "../../include/rtamd.h"
#include "host/knobs.h"
#include "host/rt_scene.h"
#include "device/rt_types_query.h"
#include "device/rt_types_adaptive.h"

using namespace rtamd;

namespace {

static_assert(sizeof(rt_bake_point) == 24 && sizeof(rt_bake_params) == 32 && sizeof(rt_bake_stats) == 88, "the baker's records as include/rtamd.h lays them out");
static_assert(sizeof(rt_ray) == 24 && sizeof(rt_hit) == 64 && sizeof(rt_surface) == 64 && sizeof(rt_rng) == 16 && sizeof(rt_scatter) == 64,
              "rt_ray is 24 bytes, rt_rng 16, rt_hit, rt_surface and rt_scatter 64: the kernels read and write them as words");

// ---- the argument predicates: each refusal's text once; every entry point asks them in its own order, which is part of the ABI ------------
const uint32_t WALK_FLAGS = RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK;
bool device_pointers(uint32_t flags) { return (flags & RT_QUERY_DEVICE_POINTERS) != 0; }

int null_arg(const std::string &who, const char *name = nullptr) {
    return fail(RT_ERR_INVALID_ARG, who + "null argument" + (name ? " (" + std::string(name) + ")" : std::string()));
}
// A struct that carries its size: a stats record (null: not wanted) or rt_bake_params.  `field`: "", "stats." or "params.".
template <class T> int check_struct_size(const T *s, const std::string &who, const char *field = "") {
    if (s && s->struct_size != sizeof(T)) return fail(RT_ERR_INVALID_ARG, who + field + "struct_size mismatch (ABI skew)");
    return RT_OK;
}
int check_flags(uint32_t flags, uint32_t allowed, const std::string &who, const char *field = "") {
    if (!(flags & ~allowed)) return RT_OK;
    const struct { uint32_t bit; const char *name; } known[] = {{RT_QUERY_DEVICE_POINTERS, "RT_QUERY_DEVICE_POINTERS"}, {RT_QUERY_REFERENCE_WALK, "RT_QUERY_REFERENCE_WALK"},
                                                                {RT_BAKE_LOCKSTEP, "RT_BAKE_LOCKSTEP"}};
    std::string names;
    for (const auto &k : known)
        if (allowed & k.bit) names += (names.empty() ? "" : " | ") + std::string(k.name);
    return fail(RT_ERR_INVALID_ARG, who + field + "flags other than " + names);
}
// The scene's part of every check: there is one, and it was created for hw8 / hw7.
int check_scene(const rt_scene *scene, const std::string &who, const char *name = nullptr) {
    if (!scene) return null_arg(who, name);
    if (scene->flavor != RT_INTEGRATOR_HW8) return fail(RT_ERR_UNSUPPORTED, who + "ray queries serve scenes created for hw8 / hw7 (this one was prepared for integrator " + std::to_string(scene->flavor) + ")");
    return RT_OK;
}
// What the ray queries and the first-hit layer check first: the stats, that there is a scene, the flags, the scene's flavor.
int check_walk_call(const rt_scene *scene, const rt_query_stats *stats, uint32_t flags, uint32_t allowed, const std::string &who) {
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (!scene) return null_arg(who);
    if (const int rc = check_flags(flags, allowed, who)) return rc;
    return check_scene(scene, who);
}
// The engines of a host array, so that no launch ever sees a state the engine cannot be in (device arrays: the kernels mark such a record invalid).
int check_engines(const rt_rng *rng, size_t n, bool on_device, const std::string &who) {
    if (rng && !on_device)
        for (size_t i = 0; i < n; i++)
            if (!rq_rng_valid(rng[i].x))
                return fail(RT_ERR_INVALID_ARG, who + "rng[" + std::to_string(i) + "].x = " + std::to_string(rng[i].x) + " is no state of the engine (1 .. 2147483646)");
    return RT_OK;
}
int check_depth(int32_t ray_depth, const std::string &who, const char *field, int &depth) {
    depth = ray_depth > 0 ? ray_depth : 6;
    if (depth > RT_MAX_DEPTH) return fail(RT_ERR_LIMIT, who + field + "ray_depth above " + std::to_string(RT_MAX_DEPTH));
    return RT_OK;
}
// `device`: the call has records and they are device arrays.
int check_aligned(bool device, std::initializer_list<const void *> arrays, unsigned bytes, const char *what, const std::string &who) {
    uintptr_t bits = 0;
    for (const void *p : arrays) bits |= (uintptr_t)p;
    if (device && (bits & (bytes - 1u))) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS " + what + " must be " + std::to_string(bytes) + "-byte aligned");
    return RT_OK;
}
// The device arrays of a call with engines: the rt_rng records by 16 bytes, its two float arrays `names` by 4.
int check_engine_arrays(bool device, const void *rng, const void *a, const void *b, const char *names, const std::string &who) {
    if (const int rc = check_aligned(device, {rng}, 16, "the rt_rng array", who)) return rc;
    return check_aligned(device, {a, b}, 4, names, who);
}
int check_bake_mode(int32_t mode, const std::string &who, const char *field) {
    if (mode != RT_BAKE_IRRADIANCE && mode != RT_BAKE_SH9)
        return fail(RT_ERR_INVALID_ARG, who + field + " = " + std::to_string(mode) + " is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9");
    return RT_OK;
}
// The block rt_bake and rt_render_bake share, up to the slot limit; K and depth: the streams and the ray depth with their defaults filled in.
int check_bake_params(const rt_bake_params *params, const rt_bake_stats *stats, size_t n_points, uint32_t allowed, const std::string &who, size_t &K, int &depth) {
    if (!params) return null_arg(who, "params");
    if (const int rc = check_struct_size(params, who, "params.")) return rc;
    if (const int rc = check_struct_size(stats, who, "stats.")) return rc;
    if (const int rc = check_bake_mode(params->mode, who, "params.mode")) return rc;
    if (const int rc = check_flags(params->flags, allowed, who, "params.")) return rc;
    if (params->reserved[0] || params->reserved[1]) return fail(RT_ERR_INVALID_ARG, who + "params.reserved must be zero");
    if (params->streams < 0) return fail(RT_ERR_INVALID_ARG, who + "params.streams must not be negative");
    if (params->streams > 64) return fail(RT_ERR_LIMIT, who + "params.streams above 64");
    K = params->streams ? (size_t)params->streams : 1u;
    if (params->samples < 1) return fail(RT_ERR_INVALID_ARG, who + "params.samples must be at least 1");
    if ((size_t)params->samples % K) return fail(RT_ERR_INVALID_ARG, who + "params.samples = " + std::to_string(params->samples) + " is no multiple of params.streams = " + std::to_string(K));
    if (const int rc = check_depth(params->ray_depth, who, "params.", depth)) return rc;
    if (n_points > (((size_t)1 << 31) - 1u) / K) return fail(RT_ERR_LIMIT, who + "n_points * params.streams must stay below 2^31");
    return RT_OK;
}
// What the three bake calls check last: their arrays, the engines of host arrays, the scene (`scene_name`: how a null one is reported), the alignment.
int check_bake_arrays(const rt_scene *scene, const char *scene_name, const void *points, const rt_rng *rng, const void *out, size_t n, size_t K, bool on_device, const std::string &who) {
    if (n && (!points || !rng || !out)) return null_arg(who);
    if (const int rc = check_engines(rng, n * K, on_device, who)) return rc;
    if (const int rc = check_scene(scene, who, scene_name)) return rc;
    return check_engine_arrays(n && on_device, rng, points, out, "points and out", who);
}

// ---- the staging map ------------------------------------------------------------------------------------------------------------------------
// Rays per chunk: what the staging is sized for.  RTAMD_QUERY_CHUNK (testing) lowers it, so that a small call crosses chunk seams; it
// changes no answer, a ray's answer does not depend on its neighbours.
const size_t QUERY_CHUNK = 262144;
size_t query_chunk() { return std::min(QUERY_CHUNK, (size_t)std::max(64, env_positive("RTAMD_QUERY_CHUNK", (int)QUERY_CHUNK))); }

// Both stagings (rt_scene::query_stage, source_stage) are one allocation carved in 256-byte steps: a pass over a null base measures, a
// pass over the allocation binds.  A part of no bytes takes no room and stays null.
struct Carver {
    uint8_t *base; size_t at = 0;
    template <class T> void operator()(T *&part, size_t bytes) {
        part = base && bytes ? (T *)(base + at) : nullptr;
        at += (bytes + 255u) & ~(size_t)255u;
    }
};

// The staging of one chunk of the composed calls: counters first, then the arrays.  The two ray queries need the first eight parts; a
// surface query or a guide pass (STAGE_FIRST_HIT) grows the allocation by the next two, an occlusion query (STAGE_OCCLUSION) by a bound
// and an answer byte per ray.  The bounce step (STAGE_SCATTER) takes the first-hit layer's parts and four more: the engines, the
// rt_scatter records, the rays of the light walk and its answers.  The baker (STAGE_BAKE) takes the bounce step's parts and its per-slot
// state: the points, the first directions, `bake_floats` accumulator floats, the samples left, its counters and, with host arrays
// (`bake_out`), the chunk's answer.
const size_t PLANE_FLOATS = 10; // albedo 3, normal 3, depth 1, emission 3
enum StageParts { STAGE_WALK, STAGE_FIRST_HIT, STAGE_OCCLUSION, STAGE_SCATTER, STAGE_BAKE };
struct StageSpec { StageParts parts; size_t bake_floats = 0; bool bake_out = false; };
struct QueryStage {
    uint32_t *ctr; unsigned long long *totals;
    float *rays; uint8_t *out; float4 *rec; uint32_t *q_fast, *q_exact, *ovf;
    uint8_t *surf; float *planes;
    float *tmax; uint8_t *occ;
    uint8_t *rng, *scat; float *walk_rays, *light_pdf;
    float *bake_points, *bake_dir0, *bake_acc, *bake_out; uint32_t *bake_left; unsigned long long *bake_ctr;
};
QueryStage query_stage(rt_scene *scene, const StageSpec &spec) {
    const bool bake = spec.parts == STAGE_BAKE, scatter = spec.parts == STAGE_SCATTER || bake, first_hit = spec.parts == STAGE_FIRST_HIT || scatter;
    const size_t C = QUERY_CHUNK, ovf_words = query_ovf_words(scene);
    QueryStage s{};
    auto carve = [&](uint8_t *base) {
        Carver take{base};
        take(s.ctr, RQ_CTR_WORDS * 4); take(s.totals, RQ_TOTAL_WORDS * 8); take(s.rays, C * sizeof(rt_ray)); take(s.out, C * sizeof(rt_hit));
        take(s.rec, C * 16); take(s.q_fast, C * 4); take(s.q_exact, C * 4); take(s.ovf, ovf_words * 4);
        if (first_hit) { take(s.surf, C * sizeof(rt_surface)); take(s.planes, C * PLANE_FLOATS * 4); }
        if (spec.parts == STAGE_OCCLUSION) { take(s.tmax, C * sizeof(float)); take(s.occ, C); }
        if (scatter) { take(s.rng, C * sizeof(rt_rng)); take(s.scat, C * sizeof(rt_scatter)); take(s.walk_rays, C * sizeof(rt_ray)); take(s.light_pdf, C * sizeof(float)); }
        if (bake) {
            take(s.bake_points, C * sizeof(rt_bake_point)); take(s.bake_dir0, C * 12); take(s.bake_acc, C * spec.bake_floats * 4); take(s.bake_left, C * 4);
            take(s.bake_ctr, RQ_BAKE_CTR_WORDS * 8); take(s.bake_out, spec.bake_out ? C * spec.bake_floats * 4 : 0);
        }
        return take.at;
    };
    grow(scene->query_stage, scene->query_stage_bytes, carve(nullptr));
    carve(scene->query_stage);
    return s;
}

// ---- the chunk loop -------------------------------------------------------------------------------------------------------------------------
// A caller's array as a call declares it, once: the caller's pointer (null: not given), the bytes per item, its slot in the staging, and
// whether the kernels read it (IN), write it (OUT) or both.  `at`: the chunk's part as the kernels see it, set by chunks().
enum { IN = 1, OUT = 2 };
struct Arr {
    void *caller; size_t stride; void *stage; int dir;
    uint8_t *at = nullptr;
    template <class T> T *as() const { return (T *)at; }
};
Arr arr_in(const void *caller, size_t stride, void *stage) { return Arr{(void *)caller, stride, stage, IN}; }
Arr arr_out(void *caller, size_t stride, void *stage) { return Arr{caller, stride, stage, OUT}; }
Arr arr_inout(void *caller, size_t stride, void *stage) { return Arr{caller, stride, stage, IN | OUT}; }

// The scene's two events around a stretch of launches; add() reads them once the stream has been waited for.
struct Timer {
    rt_scene *scene; hipStream_t stream; float ms = 0.f;
    void start() { HIP_CHECK(hipEventRecord(scene->ev_start, stream)); }
    void stop() { HIP_CHECK(hipEventRecord(scene->ev_stop, stream)); }
    void add() { float t = 0.f; HIP_CHECK(hipEventElapsedTime(&t, scene->ev_start, scene->ev_stop)); ms += t; }
};

// One call over `items` items in chunks.  Host arrays: the in-arrays of a chunk are copied to the staging, body(first, m) finds the
// staging in Arr::at, the out-arrays are copied back.  Device pointers: body finds the caller's own memory from `first` on and nothing
// is copied.  Either way a chunk ends with one synchronisation, the next reuses the staging; `timer` (nullable) then reads its events.
// body returns RT_OK or the refusal that ends the call.  `arrays`: the call's own struct of nothing but Arr members, so that the call
// names each array where it declares it and where it builds its view, and the loop sees them all.
template <class Arrays, class Body>
int chunks(size_t items, size_t chunk_items, bool on_device, Arrays &arrays, hipStream_t stream, Timer *timer, Body body) {
    static_assert(std::is_standard_layout<Arrays>::value && sizeof(Arrays) % sizeof(Arr) == 0, "a struct of Arr members and nothing else");
    Arr *const A = reinterpret_cast<Arr *>(&arrays), *const A_end = A + sizeof(Arrays) / sizeof(Arr);
    for (size_t first = 0; first < items; first += chunk_items) {
        const size_t m = std::min(chunk_items, items - first);
        for (Arr *a = A; a != A_end; a++) {
            uint8_t *own = a->caller ? (uint8_t *)a->caller + first * a->stride : nullptr;
            a->at = !own ? nullptr : on_device ? own : (uint8_t *)a->stage;
            if (own && !on_device && (a->dir & IN)) HIP_CHECK(hipMemcpyAsync(a->stage, own, m * a->stride, hipMemcpyHostToDevice, stream));
        }
        if (const int rc = body(first, m)) return rc;
        for (const Arr *a = A; a != A_end; a++)
            if (a->caller && !on_device && (a->dir & OUT)) HIP_CHECK(hipMemcpyAsync((uint8_t *)a->caller + first * a->stride, a->stage, m * a->stride, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        if (timer) timer->add();
    }
    return RT_OK;
}

// ---- the stats shell ------------------------------------------------------------------------------------------------------------------------
uint64_t &items_of(rt_query_stats &st) { return st.rays; }
uint64_t &items_of(rt_bake_stats &st) { return st.points; }
void invalid_total(rt_query_stats &st, uint64_t invalid) { st.invalid_rays = invalid; }
void invalid_total(rt_bake_stats &, uint64_t) {} // the baker counts its invalid points itself

// A call over n items under the guard: work(st) fills in what it did (n == 0: nothing to do) and returns RT_OK or its refusal.
template <class Stats, class Work>
int with_stats(const rt_scene *scene, size_t n, Stats *stats, const std::string &who, Work work) {
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        Stats st{};
        st.struct_size = sizeof(Stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        items_of(st) = n;
        if (n)
            if (const int rc = work(st)) return rc;
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
        return RT_OK;
    });
}

// A chunk of a composed call as its launch body sees it: m slots (items x K) from item `first` on.
struct Chunk { const QueryStage &S; size_t first, m; hipStream_t stream; Timer &T; };
const auto no_prepare = [](const Chunk &, const auto &) {};

// The composed calls: n items of K slots through the scene's staging.  declare(S) names the caller's arrays; per chunk prepare(chunk, arrays)
// runs before the counters are zeroed and the clock starts, body(chunk, arrays, st) builds its views, launches and returns the number
// of launches.  The totals of all walks are read once, after the last chunk.
template <class Stats, class Declare, class Prepare, class Body>
int answer(rt_scene *scene, size_t n, size_t K, Stats *stats, const std::string &who, const StageSpec &spec, bool on_device, Declare declare, Prepare prepare, Body body) {
    return with_stats(scene, n, stats, who, [&](Stats &st) -> int {
        HIP_CHECK(hipSetDevice(scene->device));
        hipStream_t stream = nullptr;
        const QueryStage S = query_stage(scene, spec);
        auto A = declare(S);
        Timer T{scene, stream};
        HIP_CHECK(hipMemsetAsync(S.totals, 0, RQ_TOTAL_WORDS * 8, stream));
        const int rc = chunks(n, query_chunk() / K, on_device, A, stream, &T, [&](size_t first, size_t items) -> int { // whole items: K <= 64, the chunk's minimum
            const Chunk c{S, first, items * K, stream, T};
            prepare(c, A);
            HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
            T.start();
            st.launches += body(c, A, st);
            T.stop();
            return RT_OK;
        });
        if (rc) return rc;
        unsigned long long totals[RQ_TOTAL_WORDS];
        HIP_CHECK(hipMemcpy(totals, S.totals, sizeof totals, hipMemcpyDeviceToHost));
        st.exact_walks = totals[RQ_TOTAL_EXACT] + totals[RQ_TOTAL_RIDE_EXACT];
        invalid_total(st, totals[RQ_TOTAL_INVALID]);
        st.kernel_ms = T.ms;
        return RT_OK;
    });
}

// ---- views and launches that several calls share --------------------------------------------------------------------------------------------
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
    if (const int rc = check_walk_call(scene, stats, flags, WALK_FLAGS, who)) return rc;
    if (light && scene->view.n_lights == 0) return fail(RT_ERR_INVALID_ARG, who + "the scene has no lights: there is no light pdf to ask for");
    if (n && (!rays || !out)) return null_arg(who);
    const bool on_device = device_pointers(flags);
    if (const int rc = check_aligned(n && on_device && !light, {out}, 16, "the rt_hit array", who)) return rc;
    struct A { Arr rays, out; };
    return answer(scene, n, 1, stats, who, {STAGE_WALK}, on_device,
        [&](const QueryStage &S) { return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_out(out, light ? sizeof(float) : sizeof(rt_hit), S.out)}; }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            QueryView Q = walk_view(scene, c.S, c.m, flags, a.rays.as<float>());
            if (light) Q.pdf = a.out.as<float>(); else Q.hits = a.out.as<uint4>();
            return light ? query_launch_light_pdf(scene, Q, c.stream) : query_launch_closest(scene, Q, c.stream);
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

// A chunk's records as the bounce step's kernels see them: the caller's device arrays from the chunk's first on, or the staging.
ScatterView scatter_view(const QueryStage &S, size_t m, const void *rays, const void *hits, const void *surfaces, void *rng, void *out) {
    ScatterView V{};
    V.rays = (const float *)rays; V.hits = (const uint4 *)hits; V.surfaces = (const uint4 *)surfaces;
    V.rng = (uint4 *)rng; V.out = (uint4 *)out;
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

// The paths of rt_trace_paths and rt_bake run over the staging: rays, hits, surfaces and scatter records there, the engines at `rng`.
// Their per-bounce stack for `paths` paths of a chunk: 16 bytes of state (zeroed per chunk: tail 0, no bounce kept, not ended), then
// 24 bytes per bounce.
struct Paths { ScatterView V; PathView P; };
void prepare_paths(rt_scene *scene, size_t paths, int depth, hipStream_t stream) {
    ensure_materials(scene, stream);
    grow(scene->path_stack, scene->path_stack_bytes, paths * (16u + 24u * (size_t)depth));
    HIP_CHECK(hipMemsetAsync(scene->path_stack, 0, paths * 16u, stream));
}
Paths paths_view(const rt_scene *scene, const Chunk &c, void *rng, size_t paths) {
    const QueryStage &S = c.S;
    Paths p{scatter_view(S, c.m, S.rays, S.out, S.surf, rng, S.scat), PathView{}};
    p.P.rays = S.rays; p.P.hits = p.V.hits; p.P.surfaces = p.V.surfaces; p.P.scatter = p.V.out;
    p.P.state = (float4 *)scene->path_stack; p.P.stack = (float *)(scene->path_stack + paths * 16u);
    p.P.n = (uint32_t)c.m;
    return p;
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

// ---- rt_render_paths / rt_render_bake / rt_render_probes: the caller's paths through the persistent kernel (device/rt_path_source.h) ---------
// Slots per chunk: the pixel slots of a 1080p frame, so the persistent kernel's path records (256 bytes per slot at depth 6) never grow
// beyond what rt_render of that frame allocates, and workload A of profiles/r30_render_paths.txt is one launch.  RTAMD_QUERY_CHUNK
// lowers it as it does for the composed calls.
const size_t SOURCE_CHUNK = 2073600;
size_t source_chunk() { return std::min(SOURCE_CHUNK, (size_t)std::max(64, env_positive("RTAMD_QUERY_CHUNK", (int)SOURCE_CHUNK))); }

} // namespace
// The same loop for rtamd_adaptive.hip, whose chunks are stretches of its list of active sub-tiles and carry no caller arrays.
size_t rtamd::source_chunk_slots() { return source_chunk(); }
int rtamd::source_chunks(size_t items, size_t chunk_items, hipStream_t stream, const std::function<int(size_t first, size_t m)> &body) {
    struct { Arr none; } A{Arr{nullptr, 0u, nullptr, 0}};
    return chunks(items, chunk_items, true, A, stream, nullptr, body);
}
namespace {

// One call: `items` rays (K = 1) or points of K slots each.  `in`: the rays or the points, 24 bytes an item.  `floats`: the answer per item,
// 3, or 27 for SH9 probes (mode 3), whose slots also keep 120 bytes each beside the state: the first direction and the 27 accumulators.
struct SourceCall {
    uint32_t mode; size_t K; int32_t depth, samples; float scale; // samples: per slot
    size_t floats;
    const void *in; rt_rng *rng; float *out; bool on_device;
};
struct SourceTotals { double kernel_ms = 0; uint32_t launches = 0, reference_exact = 0; uint64_t exact_walks = 0, no_path = 0; };

int source_run(rt_scene *scene, const SourceCall &c, size_t items, const std::string &who, SourceTotals &T) {
    HIP_CHECK(hipSetDevice(scene->device));
    hipStream_t stream = nullptr;
    const size_t chunk_items = source_chunk() / c.K; // whole points: the stream sum never crosses a seam (the chunk's minimum of 64 covers K <= 64)
    const size_t cap_items = std::min(items, chunk_items), cap = (cap_items * c.K + 63u) & ~(size_t)63u;
    const bool probes = c.mode == 3u;
    struct { uint32_t *state; float *sh; uint8_t *in, *rng; float *out; } S{}; // the kernel's state; host arrays: the records, the engines, the answer
    auto carve = [&](uint8_t *base) {
        Carver take{base};
        take(S.state, cap * 24u);
        take(S.sh, probes ? cap * 120u : 0u);
        if (!c.on_device) { take(S.in, cap_items * 24u); take(S.rng, cap * sizeof(rt_rng)); take(S.out, cap_items * c.floats * 4u); }
        return take.at;
    };
    grow(scene->source_stage, scene->source_stage_bytes, carve(nullptr));
    carve(scene->source_stage);
    struct { Arr in, rng, out; } A{arr_in(c.in, 24u, S.in), arr_inout(c.rng, c.K * sizeof(rt_rng), S.rng), arr_out(c.out, c.floats * 4u, S.out)};
    return chunks(items, chunk_items, c.on_device, A, stream, nullptr, [&](size_t, size_t m_items) -> int {
        SourceView V{};
        V.state = S.state; V.n = (uint32_t)(m_items * c.K); V.n_pixslots = (V.n + 63u) & ~63u; V.mode = c.mode;
        V.rng = A.rng.as<uint4>();
        if (c.mode == 1u) V.rays = A.in.as<float>(); else V.points = A.in.as<float>();
        if (probes) V.sh = S.sh; // shares its room with `rays`, which probes have none of
        V.streams = (uint32_t)c.K; V.scale = c.scale;
        V.out = A.out.as<float>();
        T.launches += query_launch_source_pack(scene, V, stream);
        SourceChunk C{};
        C.mode = c.mode; C.n = V.n; C.streams = V.streams; C.rays = c.mode == 1u ? V.rays : nullptr; C.points = V.points;
        C.ray_depth = c.depth; C.samples = c.samples; C.state = V.state; C.sh = S.sh;
        SourceResult res{};
        if (const int rc = source_render(scene, C, stream, res, who)) return rc;
        T.launches += res.launches + query_launch_source_unpack(scene, V, stream);
        T.kernel_ms += res.kernel_ms; T.exact_walks += res.exact_walks; T.no_path += res.no_path; T.reference_exact = res.reference_exact;
        return RT_OK;
    });
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
    // what can be judged without the scene first, each refusal naming its argument
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_flags(flags, WALK_FLAGS, who)) return rc;
    if (n && !rays) return null_arg(who, "rays");
    if (n && !out) return null_arg(who, "out");
    if (const int rc = check_scene(scene, who, "scene")) return rc;
    const bool on_device = device_pointers(flags);
    if (const int rc = check_aligned(n && on_device, {tmax}, 4, "the tmax array", who)) return rc;
    struct A { Arr rays, tmax, out; };
    return answer(scene, n, 1, stats, who, {STAGE_OCCLUSION}, on_device,
        [&](const QueryStage &S) { return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_in(tmax, sizeof(float), S.tmax), arr_out(out, 1, S.occ)}; }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            QueryView Q = walk_view(scene, c.S, c.m, flags, a.rays.as<float>());
            Q.tmax = a.tmax.as<float>(); Q.occ = a.out.at;
            return query_launch_occluded(scene, Q, c.stream);
        });
}

int rt_query_surface(rt_scene *scene, const rt_hit *hits, size_t n, uint32_t flags, rt_surface *out, rt_query_stats *stats) {
    const std::string who = "rt_query_surface: ";
    if (const int rc = check_walk_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (n && (!hits || !out)) return null_arg(who);
    const bool on_device = device_pointers(flags);
    if (const int rc = check_aligned(n && on_device, {hits, out}, 16, "the rt_hit and rt_surface arrays", who)) return rc;
    struct A { Arr hits, out; };
    return answer(scene, n, 1, stats, who, {STAGE_FIRST_HIT}, on_device,
        [&](const QueryStage &S) { return A{arr_in(hits, sizeof(rt_hit), S.out), arr_out(out, sizeof(rt_surface), S.surf)}; },
        [&](const Chunk &c, const A &) { ensure_materials(scene, c.stream); },
        [&](const Chunk &c, const A &a, rt_query_stats &) { return query_launch_surface(scene, surface_view(scene, c.S, c.m, a.hits.at, a.out.at), c.stream); });
}

int rt_query_environment(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_query_environment: ";
    if (const int rc = check_walk_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (n && (!rays || !out_rgb)) return null_arg(who);
    struct A { Arr rays, rgb; };
    return answer(scene, n, 1, stats, who, {STAGE_WALK}, device_pointers(flags), // the colours of a chunk are staged where a closest-hit query keeps its 16-byte records
        [&](const QueryStage &S) { return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_out(out_rgb, 3 * sizeof(float), S.rec)}; }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            EnvironmentView V{};
            V.rays = a.rays.as<float>(); V.rgb = a.rgb.as<float>();
            V.n = (uint32_t)c.m; V.totals = c.S.totals;
            return query_launch_environment(scene, V, c.stream);
        });
}

int rt_camera_rays(rt_scene *scene, int32_t width, int32_t height, const float *xy, size_t n, uint32_t flags, rt_ray *out) {
    const std::string who = "rt_camera_rays: ";
    if (const int rc = check_walk_call(scene, nullptr, flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, who + "width and height must be positive");
    if (n && (!xy || !out)) return null_arg(who);
    const bool on_device = device_pointers(flags);
    if (!on_device)
        for (size_t i = 0; i < 2 * n; i++)
            if (!std::isfinite(xy[i])) return fail(RT_ERR_INVALID_ARG, who + "xy holds a NaN or an infinity (point " + std::to_string(i / 2) + ")");
    struct A { Arr xy, rays; };
    return answer(scene, n, 1, (rt_query_stats *)nullptr, who, {STAGE_WALK}, on_device, // the points of a chunk are staged where a closest-hit query keeps its 16-byte records
        [&](const QueryStage &S) { return A{arr_in(xy, 2 * sizeof(float), S.rec), arr_out(out, sizeof(rt_ray), S.rays)}; }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            CameraView V{};
            V.xy = a.xy.as<float>(); V.rays = a.rays.as<float>();
            V.n = (uint32_t)c.m; V.width = width; V.height = height;
            return query_launch_camera_rays(scene, V, c.stream);
        });
}

int rt_render_guides(rt_scene *scene, int32_t width, int32_t height, uint32_t flags, float *albedo, float *normal, float *depth, float *emission,
                     rt_query_stats *stats) {
    const std::string who = "rt_render_guides: ";
    if (const int rc = check_walk_call(scene, stats, flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, who + "width and height must be positive");
    if ((int64_t)width * height >= 2147483647LL) return fail(RT_ERR_INVALID_ARG, who + "image too large (width * height must stay below 2^31-1)");
    struct A { Arr albedo, normal, depth, emission; };
    return answer(scene, (size_t)width * height, 1, stats, who, {STAGE_FIRST_HIT}, device_pointers(flags),
        [&](const QueryStage &S) { // the planes of a chunk in the staging: 3 + 3 + 1 + 3 floats per pixel of a whole chunk, in this order
            float *const p = S.planes;
            return A{arr_out(albedo, 12, p), arr_out(normal, 12, p + 3 * QUERY_CHUNK), arr_out(depth, 4, p + 6 * QUERY_CHUNK), arr_out(emission, 12, p + 7 * QUERY_CHUNK)};
        },
        [&](const Chunk &c, const A &) { ensure_materials(scene, c.stream); },
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            const QueryStage &S = c.S;
            CameraView C{};
            C.rays = S.rays; C.n = (uint32_t)c.m; C.first_pixel = (uint32_t)c.first; C.width = width; C.height = height;
            uint32_t launches = query_launch_camera_rays(scene, C, c.stream);
            QueryView Q = walk_view(scene, S, c.m, 0u, S.rays);
            Q.hits = (uint4 *)S.out;
            launches += query_launch_closest(scene, Q, c.stream);
            launches += query_launch_surface(scene, surface_view(scene, S, c.m, S.out, S.surf), c.stream);
            GuidesView G{};
            G.hits = (const uint4 *)S.out; G.surfaces = (const uint4 *)S.surf; G.rays = S.rays; G.n = (uint32_t)c.m;
            G.albedo = a.albedo.as<float>(); G.normal = a.normal.as<float>(); G.depth = a.depth.as<float>(); G.emission = a.emission.as<float>(); // null: not wanted
            return launches + query_launch_guides(scene, G, c.stream);
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

// rt_query_scatter, rt_query_bsdf and rt_trace_paths judge everything that needs no scene first.
int rt_query_scatter(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, rt_rng *rng, size_t n, uint32_t flags,
                     rt_scatter *out, rt_query_stats *stats) {
    const std::string who = "rt_query_scatter: ";
    const bool on_device = device_pointers(flags);
    if (n && (!rays || !hits || !surfaces || !rng || !out)) return null_arg(who);
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_flags(flags, WALK_FLAGS, who)) return rc;
    if (const int rc = check_engines(rng, n, on_device, who)) return rc;
    if (const int rc = check_scene(scene, who)) return rc;
    if (const int rc = check_aligned(n && on_device, {hits, surfaces, rng, out}, 16, "the rt_hit, rt_surface, rt_rng and rt_scatter arrays", who)) return rc;
    struct A { Arr rays, hits, surfaces, rng, out; };
    return answer(scene, n, 1, stats, who, {STAGE_SCATTER}, on_device,
        [&](const QueryStage &S) {
            return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_in(hits, sizeof(rt_hit), S.out), arr_in(surfaces, sizeof(rt_surface), S.surf),
                     arr_inout(rng, sizeof(rt_rng), S.rng), arr_out(out, sizeof(rt_scatter), S.scat)};
        }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            const ScatterView V = scatter_view(c.S, c.m, a.rays.at, a.hits.at, a.surfaces.at, a.rng.at, a.out.at);
            uint32_t launches = query_launch_scatter_sample(scene, V, c.stream);
            launches += launch_ride_light_pdf(scene, c.S, c.m, flags, false, c.stream);
            return launches + query_launch_scatter_finish(scene, V, c.stream);
        });
}

int rt_query_bsdf(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, const float *dirs, size_t n, uint32_t flags,
                  float *out_brdf, float *out_pdf, rt_query_stats *stats) {
    const std::string who = "rt_query_bsdf: ";
    const bool on_device = device_pointers(flags);
    if (n && (!rays || !hits || !surfaces || !dirs || !out_brdf || !out_pdf)) return null_arg(who);
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_flags(flags, WALK_FLAGS, who)) return rc;
    if (const int rc = check_scene(scene, who)) return rc;
    if (const int rc = check_aligned(n && on_device, {hits, surfaces}, 16, "the rt_hit and rt_surface arrays", who)) return rc;
    if (const int rc = check_aligned(n && on_device, {dirs, out_brdf, out_pdf}, 4, "dirs, out_brdf and out_pdf", who)) return rc;
    struct A { Arr rays, hits, surfaces, dirs, brdf, pdf; };
    return answer(scene, n, 1, stats, who, {STAGE_SCATTER}, on_device,
        [&](const QueryStage &S) { // host arrays: the directions and the two answers of a chunk are staged where a scatter keeps its records (3 + 3 + 1 floats per record)
            float *const f = (float *)S.scat;
            return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_in(hits, sizeof(rt_hit), S.out), arr_in(surfaces, sizeof(rt_surface), S.surf),
                     arr_in(dirs, 12, f), arr_out(out_brdf, 12, f + 3 * QUERY_CHUNK), arr_out(out_pdf, 4, f + 6 * QUERY_CHUNK)};
        }, no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            ScatterView V = scatter_view(c.S, c.m, a.rays.at, a.hits.at, a.surfaces.at, nullptr, nullptr);
            V.dirs = a.dirs.as<float>(); V.out_brdf = a.brdf.as<float>(); V.out_pdf = a.pdf.as<float>();
            uint32_t launches = query_launch_bsdf_rays(scene, V, c.stream);
            launches += launch_ride_light_pdf(scene, c.S, c.m, flags, false, c.stream);
            return launches + query_launch_bsdf_finish(scene, V, c.stream);
        });
}

int rt_trace_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng, size_t n, int32_t ray_depth, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_trace_paths: ";
    const bool on_device = device_pointers(flags);
    int depth = 0;
    if (n && (!rays || !rng || !out_rgb)) return null_arg(who);
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_flags(flags, WALK_FLAGS, who)) return rc;
    if (const int rc = check_engines(rng, n, on_device, who)) return rc;
    if (const int rc = check_scene(scene, who)) return rc;
    if (const int rc = check_depth(ray_depth, who, "", depth)) return rc;
    if (const int rc = check_engine_arrays(n && on_device, rng, rays, out_rgb, "rays and out_rgb", who)) return rc;
    const size_t paths = std::min(n, query_chunk());
    struct A { Arr rays, rng, rgb; };
    return answer(scene, n, 1, stats, who, {STAGE_SCATTER}, on_device, // the colours of a chunk are staged where a closest-hit query keeps its records
        [&](const QueryStage &S) { return A{arr_in(rays, sizeof(rt_ray), S.rays), arr_inout(rng, sizeof(rt_rng), S.rng), arr_out(out_rgb, 12, S.rec)}; },
        [&](const Chunk &c, const A &a) {
            prepare_paths(scene, paths, depth, c.stream);
            // the rays change from bounce to bounce: always a copy in the staging
            if (on_device) HIP_CHECK(hipMemcpyAsync(c.S.rays, a.rays.at, c.m * sizeof(rt_ray), hipMemcpyDeviceToDevice, c.stream));
        },
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            Paths p = paths_view(scene, c, a.rng.at, paths);
            p.P.rgb = a.rgb.as<float>();
            uint32_t launches = 0;
            for (int b = 0; b < depth; b++) {
                launches += launch_round(scene, c.S, p.V, c.m, flags, b != 0, c.stream);
                p.P.last = b == depth - 1 ? 1u : 0u;
                launches += query_launch_path_advance(scene, p.P, c.stream);
            }
            return launches;
        });
}

// The bake calls judge everything that needs no scene first, too.
int rt_bake_rays(rt_scene *scene, const rt_bake_point *points, rt_rng *rng, size_t n, int32_t mode, uint32_t flags, rt_ray *out, rt_query_stats *stats) {
    const std::string who = "rt_bake_rays: ";
    const bool on_device = device_pointers(flags);
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_bake_mode(mode, who, "mode")) return rc;
    if (const int rc = check_flags(flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (const int rc = check_bake_arrays(scene, nullptr, points, rng, out, n, 1, on_device, who)) return rc;
    struct A { Arr points, rng, out; };
    return answer(scene, n, 1, stats, who, {STAGE_BAKE}, on_device, // the points of a chunk are staged with the baker's state
        [&](const QueryStage &S) { return A{arr_in(points, sizeof(rt_bake_point), S.bake_points), arr_inout(rng, sizeof(rt_rng), S.rng), arr_out(out, sizeof(rt_ray), S.rays)}; },
        no_prepare,
        [&](const Chunk &c, const A &a, rt_query_stats &) {
            BakeView B{};
            B.points = a.points.as<float>(); B.rng = a.rng.as<uint4>(); B.rays = a.out.as<float>();
            B.totals = c.S.totals; B.n = (uint32_t)c.m; B.streams = 1u; B.mode = mode;
            return query_launch_bake_rays(scene, B, c.stream);
        });
}

int rt_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params, rt_rng *rng, float *out, rt_bake_stats *stats) {
    const std::string who = "rt_bake: ";
    size_t K = 1;
    int depth = 0;
    if (const int rc = check_bake_params(params, stats, n_points, WALK_FLAGS | RT_BAKE_LOCKSTEP, who, K, depth)) return rc;
    const uint32_t flags = params->flags, walk_flags = flags & WALK_FLAGS;
    const bool on_device = device_pointers(flags), lockstep = (flags & RT_BAKE_LOCKSTEP) != 0;
    if (const int rc = check_bake_arrays(scene, "scene", points, rng, out, n_points, K, on_device, who)) return rc;
    const size_t floats = params->mode == RT_BAKE_SH9 ? 27u : 3u;
    const uint32_t q = (uint32_t)((size_t)params->samples / K);
    const double pi = 3.14159265358979323846;
    const float scale = params->mode == RT_BAKE_SH9 ? (float)(4.0 * pi / (double)params->samples) : (float)(pi / (double)params->samples);
    const size_t slots_max = std::min(n_points, query_chunk() / K) * K; // a chunk holds whole points: the stream sum never crosses a seam
    struct A { Arr points, rng, out; };
    return answer(scene, n_points, K, stats, who, StageSpec{STAGE_BAKE, floats, !on_device}, on_device,
        [&](const QueryStage &S) { return A{arr_in(points, sizeof(rt_bake_point), S.bake_points), arr_inout(rng, K * sizeof(rt_rng), S.rng), arr_out(out, floats * sizeof(float), S.bake_out)}; },
        [&](const Chunk &c, const A &) {
            prepare_paths(scene, slots_max, depth, c.stream);
            HIP_CHECK(hipMemsetAsync(c.S.bake_ctr, 0, RQ_BAKE_CTR_WORDS * 8, c.stream));
        },
        [&](const Chunk &c, const A &a, rt_bake_stats &st) {
            const QueryStage &S = c.S;
            const Paths p = paths_view(scene, c, a.rng.at, slots_max);
            BakeView B{};
            B.points = a.points.as<float>(); B.out = a.out.as<float>();
            B.rng = p.V.rng; B.rays = S.rays; B.dir0 = params->mode == RT_BAKE_SH9 ? S.bake_dir0 : nullptr; B.acc = S.bake_acc; B.left = S.bake_left;
            B.ctr = S.bake_ctr; B.totals = S.totals;
            B.n = (uint32_t)c.m; B.streams = (uint32_t)K; B.per_stream = q; B.depth = (uint32_t)depth; B.lockstep = lockstep ? 1u : 0u;
            B.mode = params->mode; B.floats = (uint32_t)floats; B.scale = scale;
            unsigned long long ctr[RQ_BAKE_CTR_WORDS] = {};
            auto poll = [&]() { c.T.stop(); HIP_CHECK(hipMemcpy(ctr, S.bake_ctr, sizeof ctr, hipMemcpyDeviceToHost)); c.T.add(); }; // waits for the stream
            uint64_t rounds = 0;
            uint32_t launches = query_launch_bake_rays(scene, B, c.stream);
            auto round = [&](bool last) {
                launches += launch_round(scene, S, p.V, c.m, walk_flags, rounds != 0, c.stream);
                B.last = last ? 1u : 0u;
                launches += query_launch_bake_advance(scene, p.P, B, c.stream);
                rounds++;
            };
            if (lockstep) { // the plain composition: every slot starts sample j in the same round, every sample takes `depth` rounds
                for (uint32_t j = 0; j < q; j++)
                    for (int b = 0; b < depth; b++) round(b == depth - 1);
                poll();
            } else {        // regeneration: a round at a time, until every valid slot is parked
                for (poll(); ctr[RQ_BAKE_CTR_PARKED] < ctr[RQ_BAKE_CTR_SLOTS]; poll()) {
                    c.T.start();
                    round(false);
                }
            }
            c.T.start();
            BakeView R = B;
            R.n = (uint32_t)(c.m / K * floats);
            st.invalid_points += ctr[RQ_BAKE_CTR_INVALID_POINTS];
            st.paths += ctr[RQ_BAKE_CTR_SLOTS] * q;
            st.live_ray_slots += ctr[RQ_BAKE_CTR_LIVE_RAY_SLOTS];
            st.rounds += rounds;
            st.ray_slots += rounds * c.m;
            return launches + query_launch_bake_resolve(scene, R, c.stream);
        });
}

int rt_render_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng, size_t n, int32_t ray_depth, uint32_t flags, float *out_rgb, rt_query_stats *stats) {
    const std::string who = "rt_render_paths: ";
    const bool on_device = device_pointers(flags);
    int depth = 0;
    if (n && (!rays || !rng || !out_rgb)) return null_arg(who);
    if (const int rc = check_struct_size(stats, who)) return rc;
    if (const int rc = check_flags(flags, RT_QUERY_DEVICE_POINTERS, who)) return rc;
    if (const int rc = check_engines(rng, n, on_device, who)) return rc;
    if (const int rc = check_depth(ray_depth, who, "", depth)) return rc;
    if (const int rc = check_scene(scene, who)) return rc;
    if (const int rc = check_engine_arrays(n && on_device, rng, rays, out_rgb, "rays and out_rgb", who)) return rc;
    if (const int rc = source_check(scene, (uint32_t)std::min(std::max<size_t>(n, 1u), source_chunk()), depth, 1, who)) return rc;
    return with_stats(scene, n, stats, who, [&](rt_query_stats &st) -> int {
        SourceTotals T;
        if (const int rc = source_run(scene, SourceCall{1u, 1u, depth, 1, 0.f, 3u, rays, rng, out_rgb, on_device}, n, who, T)) return rc;
        st.exact_walks = T.exact_walks; st.invalid_rays = T.no_path; st.kernel_ms = T.kernel_ms; st.launches = T.launches;
        st.reference_exact = T.reference_exact;
        return RT_OK;
    });
}

int rt_render_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params, rt_rng *rng, float *out, rt_bake_stats *stats) {
    const std::string who = "rt_render_bake: ";
    size_t K = 1;
    int depth = 0;
    if (const int rc = check_bake_params(params, stats, n_points, RT_QUERY_DEVICE_POINTERS, who, K, depth)) return rc;
    const size_t q = (size_t)params->samples / K;
    if (q >= ((size_t)1 << 25)) return fail(RT_ERR_LIMIT, who + "params.samples / params.streams must stay below 2^25 (the path record's sample index)");
    if (params->mode == RT_BAKE_SH9)
        return fail(RT_ERR_UNSUPPORTED, who + "RT_BAKE_SH9 does not fit the persistent kernel's path record (27 accumulators and the first direction): rt_bake serves it");
    const bool on_device = device_pointers(params->flags);
    if (const int rc = check_bake_arrays(scene, "scene", points, rng, out, n_points, K, on_device, who)) return rc;
    if (const int rc = source_check(scene, (uint32_t)std::min(std::max<size_t>(n_points, 1u) * K, source_chunk()), depth, (int32_t)q, who)) return rc;
    const double pi = 3.14159265358979323846;
    const float scale = (float)(pi / (double)params->samples);
    return with_stats(scene, n_points, stats, who, [&](rt_bake_stats &st) -> int {
        SourceTotals T;
        if (const int rc = source_run(scene, SourceCall{2u, K, depth, (int32_t)q, scale, 3u, points, rng, out, on_device}, n_points, who, T)) return rc;
        st.invalid_points = T.no_path; st.paths = (n_points - T.no_path) * K * q; st.exact_walks = T.exact_walks;
        st.kernel_ms = T.kernel_ms; st.launches = T.launches; st.reference_exact = T.reference_exact;
        return RT_OK;
    });
}

int rt_render_probes(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params, rt_rng *rng, float *out, rt_bake_stats *stats) {
    const std::string who = "rt_render_probes: ";
    size_t K = 1;
    int depth = 0;
    if (const int rc = check_bake_params(params, stats, n_points, RT_QUERY_DEVICE_POINTERS, who, K, depth)) return rc;
    const size_t q = (size_t)params->samples / K;
    if (q >= ((size_t)1 << 25)) return fail(RT_ERR_LIMIT, who + "params.samples / params.streams must stay below 2^25 (the path record's sample index)");
    if (params->mode == RT_BAKE_IRRADIANCE)
        return fail(RT_ERR_INVALID_ARG, who + "params.mode = RT_BAKE_IRRADIANCE: this call bakes RT_BAKE_SH9 probes, rt_render_bake serves irradiance");
    const bool on_device = device_pointers(params->flags);
    if (const int rc = check_bake_arrays(scene, "scene", points, rng, out, n_points, K, on_device, who)) return rc;
    if (const int rc = source_check(scene, (uint32_t)std::min(std::max<size_t>(n_points, 1u) * K, source_chunk()), depth, (int32_t)q, who)) return rc;
    const double pi = 3.14159265358979323846;
    const float scale = (float)(4.0 * pi / (double)params->samples);
    return with_stats(scene, n_points, stats, who, [&](rt_bake_stats &st) -> int {
        SourceTotals T;
        if (const int rc = source_run(scene, SourceCall{3u, K, depth, (int32_t)q, scale, 27u, points, rng, out, on_device}, n_points, who, T)) return rc;
        st.invalid_points = T.no_path; st.paths = (n_points - T.no_path) * K * q; st.exact_walks = T.exact_walks;
        st.kernel_ms = T.kernel_ms; st.launches = T.launches; st.reference_exact = T.reference_exact;
        return RT_OK;
    });
}

} // extern "C"

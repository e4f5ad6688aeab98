// One chunk of a batched ray query as its kernels see it (rt_query.h), and what the host side (rtamd_query.hip) asks of the translation
// unit that holds them (rtamd_api.hip: every __global__ keeps one definition there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

struct rt_scene;

namespace rtamd {

// Counter words of a chunk (QueryView::ctr; zeroed before every chunk) and of a call (QueryView::totals; zeroed once per call).
enum { RQ_CTR_FAST = 0,      // rays on the fast list (q_fast)
       RQ_CTR_EXACT = 1,     // rays on the exact list (q_exact)
       RQ_CTR_HEAD = 2,      // dynamic tail of the fast list (wf_steal)
       RQ_CTR_WORDS = 4 };
// RQ_TOTAL_RIDE_*: the same two of a walk whose invalid rays are records that ride along (rt_query_scatter's light walk, rt_trace_paths'
// later bounces; QueryView::totals then points at RQ_TOTAL_RIDE_EXACT): its exact walks count for the call, its invalid rays for nothing.
enum { RQ_TOTAL_EXACT = 0, RQ_TOTAL_INVALID = 1, RQ_TOTAL_RIDE_EXACT = 2, RQ_TOTAL_RIDE_INVALID = 3, RQ_TOTAL_WORDS = 4 };

struct QueryView {
    const float *rays;            // n x {o.xyz, d.xyz} (rt_ray): the chunk's rays, staged or the caller's own device memory
    uint32_t n;
    uint32_t reference_walk;      // RT_QUERY_REFERENCE_WALK: every valid ray goes on the exact list
    float origin_bound;           // max |coordinate| of scene and camera: what the gate's margin box_c2 was derived for (rt_query.h)
    float4 *rec;                  // closest hit, per ray: t, u, v, hit word with the gap code (what WfClosest::store leaves in a path record)
    uint32_t *q_fast, *q_exact;   // ray indices, n words each
    uint32_t *ctr;                // RQ_CTR_*
    unsigned long long *totals;   // RQ_TOTAL_*
    uint4 *hits;                  // closest hit: 4 per ray (rt_hit), 16-byte aligned
    float *pdf;                   // light pdf: 1 per ray
    const float *tmax;            // occlusion: the bound per ray, 4-byte aligned; null = +inf for every ray
    uint8_t *occ;                 // occlusion: 1 byte per ray (RT_OCCLUSION_*), no alignment
    uint32_t *ovf;                // SPILL variant: WF_OVF words per persistent thread
};

// The first-hit layer (rt_query_surface.h): one chunk of each call as its kernel sees it.
struct SurfaceView {
    const uint4 *hits;            // n x 4 (rt_hit), 16-byte aligned: what rt_query_closest wrote, or the caller's own
    uint4 *out;                   // n x 4 (rt_surface), 16-byte aligned
    uint32_t n, n_tris;
    const uint32_t *tri_material; // n_tris words: material index by LOAD-order triangle (rt_scene::query_materials)
    unsigned long long *totals;   // RQ_TOTAL_*
};
struct EnvironmentView {
    const float *rays;            // n x {o.xyz, d.xyz}
    float *rgb;                   // n x 3
    uint32_t n;
    unsigned long long *totals;
};
struct CameraView {
    const float *xy;              // n x {nx, ny} in pixel units; null = the centres of the pixels first_pixel .. first_pixel + n in frame order
    float *rays;                  // n x {o.xyz, d.xyz}
    uint32_t n, first_pixel;
    int32_t width, height;
    float tan_fov_x;              // set by query_launch_camera_rays, as the render launch sets RenderView::tan_fov_x
};
struct GuidesView {
    const uint4 *hits, *surfaces; // the chunk's rt_hit and rt_surface records
    const float *rays;            // and its camera rays
    float *albedo, *normal, *depth, *emission; // the chunk's part of each plane; null = not wanted
    uint32_t n;
};

// The bounce step (rt_query_scatter.h): one chunk of rt_query_scatter, rt_query_bsdf and of one bounce of rt_trace_paths.
struct ScatterView {
    const float *rays;            // n x {o.xyz, d.xyz}: the rays that hit
    const uint4 *hits, *surfaces; // n x 4 each (rt_hit, rt_surface), 16-byte aligned
    uint4 *rng;                   // n (rt_rng), in and out, 16-byte aligned; unused by rt_query_bsdf
    uint4 *out;                   // n x 4 (rt_scatter), 16-byte aligned; unused by rt_query_bsdf
    const float *dirs;            // rt_query_bsdf: n x 3
    float *out_brdf, *out_pdf;    // rt_query_bsdf: n x 3, n
    float *walk_rays;             // n x {o.xyz, d.xyz}: what the light walk is asked, an invalid ray where no walk is needed
    const float *light_pdf;       // n: what it answered; not read on a scene without lights
    uint32_t n;
    unsigned long long *totals;   // RQ_TOTAL_*
};
// rt_trace_paths: the paths of a chunk between two bounces.
struct PathView {
    float *rays;                  // n x {o.xyz, d.xyz}: the bounce's rays in, the next bounce's out (an ended path: NaNs)
    const uint4 *hits, *surfaces, *scatter; // what the bounce's three queries answered
    float4 *state;                // n: tail.xyz, bounces kept | RQ_PATH_ENDED
    float *stack;                 // depth x n x {e.xyz, m.xyz}
    float *rgb;                   // n x 3, written after the last bounce
    uint32_t n, last;             // last: this was the last bounce, fold and write rgb
};

// The baker (rt_bake.h): the records of rt_bake_rays, or the slots of one chunk of rt_bake.  Slot s = point * streams + stream.
enum { RQ_BAKE_CTR_SLOTS = 0,          // valid slots of the chunk (the start launch)
       RQ_BAKE_CTR_PARKED = 1,         // of which every sample is in: the chunk is done when the two are equal
       RQ_BAKE_CTR_LIVE_RAY_SLOTS = 2, // closest-hit queries made for live paths
       RQ_BAKE_CTR_INVALID_POINTS = 3,
       RQ_BAKE_CTR_WORDS = 4 };
struct BakeView {
    const float *points;          // n / streams x {p.xyz, n.xyz} (rt_bake_point), 4-byte aligned
    uint4 *rng;                   // n (rt_rng), in and out, 16-byte aligned
    float *rays;                  // n x {o.xyz, d.xyz}: the ray of a record or of a slot's sample; an invalid ray for an invalid or parked one
    float *dir0;                  // rt_bake: n x 3, the first direction of the slot's sample in flight; null in rt_bake_rays
    float *acc;                   // rt_bake: floats x n, [j][slot]
    uint32_t *left;               // rt_bake: n, the slot's samples not yet in; null in rt_bake_rays
    float *out;                   // the resolve launch: n floats, [point][j]
    unsigned long long *ctr;      // RQ_BAKE_CTR_*
    unsigned long long *totals;   // RQ_TOTAL_* (rt_bake_rays counts its invalid records there)
    uint32_t n;                   // records or slots; in the resolve launch the floats of the chunk's answer
    uint32_t streams;             // K; 1 in rt_bake_rays
    uint32_t per_stream;          // q = samples / K
    uint32_t depth, lockstep, last; // the advance launch: ray_depth, RT_BAKE_LOCKSTEP, this round spends the depth
    int32_t mode;                 // RT_BAKE_IRRADIANCE or RT_BAKE_SH9
    uint32_t floats;              // 3 or 27
    float scale;
};

// rt_render_paths / rt_render_bake / rt_render_probes (rt_path_source.h): one chunk's slots between the caller's records and the state the persistent
// kernel runs over (RenderView::accum's layout: n_pixslots x {sum.xyz, Rng::x}, then n_pixslots x {Rng::saved, Rng::has_saved}).
struct SourceView {
    uint32_t *state;
    uint32_t n_pixslots;          // slots of the chunk's frame: n rounded up to whole 64-slot groups
    uint32_t n;                   // records (bake: points x streams)
    uint32_t mode;                // RenderView::src_mode: 1 = rays, 2 = bake irradiance, 3 = SH9 probes
    uint4 *rng;                   // n (rt_rng), in (pack) and out (unpack), 16-byte aligned
    union {                       // one pointer's room, as in RenderView: the two older kernels' argument block is laid out as before mode 3
        const float *rays;        // mode 1: n x {o.xyz, d.xyz}
        float *sh;                // mode 3: RenderView::src_sh, n_pixslots x 30 floats
    };
    const float *points;          // mode 2 and 3: n / streams x {p.xyz, n.xyz}
    uint32_t streams;             // mode 2 and 3: K
    float scale;                  // mode 2: pi / samples; mode 3: 4 pi / samples
    float *out;                   // unpack: n x 3 (mode 1), n / streams x 3 (mode 2) or n / streams x 27 (mode 3)
};
// One chunk through the persistent hw8 kernel with a path source: a slice of `samples` samples per slot of the strip frame over `state`.
struct ViewCamera;                // rt_types.h, which this header does not need
struct SourceChunk {
    uint32_t mode, n, streams;    // as in SourceView
    const float *rays, *points;
    int32_t ray_depth, samples;
    uint32_t *state;
    float *sh;                    // mode 3
    const uint32_t *pixels;       // mode 4: n x (x | y << 16) of the real frame (rt_adaptive.h)
    int32_t frame_w, frame_h;     // mode 4: the real frame, whose camera the slots' rays come from
    const ViewCamera *cameras;    // mode 5: `pixels` also holds n / 64 view indices, frame_w x frame_h is the views' frame (rt_views.h)
};
struct SourceResult { float kernel_ms; uint32_t launches, reference_exact; uint64_t exact_walks, no_path; };

// The engine states std::minstd_rand can be in: 1 .. 2^31 - 2.  Any other x is refused (host arrays) or marked invalid (device arrays)
// before a draw: 0 stays 0 for ever, and rng_n01's rejection loop would not end.
__host__ __device__ inline bool rq_rng_valid(uint32_t x) { return x - 1u < 2147483646u; }

// Launch geometry of the persistent walk (the round pipeline's traverse launch) as the host side sizes its overflow area by it.
#define RQ_BLOCKS_PER_CU 5u
size_t query_ovf_words(const rt_scene *scene);                        // 0 when neither tree needs the SPILL variant
// The launches of one chunk on `stream`; both return the number of launches.  The scene is only read.
uint32_t query_launch_closest(const rt_scene *scene, const QueryView &Q, hipStream_t stream);
uint32_t query_launch_light_pdf(const rt_scene *scene, const QueryView &Q, hipStream_t stream);
uint32_t query_launch_occluded(const rt_scene *scene, const QueryView &Q, hipStream_t stream);
uint32_t query_launch_material_table(const rt_scene *scene, uint32_t *table, hipStream_t stream); // fills n_triangles words
uint32_t query_launch_surface(const rt_scene *scene, const SurfaceView &V, hipStream_t stream);
uint32_t query_launch_environment(const rt_scene *scene, const EnvironmentView &V, hipStream_t stream);
uint32_t query_launch_camera_rays(const rt_scene *scene, const CameraView &V, hipStream_t stream);
uint32_t query_launch_guides(const rt_scene *scene, const GuidesView &V, hipStream_t stream);
uint32_t query_launch_scatter_sample(const rt_scene *scene, const ScatterView &V, hipStream_t stream);
uint32_t query_launch_scatter_finish(const rt_scene *scene, const ScatterView &V, hipStream_t stream);
uint32_t query_launch_bsdf_rays(const rt_scene *scene, const ScatterView &V, hipStream_t stream);
uint32_t query_launch_bsdf_finish(const rt_scene *scene, const ScatterView &V, hipStream_t stream);
uint32_t query_launch_path_advance(const rt_scene *scene, const PathView &V, hipStream_t stream);
uint32_t query_launch_bake_rays(const rt_scene *scene, const BakeView &B, hipStream_t stream);
uint32_t query_launch_bake_advance(const rt_scene *scene, const PathView &V, const BakeView &B, hipStream_t stream);
uint32_t query_launch_bake_resolve(const rt_scene *scene, const BakeView &B, hipStream_t stream);
uint32_t query_launch_source_pack(const rt_scene *scene, const SourceView &V, hipStream_t stream);
uint32_t query_launch_source_unpack(const rt_scene *scene, const SourceView &V, hipStream_t stream);
// rt_render_paths / rt_render_bake / rt_render_probes.  source_check: what stands in the way of a chunk of `slots` slots (host only; RT_OK, or the refusal
// with `who` in front).  source_render: the chunk's launches through the renders' own driver (check_frame, launch_frame, collect_frame
// of rtamd_api.hip), synchronous; the chunk's state is advanced in place.
int source_check(const rt_scene *scene, uint32_t slots, int32_t ray_depth, int32_t samples, const std::string &who);
int source_render(rt_scene *scene, const SourceChunk &C, hipStream_t stream, SourceResult &res, const std::string &who);

} // namespace rtamd

// Batched ray queries through the C-ABI (include/rtamd.h: rt_query_closest, rt_query_light_pdf): argument checks, the chunking, the
// staging and the statistics.  No kernel and no kernel header here: the kernels (device/rt_query.h) live in rtamd_api.hip, where every
// __global__ keeps one definition, and are launched through query_launch_* (device/rt_types_query.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "../../include/rtamd.h"
#include "host/knobs.h"
#include "host/rt_scene.h"
#include "device/rt_types_query.h"

using namespace rtamd;

namespace {

static_assert(sizeof(rt_ray) == 24 && sizeof(rt_hit) == 64, "rt_ray is 24 bytes and rt_hit 64: the kernels read and write them as words");

// Rays per chunk: what the staging is sized for.  RTAMD_QUERY_CHUNK (testing) lowers it, so that a small call crosses chunk seams; it
// changes no answer, a ray's answer does not depend on its neighbours.
const size_t QUERY_CHUNK = 262144;
size_t query_chunk() { return std::min(QUERY_CHUNK, (size_t)std::max(64, env_positive("RTAMD_QUERY_CHUNK", (int)QUERY_CHUNK))); }

// The staging of one chunk, carved out of one allocation that the scene keeps: counters first, then the arrays in 256-byte steps.
struct QueryStage {
    uint32_t *ctr; unsigned long long *totals;
    float *rays; uint8_t *out; float4 *rec; uint32_t *q_fast, *q_exact, *ovf;
};
QueryStage query_stage(rt_scene *scene) {
    const size_t C = QUERY_CHUNK, ovf_words = query_ovf_words(scene);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255u) & ~(size_t)255u; return here; };
    const size_t o_ctr = take(RQ_CTR_WORDS * 4), o_tot = take(RQ_TOTAL_WORDS * 8), o_rays = take(C * sizeof(rt_ray)), o_out = take(C * sizeof(rt_hit)),
                 o_rec = take(C * 16), o_fast = take(C * 4), o_exact = take(C * 4), o_ovf = take(ovf_words * 4);
    grow(scene->query_stage, scene->query_stage_bytes, at);
    uint8_t *b = scene->query_stage;
    QueryStage s;
    s.ctr = (uint32_t *)(b + o_ctr); s.totals = (unsigned long long *)(b + o_tot);
    s.rays = (float *)(b + o_rays); s.out = b + o_out; s.rec = (float4 *)(b + o_rec);
    s.q_fast = (uint32_t *)(b + o_fast); s.q_exact = (uint32_t *)(b + o_exact);
    s.ovf = ovf_words ? (uint32_t *)(b + o_ovf) : nullptr;
    return s;
}

// Both queries: `light` answers one float per ray, else one rt_hit.
int query(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, void *out, rt_query_stats *stats, bool light, const std::string &who) {
    if (stats && stats->struct_size != sizeof(rt_query_stats)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (flags & ~(RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK)) return fail(RT_ERR_INVALID_ARG, who + "flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK");
    if (scene->flavor != RT_INTEGRATOR_HW8) return fail(RT_ERR_UNSUPPORTED, who + "ray queries serve scenes created for hw8 / hw7 (this one was prepared for integrator " + std::to_string(scene->flavor) + ")");
    if (light && scene->view.n_lights == 0) return fail(RT_ERR_INVALID_ARG, who + "the scene has no lights: there is no light pdf to ask for");
    if (n && (!rays || !out)) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    const bool on_device = (flags & RT_QUERY_DEVICE_POINTERS) != 0;
    if (n && on_device && !light && ((uintptr_t)out & 15u)) return fail(RT_ERR_INVALID_ARG, who + "with RT_QUERY_DEVICE_POINTERS the rt_hit array must be 16-byte aligned");
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        rt_query_stats st{};
        st.struct_size = sizeof(rt_query_stats);
        st.reference_exact = scene->view.exact_boxes == 1u ? 1u : 0u;
        st.rays = n;
        if (n) {
            HIP_CHECK(hipSetDevice(scene->device));
            hipStream_t stream = nullptr;
            const QueryStage S = query_stage(scene);
            const size_t out_size = light ? sizeof(float) : sizeof(rt_hit), chunk = query_chunk();
            HIP_CHECK(hipMemsetAsync(S.totals, 0, RQ_TOTAL_WORDS * 8, stream));
            float ms_sum = 0.f;
            for (size_t first = 0; first < n; first += chunk) {
                const size_t m = std::min(chunk, n - first);
                uint8_t *out_here = (uint8_t *)out + first * out_size;
                QueryView Q{};
                Q.n = (uint32_t)m;
                Q.reference_walk = (flags & RT_QUERY_REFERENCE_WALK) ? 1u : 0u;
                Q.origin_bound = scene->view.box_c2 * 1048576.f; // box_c2 = 2^-20 max|coordinate| of scene and camera
                Q.rec = S.rec; Q.q_fast = S.q_fast; Q.q_exact = S.q_exact; Q.ctr = S.ctr; Q.totals = S.totals; Q.ovf = S.ovf;
                if (on_device) Q.rays = (const float *)(rays + first);
                else { HIP_CHECK(hipMemcpyAsync(S.rays, rays + first, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream)); Q.rays = S.rays; }
                uint8_t *dev_out = on_device ? out_here : S.out;
                if (light) Q.pdf = (float *)dev_out; else Q.hits = (uint4 *)dev_out;
                HIP_CHECK(hipMemsetAsync(S.ctr, 0, RQ_CTR_WORDS * 4, stream));
                HIP_CHECK(hipEventRecord(scene->ev_start, stream));
                st.launches += light ? query_launch_light_pdf(scene, Q, stream) : query_launch_closest(scene, Q, stream);
                HIP_CHECK(hipEventRecord(scene->ev_stop, stream));
                if (!on_device) HIP_CHECK(hipMemcpyAsync(out_here, S.out, m * out_size, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream)); // the next chunk reuses the staging
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop));
                ms_sum += ms;
            }
            unsigned long long totals[RQ_TOTAL_WORDS];
            HIP_CHECK(hipMemcpy(totals, S.totals, sizeof totals, hipMemcpyDeviceToHost));
            st.exact_walks = totals[RQ_TOTAL_EXACT]; st.invalid_rays = totals[RQ_TOTAL_INVALID];
            st.kernel_ms = ms_sum;
        }
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
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

} // extern "C"

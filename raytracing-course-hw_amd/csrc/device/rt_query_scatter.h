// The bounce step through the C-ABI (include/rtamd.h: rt_query_scatter, rt_query_bsdf, rt_trace_paths): what Scene::getColor decides at
// a hit (hw8/src/scene.cpp:151-164) for records of the caller's own.  One iteration of trace_path (rt_kernels_hw8.h) taken apart at its
// light walk, with the same device functions in the same order; no kernel here walks a tree, the light pdf comes from rt_query.h's
// launches over the rays the sample kernel leaves behind.
//
//   rq_scatter_sample_kernel  one lane per record: classify, the component draw, cosine_sample / vndf_sample / light_sample, material_brdf,
//                             the brdf < eps return; writes o, d, brdf, component, the engine, and the ray of the light walk
//   rq_scatter_finish_kernel  one lane per record that goes on: cosine_pdf + vndf_pdf (+ the walk's answer), / components, k in double,
//                             k * brdf, the clamp return
//   rq_bsdf_rays_kernel       rt_query_bsdf: classify and the ray of the light walk for a direction of the caller's
//   rq_bsdf_finish_kernel     rt_query_bsdf: material_brdf and the finish kernel's pdf for that direction
//   rq_path_advance_kernel    rt_trace_paths: after a bounce's queries (rq_path_end_or_keep, which rt_bake.h shares), end a path (miss: rq_environment; END_*: the emission) or keep
//                             e[b], m[b] and make (o, d) its ray; after the last bounce fold L = e[b] + m[b] * L backwards
//
// A record is classified before any dependent work, as rq_surface_kernel does: no surface (hit.triangle or surface.material 0xFFFFFFFF)
// answers zeros and is not counted; an invalid ray (rq_valid_ray), a non-finite t or ng, or an engine state outside 1 .. 2^31-2
// (rq_rng_valid: rng_n01's loop would never end on it) answers zeros and is counted; neither touches the engine.  Nothing is indexed
// by a word of a caller's record: the scene is read at the light the engine picks (k < n_lights by construction) and in the light tree.
// Records are read and written as 16-byte words; floats leave through rq_bits, like every record of the queries.
#pragma once
#include "rt_query_surface.h"

namespace rtamd {
namespace dev {

// rt_scatter::flags (include/rtamd.h)
#define RQ_SCATTER_END_BRDF 1u
#define RQ_SCATTER_END_CLAMP 2u
#define RQ_SCATTER_NO_SURFACE 4u
#define RQ_SCATTER_INVALID 8u
#define RQ_PATH_ENDED 0x80000000u

#define RQ_EPS 9.99999974737875163555e-05f // (float)1e-4L, as trace_path spells it

RT_DEV F3 rq_f3(uint32_t x, uint32_t y, uint32_t z) { return f3(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z)); }
RT_DEV void rq_store_ray(float *p, F3 o, F3 d) { p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = d.x; p[4] = d.y; p[5] = d.z; }
RT_DEV void rq_store_no_ray(float *p) { // an invalid ray: never walked, answered 0
    const float nan = __uint_as_float(0x7FC00000u);
    p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = nan; p[4] = nan; p[5] = nan;
}

// What the kernels need of a record's ray, hit and surface; `kind`: 0 = it goes on, else RQ_SCATTER_NO_SURFACE or RQ_SCATTER_INVALID.
struct ScatterIn {
    F3 o, d, ng, xo, color, sn, base_color;
    float alpha, metallic, base_metallic;
    uint32_t kind;
};
RT_DEV ScatterIn rq_scatter_load(const ScatterView &V, uint32_t i) {
    ScatterIn R;
    const uint4 *hp = V.hits + 4 * (size_t)i, *sp = V.surfaces + 4 * (size_t)i;
    const uint4 h0 = hp[0], h1 = hp[1];                     // t triangle ng.xy | ng.z ...
    const uint4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
    const float *p = V.rays + 6 * (size_t)i;
    R.o = f3(p[0], p[1], p[2]); R.d = f3(p[3], p[4], p[5]);
    R.ng = rq_f3(h0.z, h0.w, h1.x);
    R.color = rq_f3(s0.x, s0.y, s0.z); R.alpha = __uint_as_float(s0.w);
    R.metallic = __uint_as_float(s1.w);                      // the emission belongs to the caller's fold, not to the bounce
    R.sn = rq_f3(s2.x, s2.y, s2.z);
    R.base_color = rq_f3(s3.x, s3.y, s3.z); R.base_metallic = __uint_as_float(s3.w);
    const float t = __uint_as_float(h0.x);
    if (h0.y == RQ_NO_TRIANGLE || s2.w == RQ_NO_TRIANGLE) R.kind = RQ_SCATTER_NO_SURFACE;
    else if (!rq_valid_ray(R.o, R.d) || !(rq_finite_word(h0.x) && rq_finite_word(h0.z) && rq_finite_word(h0.w) && rq_finite_word(h1.x))) R.kind = RQ_SCATTER_INVALID;
    else R.kind = 0u;
    const F3 x = R.o + t * R.d;                              // scene.cpp:104
    R.xo = x + RQ_EPS * R.ng;                                // x + eps * geomNorma
    return R;
}
RT_DEV void rq_write_scatter_blank(uint4 *out, uint32_t flags) {
    out[0] = make_uint4(0u, 0u, 0u, 0u); out[1] = make_uint4(0u, 0u, 0u, flags);
    out[2] = make_uint4(0u, 0u, 0u, 0u); out[3] = make_uint4(0u, 0u, 0u, 0u);
}

// Mix::pdf (distributions.h:267-279) of nd, the light term given as the walk answered it (already divided by the light count).
RT_DEV float rq_mix_pdf(const SceneView &S, const ScatterIn &R, F3 nd, const float *light_pdf, uint32_t i) {
    float pdf = 0.f;
    pdf += cosine_pdf(R.sn, nd);
    pdf += vndf_pdf(R.sn, nd, R.d, R.alpha);
    if (S.n_components == 3) pdf += light_pdf[i];
    return pdf / S.n_components_f;
}
RT_DEV F3 rq_brdf(const ScatterIn &R, F3 nd) {               // scene.cpp:153
    return material_brdf(R.base_color, R.base_metallic, nd, neg(R.d), R.sn, R.color, R.metallic, R.alpha);
}

__global__ __launch_bounds__(256) void rq_scatter_sample_kernel(SceneView S, ScatterView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const ScatterIn R = rq_scatter_load(V, i);
        const uint4 e = V.rng[i];                            // x saved has_saved reserved
        uint4 *out = V.out + 4 * (size_t)i;
        float *walk = V.walk_rays + 6 * (size_t)i;
        const uint32_t kind = R.kind ? R.kind : rq_rng_valid(e.x) ? 0u : RQ_SCATTER_INVALID;
        if (kind) {
            if (kind == RQ_SCATTER_INVALID) atomicAdd(V.totals + RQ_TOTAL_INVALID, 1ull);
            rq_write_scatter_blank(out, kind);
            rq_store_no_ray(walk);
            continue;
        }
        Rng rng; rng.x = e.x; rng.saved = __uint_as_float(e.y); rng.has_saved = e.z != 0u;
        // Mix::sample (distributions.h:256-265)
        const int comp = (int)(rng_u01(rng) * S.n_components_f);
        F3 nd;
        if (comp == 0) nd = cosine_sample(rng, R.sn);
        else if (comp == 2) nd = light_sample(S, rng, R.xo);
        else nd = vndf_sample(rng, R.sn, R.d, R.alpha);
        V.rng[i] = make_uint4(rng.x, rng.has_saved ? __float_as_uint(rng.saved) : 0u, rng.has_saved ? 1u : 0u, e.w);
        const F3 brdf = rq_brdf(R, nd);
        // brdf < eps with eps = 1e-4L: for a float this is  brdf <= (float)1e-4  (no float lies in between)
        const bool ends = brdf.x <= RQ_EPS && brdf.y <= RQ_EPS && brdf.z <= RQ_EPS;                           // :154-156
        out[0] = make_uint4(rq_bits(R.xo.x), rq_bits(R.xo.y), rq_bits(R.xo.z), 0u);
        out[1] = make_uint4(rq_bits(nd.x), rq_bits(nd.y), rq_bits(nd.z), ends ? RQ_SCATTER_END_BRDF : 0u);
        out[2] = make_uint4(0u, 0u, 0u, (uint32_t)comp);
        out[3] = make_uint4(rq_bits(brdf.x), rq_bits(brdf.y), rq_bits(brdf.z), 0u);
        if (ends || S.n_components != 3) rq_store_no_ray(walk); else rq_store_ray(walk, R.xo, nd);
    }
}

__global__ __launch_bounds__(256) void rq_scatter_finish_kernel(SceneView S, ScatterView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        uint4 *out = V.out + 4 * (size_t)i;
        const uint4 o1 = out[1];
        if (o1.w) continue;                                  // ended in the sample kernel, or blank
        const uint4 o0 = out[0], o2 = out[2], o3 = out[3];
        const ScatterIn R = rq_scatter_load(V, i);
        const F3 nd = rq_f3(o1.x, o1.y, o1.z), brdf = rq_f3(o3.x, o3.y, o3.z);
        const float pdf = rq_mix_pdf(S, R, nd, V.light_pdf, i);
        const float k = (float)(1. / (double)pdf * fabs((double)dot(nd, R.sn)));                              // :159
        const F3 mult = k * brdf;
        const bool ends = mult.x > 6.f || mult.y > 6.f || mult.z > 6.f || mult.x != mult.x || mult.y != mult.y || mult.z != mult.z; // :161-163
        out[0] = make_uint4(o0.x, o0.y, o0.z, rq_bits(pdf));
        if (ends) out[1] = make_uint4(o1.x, o1.y, o1.z, RQ_SCATTER_END_CLAMP);
        else out[2] = make_uint4(__float_as_uint(mult.x), __float_as_uint(mult.y), __float_as_uint(mult.z), o2.w);
    }
}

// rt_query_bsdf.  A direction with a NaN, an infinity, or all zeros makes its record invalid, like such a ray.
RT_DEV uint32_t rq_bsdf_kind(const ScatterIn &R, F3 nd) { return R.kind ? R.kind : rq_valid_ray(R.xo, nd) ? 0u : RQ_SCATTER_INVALID; }

__global__ __launch_bounds__(256) void rq_bsdf_rays_kernel(SceneView S, ScatterView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const ScatterIn R = rq_scatter_load(V, i);
        const float *q = V.dirs + 3 * (size_t)i;
        const F3 nd = f3(q[0], q[1], q[2]);
        float *walk = V.walk_rays + 6 * (size_t)i;
        if (rq_bsdf_kind(R, nd)) rq_store_no_ray(walk); else rq_store_ray(walk, R.xo, nd);
    }
}

__global__ __launch_bounds__(256) void rq_bsdf_finish_kernel(SceneView S, ScatterView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const ScatterIn R = rq_scatter_load(V, i);
        const float *q = V.dirs + 3 * (size_t)i;
        const F3 nd = f3(q[0], q[1], q[2]);
        const uint32_t kind = rq_bsdf_kind(R, nd);
        if (kind == RQ_SCATTER_INVALID) atomicAdd(V.totals + RQ_TOTAL_INVALID, 1ull);
        uint32_t *ob = reinterpret_cast<uint32_t *>(V.out_brdf) + 3 * (size_t)i, *op = reinterpret_cast<uint32_t *>(V.out_pdf) + i;
        if (kind) { ob[0] = 0u; ob[1] = 0u; ob[2] = 0u; *op = 0u; continue; }
        const F3 brdf = rq_brdf(R, nd);
        const float pdf = rq_mix_pdf(S, R, nd, V.light_pdf, i);
        ob[0] = rq_bits(brdf.x); ob[1] = rq_bits(brdf.y); ob[2] = rq_bits(brdf.z); *op = rq_bits(pdf);
    }
}

// ---- rt_trace_paths ------------------------------------------------------------------------------------------------------------------------
// A chunk's state starts as zeros (the host clears it): tail 0, no bounce kept, not ended.
// The end-or-keep step of a live path after a bounce's queries, shared with the baker (rt_bake.h): end it (miss: rq_environment; END_*:
// the emission) with `tail`, RQ_PATH_ENDED in `word` and an invalid ray, or keep e[b], m[b], count the bounce in `word` and make (o, d) its ray.
RT_DEV bool rq_path_end_or_keep(const SceneView &S, const PathView &V, uint32_t i, float *ray, uint32_t &word, F3 &tail) {
    const uint32_t tri = V.hits[4 * (size_t)i].y;
    tail = f3(0.f, 0.f, 0.f);
    bool ended = true;
    if (tri == RQ_NO_TRIANGLE) {                             // scene.cpp:90-97; an invalid ray sees 0, 0, 0
        bool valid;
        tail = rq_environment(S, f3(ray[0], ray[1], ray[2]), f3(ray[3], ray[4], ray[5]), valid);
    } else {
        const uint4 *sc = V.scatter + 4 * (size_t)i;
        const uint4 c0 = sc[0], c1 = sc[1], c2 = sc[2];
        const uint4 s1 = V.surfaces[4 * (size_t)i + 1];
        const F3 emission = rq_f3(s1.x, s1.y, s1.z);
        if (c1.w) tail = (c1.w & RQ_SCATTER_NO_SURFACE) ? tail : emission;                                    // :154-156, :161-163
        else {
            float *e = V.stack + 6 * ((size_t)(word & 0xFFu) * V.n + i);
            e[0] = emission.x; e[1] = emission.y; e[2] = emission.z;
            e[3] = __uint_as_float(c2.x); e[4] = __uint_as_float(c2.y); e[5] = __uint_as_float(c2.z);
            word++;
            rq_store_ray(ray, rq_f3(c0.x, c0.y, c0.z), rq_f3(c1.x, c1.y, c1.z));
            ended = false;
        }
    }
    if (ended) { word |= RQ_PATH_ENDED; rq_store_no_ray(ray); }
    return ended;
}
// L = e[b] + m[b] * L backwards from the tail over the bounces kept.
RT_DEV F3 rq_path_fold(const PathView &V, uint32_t i, uint32_t word, F3 tail) {
    F3 L = tail;                                             // recLimit == 0 -> 0: a path that never ended keeps the tail 0
    for (int b = (int)(word & 0xFFu) - 1; b >= 0; b--) {
        const float *e = V.stack + 6 * ((size_t)b * V.n + i);
        L = f3(e[0], e[1], e[2]) + f3(e[3], e[4], e[5]) * L;                                                  // :164
    }
    return L;
}

__global__ __launch_bounds__(256) void rq_path_advance_kernel(SceneView S, PathView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        float4 st = V.state[i];
        uint32_t word = __float_as_uint(st.w);
        if (!(word & RQ_PATH_ENDED)) {
            F3 tail;
            rq_path_end_or_keep(S, V, i, V.rays + 6 * (size_t)i, word, tail);
            st = make_float4(tail.x, tail.y, tail.z, __uint_as_float(word));
            if (!V.last) V.state[i] = st;
        }
        if (V.last) {
            const F3 L = rq_path_fold(V, i, word, f3(st.x, st.y, st.z));
            float *out = V.rgb + 3 * (size_t)i;
            out[0] = L.x; out[1] = L.y; out[2] = L.z;
        }
    }
}

} // namespace dev
} // namespace rtamd

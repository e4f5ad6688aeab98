// Test-only entry points (NOT part of include/rtamd.h, built into librtamd_testhooks.so): run individual
// device functions of rt_device.h on the GPU so tests can compare them with the host libm / libstdc++, and the on-device tree builder
// on boxes of the test's own so its tree can be read back.
#include <hip/hip_runtime.h>
#include "../../include/rtamd.h"
#include "device/rt_device.h"
#include "device/rt_exact.h"
#define RT_DEVICE_FUNCTIONS_ONLY // the hooks call the device functions of the .txt kernels; the kernels themselves stay the library's alone
#include "device/rt_kernels_hw5.h"
#include "device/rt_kernels_hw8.h"
#include "device/rt_node_grid.h"
#include "device/rt_pt_queue.h"
#include "device/rt_ref_walk.h"
#include "host/device_build.h"
#include "host/fold_nodes.h"
#include "host/hip_check.h"
#include "host/rt_adaptive_decide.h"
#include "host/rt_view_adaptive_plan.h"
#include "host/rt_views_camera.h"
#include "host/rt_guard.h"
#include "host/rt_scene.h"
#include "host/scene_prep.h"
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace rtamd::dev;

__global__ void k_logf(const float *in, float *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = rt_logf(in[i]);
}
__global__ void k_asinf(const float *in, float *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = rt_asinf(in[i]);
}
__global__ void k_atan2f(const float *y, const float *x, float *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = rt_atan2f(y[i], x[i]);
}
__global__ void k_env_uv(const float *d, float *uv, size_t n) { // d: n x 3 directions, uv: n x 2
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) env_uv(f3(d + 3 * i), uv[2 * i], uv[2 * i + 1]);
}
__global__ void k_rng(uint32_t seed0, int n_seeds, int n_u, int n_n, float *out) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seeds) return;
    Rng r;
    rng_seed(r, seed0 + (uint32_t)s);
    float *o = out + (size_t)s * (n_u + n_n);
    for (int i = 0; i < n_u; i++) o[i] = rng_u01(r);
    for (int i = 0; i < n_n; i++) o[n_u + i] = rng_n01(r);
}
// rng_n01x3 against three rng_n01 calls, after `prior` (0 or 1) rng_n01 calls on the stream of seed0 + s.  Per seed and side (0: three
// rng_n01, 1: rng_n01x3) eight words: the three values' bits, x, the bits of saved, has_saved, has_saved on entry, engine steps of the triple.
RT_DEV uint32_t hook_rng_steps(uint32_t from, uint32_t to) { // steps of the engine from state `from` to state `to` (a triple makes a few)
    Rng g; g.x = from; g.saved = 0.f; g.has_saved = false;
    uint32_t n = 0;
    while (g.x != to && n < 4096u) { (void)rng_u01(g); n++; }
    return n;
}
__global__ void k_rng_triple(uint32_t seed0, int n_seeds, int prior, uint32_t *out) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seeds) return;
    for (int side = 0; side < 2; side++) {
        Rng r;
        rng_seed(r, seed0 + (uint32_t)s);
        for (int i = 0; i < prior; i++) (void)rng_n01(r);
        const uint32_t entered = r.has_saved ? 1u : 0u, x0 = r.x;
        float a, b, c;
        if (side == 0) { a = rng_n01(r); b = rng_n01(r); c = rng_n01(r); }
        else rng_n01x3(r, a, b, c);
        uint32_t *o = out + ((size_t)s * 2 + side) * 8;
        o[0] = __float_as_uint(a); o[1] = __float_as_uint(b); o[2] = __float_as_uint(c);
        o[3] = r.x; o[4] = __float_as_uint(r.saved); o[5] = r.has_saved ? 1u : 0u; o[6] = entered; o[7] = hook_rng_steps(x0, r.x);
    }
}

// The shading layer of rt_device.h, one lane per case (tests/shading_cases.py has the cases and the row layouts).
// in: 18 floats (base_metallic, base_color 3, l 3, v 3, n 3, color 3, metallic, alpha), out: 3.  variant 0: material_brdf; 1: material_brdf_pre on
// the two products the shader forms (rt_persistent.h, shade_fetch_attr's results); 2: material_brdf_hw7 with alpha2 = alpha * alpha as there
__global__ void k_brdf(int variant, const float *in, float *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 18 * i;
    const float base_metallic = p[0], metallic = p[16], alpha = p[17];
    const F3 base_color = f3(p + 1), l = f3(p + 4), v = f3(p + 7), nn = f3(p + 10), color = f3(p + 13);
    F3 r;
    if (variant == 0) r = material_brdf(base_color, base_metallic, l, v, nn, color, metallic, alpha);
    else if (variant == 1) r = material_brdf_pre(base_color * color, metallic * base_metallic, l, v, nn, alpha);
    else r = material_brdf_hw7(base_color, base_metallic, l, v, nn, alpha * alpha);
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
// in: 7 floats (n 3, v 3, alpha), out: 5 (d 3, pdf of d, the next rng_u01), state: the engine after the sample.  form 0: the plain pair;
// 1: the frame-given pair on a frame built as the persistent shader builds it
__global__ void k_vndf(int form, const uint32_t *seed, const float *in, float *out, uint32_t *state, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 7 * i;
    const F3 nn = f3(p), v = f3(p + 3);
    const float alpha = p[6];
    Rng rng;
    rng_seed(rng, seed[i]);
    F3 d; float pdf;
    if (form == 0) { d = vndf_sample(rng, nn, v, alpha); pdf = vndf_pdf(nn, d, v, alpha); }
    else {
        const Quat q = vndf_getq(nn);
        const F3 vT = qtransform(q, neg(v));
        d = vndf_sample(rng, q, vT, alpha);
        pdf = vndf_pdf(q, vT, d, alpha);
    }
    state[i] = rng.x;
    out[5 * i] = d.x; out[5 * i + 1] = d.y; out[5 * i + 2] = d.z; out[5 * i + 3] = pdf; out[5 * i + 4] = rng_u01(rng);
}
__global__ void k_vndf_local(const float *in, float *out, size_t n) { // in: t1, t2, vT 3, alpha
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 6 * i;
    const F3 r = vndf_sample_local(p[0], p[1], f3(p + 2), p[5]);
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
__global__ void k_vndf_pdf(const float *in, float *out, size_t n) { // in: n 3, d 3, v 3, alpha
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 10 * i;
    out[i] = vndf_pdf(f3(p), f3(p + 3), f3(p + 6), p[9]);
}
__global__ void k_cosine(const uint32_t *seed, const float *in, float *out, uint32_t *state, size_t n) { // in: n 3; out as k_vndf
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 nn = f3(in + 3 * i);
    Rng rng;
    rng_seed(rng, seed[i]);
    const F3 d = cosine_sample(rng, nn);
    state[i] = rng.x;
    out[5 * i] = d.x; out[5 * i + 1] = d.y; out[5 * i + 2] = d.z; out[5 * i + 3] = cosine_pdf(nn, d); out[5 * i + 4] = rng_u01(rng);
}
__global__ void k_cosine_pdf(const float *in, float *out, size_t n) { // in: n 3, d 3
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = cosine_pdf(f3(in + 6 * i), f3(in + 6 * i + 3));
}
__global__ void k_tonemap(const float *in, uint8_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = tonemap1(in[i]);
}
// The texture layer (rt_device.h sample_texture / load_texel / apply_normal_map), one lane per case.  k_sample_texture taps the images of a
// scene made through the public API, so the texel array, the descriptors and the sRGB table are scene preparation's: slot = an image slot,
// -1 = the environment map; form 0 = the overload that loads the descriptor by slot, 1 = the one that is handed the descriptor.
__global__ void k_sample_texture(rtamd::SceneView S, int form, const int32_t *slot, const float *uv, const int32_t *srgb, float *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i] < 0 ? S.env_image : slot[i];
    const F3 r = form == 0 ? sample_texture(S, s, uv[2 * i], uv[2 * i + 1], srgb[i] != 0)
                           : sample_texture(S, S.images[s], uv[2 * i], uv[2 * i + 1], srgb[i] != 0);
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
__global__ void k_apply_normal_map(const float *in, float *out, size_t n) { // in: sn 3, tangent 3, tanw, sample 3
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 10 * i;
    const F3 r = apply_normal_map(f3(p), f3(p + 3), p[6], f3(p + 7));
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
// vndf_disk_point on the stream of seed0 + i: u = the two uniforms the call consumed (from a copy of the engine), t = (t1, t2), cs = the
// device libm's cos and sin of the angle in double, which the call narrows (for the census of the test)
__global__ void k_disk_point(uint32_t seed0, float *u, float *t, double *cs, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng_seed(rng, seed0 + (uint32_t)i);
    Rng copy = rng;
    const float u1 = rng_u01(copy), u2 = rng_u01(copy);
    float t1, t2;
    vndf_disk_point(rng, t1, t2);
    const float phi = (float)(2.0 * RT_PI * (double)u2);
    u[2 * i] = u1; u[2 * i + 1] = u2;
    t[2 * i] = t1; t[2 * i + 1] = t2;
    cs[2 * i] = cos((double)phi); cs[2 * i + 1] = sin((double)phi);
}

// rt_exact.h: the runner-up's distance as it travels in the hit word, and the gate's decision on a box / ray / hit / gap
__global__ void k_gap(const float *t, const float *t2, float *floor_out, uint32_t *code_out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = pt_gap_code(t[i], t2[i]);
    code_out[i] = c;
    floor_out[i] = pt_gap_floor(c | 5u, t[i]);   // some figure index in the low bits: it must not disturb the code
}
__global__ void k_stands(const float *in, uint32_t *out, size_t n) { // per case 16 floats: lo.xyz hi.xyz o.xyz d.xyz t gap c2 cull_k
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 16 * i;
    out[i] = pt_hit_stands(f3(p[0], p[1], p[2]), f3(p[3], p[4], p[5]), f3(p[6], p[7], p[8]), f3(p[9], p[10], p[11]), p[12], p[13], p[14], 1.25f * p[14], p[15]) ? 1u : 0u;
}

// The intersection layer, one lane per case (tests/intersection_cases.py has the cases and the row layouts).
// rt_ref_walk.h ref_box_test.  in: 12 floats (mn, mx, o, d); out: 2 words (1 accepted | 2 inside, the bits of t; 0 for a rejected box)
__global__ void k_ref_box(const float *in, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 12 * i;
    float t = 0.f; bool inside = false;
    const bool ok = ref_box_test(f3(p), f3(p + 3), f3(p + 6), f3(p + 9), t, inside);
    out[2 * i] = ok ? (1u | (inside ? 2u : 0u)) : 0u;
    out[2 * i + 1] = ok ? __float_as_uint(t) : 0u;
}
// rt_device.h tri_test and tri_test_closer on the host's record of the triangle.  rays: 6 floats (o, d); out: 8 words, for each of the
// two tests (1 hit | 2 inside) and the bits of t, u, v (0 for a miss)
__global__ void k_tri(const rtamd::TriIsect *isect, const float *rays, const float *keep_t, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rtamd::TriIsect T = load_isect(isect + i);
    const F3 o = f3(rays + 6 * i), d = f3(rays + 6 * i + 3);
    for (int side = 0; side < 2; side++) {
        float t = 0.f, u = 0.f, v = 0.f; bool inside = false;
        const bool hit = side == 0 ? tri_test(T, o, d, t, u, v, inside) : tri_test_closer(T, o, d, keep_t[i], t, u, v, inside);
        uint32_t *q = out + 8 * i + 4 * side;
        q[0] = hit ? (1u | (inside ? 2u : 0u)) : 0u;
        q[1] = hit ? __float_as_uint(t) : 0u; q[2] = hit ? __float_as_uint(u) : 0u; q[3] = hit ? __float_as_uint(v) : 0u;
    }
}
// rt_exact.h pt_box_robust with and without its pretest (bits 1 and 2) and rq_any_hit_stands (bit 4, with tmax in the gap's place), on
// k_stands's 16 floats
__global__ void k_robust(const float *in, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 16 * i;
    const F3 lo = f3(p), hi = f3(p + 3), o = f3(p + 6), d = f3(p + 9);
    const F3 P = o + p[12] * d;
    out[i] = (pt_box_robust<true>(lo, hi, P, d, p[12], p[14]) ? 1u : 0u) | (pt_box_robust<false>(lo, hi, P, d, p[12], p[14]) ? 2u : 0u) |
             (rq_any_hit_stands(lo, hi, o, d, p[12], p[13], p[14]) ? 4u : 0u);
}
// rt_device.h slab_test on boxes the host has padded.  boxes: 6 floats (lo, hi), rays: 12 floats, of which o and d are read
__global__ void k_slab_padded(const float *boxes, const float *in, float tbest, uint32_t *flag, float *tnear, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *b = boxes + 6 * i, *p = in + 12 * i;
    float tn = 0.f;
    flag[i] = slab_test(make_float4(b[0], b[1], b[2], 0.f), make_float4(b[3], b[4], b[5], 0.f), make_ray_inv(f3(p + 6), f3(p + 9)), tbest, tn) ? 1u : 0u;
    tnear[i] = tn;
}

// The analytic layer of the .txt snapshots, one lane per case (tests/analytic_cases.py has the cases and the row layouts).  A hit is 5 words:
// 1 hit | 2 inside, the bits of t and of the normal; all 0 for a miss.
__device__ inline void put_hit(bool ok, bool inside, float t, F3 n, uint32_t *o) {
    o[0] = ok ? (1u | (inside ? 2u : 0u)) : 0u;
    o[1] = ok ? __float_as_uint(t) : 0u; o[2] = ok ? __float_as_uint(n.x) : 0u; o[3] = ok ? __float_as_uint(n.y) : 0u; o[4] = ok ? __float_as_uint(n.z) : 0u;
}
// rt_kernels_txt.h smallest_root<true> (hw1 / hw2) and <false> (hw3+).  in: a, b, c; out: 2 words each (flags, t)
__global__ void k_quad(const float *in, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 3 * i;
    float t = 0.f; bool inside = false;
    bool ok = smallest_root<true>(p[0], p[1], p[2], t, inside);
    out[4 * i] = ok ? (1u | (inside ? 2u : 0u)) : 0u; out[4 * i + 1] = ok ? __float_as_uint(t) : 0u;
    t = 0.f; inside = false;
    ok = smallest_root<false>(p[0], p[1], p[2], t, inside);
    out[4 * i + 2] = ok ? (1u | (inside ? 2u : 0u)) : 0u; out[4 * i + 3] = ok ? __float_as_uint(t) : 0u;
}
// box_slabs.  in: s, o, d; out: 2 words (flags, t)
__global__ void k_slabs(const float *in, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 9 * i;
    float t = 0.f; bool inside = false;
    const bool ok = box_slabs(f3(p), f3(p + 3), f3(p + 6), t, inside);
    out[2 * i] = ok ? (1u | (inside ? 2u : 0u)) : 0u; out[2 * i + 1] = ok ? __float_as_uint(t) : 0u;
}
// The figure test of each snapshot on the host's own records: prim_hit1 (hw1; no side, no normal), prim_hit<true> (hw2), prim_hit<false> (hw3),
// prim_hit<false, true> (hw4) on the GpuPrim, fig_hit5 (hw5) on the GpuFig5.  rays: o, d; out: 5 hits
__global__ void k_fig(const rtamd::GpuPrim *prims, const rtamd::GpuFig5 *figs, const float *rays, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PrimRegs P = load_prim(prims + i);
    const FigRegs F = load_fig5(figs + i);
    const F3 o = f3(rays + 6 * i), d = f3(rays + 6 * i + 3), zero = f3(0.f, 0.f, 0.f);
    uint32_t *q = out + 25 * i;
    float t = 0.f; F3 nn = zero; bool inside = false;
    bool ok = prim_hit1(P, o, d, t);
    put_hit(ok, false, t, zero, q);
    t = 0.f; nn = zero; inside = false;
    ok = prim_hit<true>(P, o, d, t, nn, inside); put_hit(ok, inside, t, nn, q + 5);
    t = 0.f; nn = zero; inside = false;
    ok = prim_hit<false>(P, o, d, t, nn, inside); put_hit(ok, inside, t, nn, q + 10);
    t = 0.f; nn = zero; inside = false;
    ok = prim_hit<false, true>(P, o, d, t, nn, inside); put_hit(ok, inside, t, nn, q + 15);
    t = 0.f; nn = zero; inside = false;
    ok = fig_hit5(F, o, d, t, nn, inside); put_hit(ok, inside, t, nn, q + 20);
}
// light_pdf4 (box and ellipsoid figures) and light_pdf_one5.  rays: x, d; out: 2 words
__global__ void k_lpdf(const rtamd::GpuPrim *prims, const rtamd::GpuFig5 *figs, const float *rays, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PrimRegs P = load_prim(prims + i);
    const FigRegs F = load_fig5(figs + i);
    const F3 x = f3(rays + 6 * i), d = f3(rays + 6 * i + 3);
    out[2 * i] = P.type == RT_PRIM_TRIANGLE ? 0u : __float_as_uint(light_pdf4(P, x, d));
    out[2 * i + 1] = __float_as_uint(light_pdf_one5(F, x, d));
}
// pdf_one4 (box and ellipsoid figures) and pdf_one5 on a y and yn of the case's own.  pts: x, d, y, yn; out: 2 words
__global__ void k_pdf_one(const rtamd::GpuPrim *prims, const rtamd::GpuFig5 *figs, const float *pts, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PrimRegs P = load_prim(prims + i);
    const FigRegs F = load_fig5(figs + i);
    const float *p = pts + 12 * i;
    const F3 x = f3(p), d = f3(p + 3), y = f3(p + 6), yn = f3(p + 9);
    out[2 * i] = P.type == RT_PRIM_TRIANGLE ? 0u : __float_as_uint(pdf_one4(P, x, d, y, yn));
    out[2 * i + 1] = __float_as_uint(pdf_one5(F, x, d, y, yn));
}
// box_face_point.  in: the half-sizes; out: 4 words (the point in the box's frame, engine state after); the normal cache must stay as it was
__global__ void k_face_point(const float *in, const uint32_t *seeds, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng_seed(rng, seeds[i]);
    const F3 p = box_face_point(rng, f3(in + 3 * i));
    out[4 * i] = __float_as_uint(p.x); out[4 * i + 1] = __float_as_uint(p.y); out[4 * i + 2] = __float_as_uint(p.z); out[4 * i + 3] = rng.x;
}
#define HOOK_SENTINEL 12345.f
// light_sample4 as light number i % 32 of a pixel whose other normal caches (Cosine's and the other lights') all hold a sentinel, and
// light_sample5 with the pixel's one cache.  aux: seed, whether the cache holds a value, its bits.  out: 13 words: hw4 direction 3, engine
// state, the light's cache 2, 1 when every other cache still holds the sentinel; hw5 direction 3, engine state, cache 2
__global__ void k_lsample(const rtamd::GpuPrim *prims, const rtamd::GpuFig5 *figs, const float *xs, const uint32_t *aux, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PrimRegs P = load_prim(prims + i);
    const FigRegs F = load_fig5(figs + i);
    const F3 x = f3(xs + 3 * i);
    const uint32_t seed = aux[3 * i], has = aux[3 * i + 1];
    const float saved = __uint_as_float(aux[3 * i + 2]);
    uint32_t *q = out + 13 * i;
    for (int k = 0; k < 13; k++) q[k] = 0u;
    Rng rng;
    if (P.type != RT_PRIM_TRIANGLE) {
        const int li = (int)(i % RT4_MAX_LIGHTS);
        LightNormals N;
        for (int k = 0; k < RT4_MAX_LIGHTS; k++) N.saved[k] = HOOK_SENTINEL;
        N.has = 0xffffffffu;
        N.saved[li] = saved;
        if (!has) N.has &= ~(1u << li);
        rng_seed(rng, seed);
        rng.saved = HOOK_SENTINEL; rng.has_saved = true;
        const F3 d = light_sample4(P, rng, N, li, x);
        q[0] = __float_as_uint(d.x); q[1] = __float_as_uint(d.y); q[2] = __float_as_uint(d.z); q[3] = rng.x;
        q[4] = (N.has >> li) & 1u; q[5] = q[4] ? __float_as_uint(N.saved[li]) : 0u;
        bool intact = rng.has_saved && rng.saved == HOOK_SENTINEL;
        for (int k = 0; k < RT4_MAX_LIGHTS; k++) if (k != li) intact = intact && ((N.has >> k) & 1u) && N.saved[k] == HOOK_SENTINEL;
        q[6] = intact ? 1u : 0u;
    }
    rng_seed(rng, seed);
    rng.saved = saved; rng.has_saved = has != 0u;
    const F3 d = light_sample5(F, rng, x);
    q[7] = __float_as_uint(d.x); q[8] = __float_as_uint(d.y); q[9] = __float_as_uint(d.z); q[10] = rng.x;
    q[11] = rng.has_saved ? 1u : 0u; q[12] = rng.has_saved ? __float_as_uint(rng.saved) : 0u;
}
// cosine_sample_txt.  in: the normal; aux as k_lsample; out: 6 words (direction 3, engine state, cache 2)
__global__ void k_cosine_txt(const float *in, const uint32_t *aux, uint32_t *out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng_seed(rng, aux[3 * i]);
    rng.saved = __uint_as_float(aux[3 * i + 2]); rng.has_saved = aux[3 * i + 1] != 0u;
    const F3 d = cosine_sample_txt(rng, f3(in + 3 * i));
    uint32_t *q = out + 6 * i;
    q[0] = __float_as_uint(d.x); q[1] = __float_as_uint(d.y); q[2] = __float_as_uint(d.z); q[3] = rng.x;
    q[4] = rng.has_saved ? 1u : 0u; q[5] = rng.has_saved ? __float_as_uint(rng.saved) : 0u;
}

// rt_device.h slab_test_q against slab_test: a box on the walkers' 16-bit grid must be entered by every ray that enters the float box
__global__ void k_slab_q(const float *in, rtamd::NodeGrid G, uint32_t *out, size_t n) { // per case 13 floats: lo.xyz hi.xyz o.xyz d.xyz tbest
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 13 * i;
    const F3 o = f3(p[6], p[7], p[8]), d = f3(p[9], p[10], p[11]);
    float tn = 0.f, tq = 0.f;
    const bool hf = slab_test(make_float4(p[0], p[1], p[2], 0.f), make_float4(p[3], p[4], p[5], 0.f), make_ray_inv(o, d), p[12], tn);
    bool fits = true;
    uint4 b;
    b.x = rtamd::grid_axis_word(p[0], p[3], G.lo[0], G.step[0], fits);
    b.y = rtamd::grid_axis_word(p[1], p[4], G.lo[1], G.step[1], fits);
    b.z = rtamd::grid_axis_word(p[2], p[5], G.lo[2], G.step[2], fits);
    b.w = 0u;
    const bool hq = slab_test_q(b, make_ray_grid(G, o, d), p[12], tq);
    out[i] = (hf ? 1u : 0u) | (hq ? 2u : 0u) | (fits ? 4u : 0u) | (tq <= tn ? 8u : 0u);
}
// what the model of slab_test_q (tests/slab_fma_model.py) takes from the device: the reciprocals make_ray_grid forms its 1/d' from, and
// the grid test's entry distance as it is, for a bit-for-bit comparison
__global__ void k_slab_q_entry(const float *in, rtamd::NodeGrid G, float *rcp, float *entry, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 13 * i;
    for (int k = 0; k < 3; k++) { const float d = p[9 + k]; rcp[3 * i + k] = __builtin_amdgcn_rcpf(fabsf(d) > 1e-30f ? d : copysignf(1e-30f, d)); }
    bool fits = true;
    uint4 b;
    b.x = rtamd::grid_axis_word(p[0], p[3], G.lo[0], G.step[0], fits);
    b.y = rtamd::grid_axis_word(p[1], p[4], G.lo[1], G.step[1], fits);
    b.z = rtamd::grid_axis_word(p[2], p[5], G.lo[2], G.step[2], fits);
    b.w = 0u;
    float tq = 0.f;
    (void)slab_test_q(b, make_ray_grid(G, f3(p[6], p[7], p[8]), f3(p[9], p[10], p[11])), p[12], tq);
    entry[i] = tq;
}

// rt_pt_queue.h pt_pop on a bitmap of the test's own: every wave of the one workgroup makes n_calls calls, call c with the lanes of
// want[c] wanting a path.  got: [wave][call][64] results; cursor_out, count_out: [wave][call] the wave's cursor and the queue's count after the call.
#define HOOK_POP_NW 160
__global__ void k_pt_pop(uint32_t *bitmap, int *count, uint32_t nw, uint32_t cursor0, const unsigned long long *want, int n_calls, int from_start,
                         uint32_t *got, uint32_t *cursor_out, int *count_out) {
    __shared__ uint32_t bm[HOOK_POP_NW];
    __shared__ int cnt;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) bm[i] = bitmap[i];
    if (threadIdx.x == 0) cnt = *count;
    __syncthreads();
    uint32_t cursor = cursor0;
    for (int c = 0; c < n_calls; c++) {
        const uint32_t g = pt_pop(bm, &cnt, nw, cursor, ((want[c] >> lane) & 1ull) != 0ull, from_start != 0);
        got[((size_t)wave * n_calls + c) * 64 + lane] = g;
        const int left = pt_count(&cnt);
        if (lane == 0) { cursor_out[wave * n_calls + c] = cursor; count_out[wave * n_calls + c] = left; }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) bitmap[i] = bm[i];
    if (threadIdx.x == 0) *count = cnt;
}

// rt_ref_walk.h frame_sum on a node table of the test's own, one tree per thread (workgroups of FS_BATCH threads).  A node is four words
// {kind (FRAME_TOTAL / FRAME_ONE / FRAME_BOTH), left, right, value bits}; a node number beyond the table counts as a total of 0.
// LDS_VIEW: the stack is a StridedStack<FS_BATCH> over LDS, the layout of the persistent kernel's exact role; else a private array.
#define FS_BATCH 16
template <int MAXDEPTH, bool LDS_VIEW>
__global__ void k_frame_sum(const uint4 *nodes, uint32_t n_nodes, const uint32_t *roots, int n_roots, float *out) {
    __shared__ uint32_t area[LDS_VIEW ? MAXDEPTH * FS_BATCH : 1];
    uint32_t own[LDS_VIEW ? 1 : MAXDEPTH];
    const int i = blockIdx.x * FS_BATCH + threadIdx.x;
    if (i >= n_roots) return;
    auto node = [&](uint32_t cur, uint32_t &l, uint32_t &r, float &v) {
        if (cur >= n_nodes) { v = 0.f; return (int)FRAME_TOTAL; }
        const uint4 n = nodes[cur];
        l = n.y; r = n.z;
        if (n.x == FRAME_TOTAL) v = __uint_as_float(n.w);
        return (int)n.x;
    };
    if (LDS_VIEW) { const StridedStack<FS_BATCH> view = {area + threadIdx.x}; out[i] = frame_sum<MAXDEPTH>(view, node, roots[i]); }
    else out[i] = frame_sum<MAXDEPTH>(own, node, roots[i]);
}

// The host-side preparation (host/scene_prep.h) as text, one line per member of the prepared struct: `name element_count hash`, the
// hash FNV-1a (64 bit) over the member's raw bytes; a scalar is `name 1 bits`, its value's bits in hex.
namespace {
struct PreparedDigest {
    std::string text;
    void line(const char *name, size_t count, unsigned long long word, int digits) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s %zu %0*llx\n", name, count, digits, word);
        text += buf;
    }
    void bytes(const char *name, size_t count, const void *p, size_t n) {
        unsigned long long h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
        line(name, count, h, 16);
    }
    template <class T> void vec(const char *name, const std::vector<T> &v) { bytes(name, v.size(), v.data(), v.size() * sizeof(T)); }
    template <class T> void scalar(const char *name, const T &v) {
        static_assert(sizeof(T) <= 4, "scalars of the prepared structs are 32 bits at the most");
        uint32_t bits = 0;
        memcpy(&bits, &v, sizeof(T));
        line(name, 1, bits, 8);
    }
};
#define PD_VEC(m) D.vec(#m, P.m)
#define PD_SCALAR(m) D.scalar(#m, P.m)
void digest_of(PreparedDigest &D, const rtamd::PreparedScene &P) {
    PD_VEC(nodes); PD_VEC(light_nodes); PD_VEC(ref_nodes); PD_VEC(ref_light_nodes); PD_VEC(tri_box); PD_VEC(walk_box); PD_VEC(light_walk_box);
    PD_VEC(tripwires); PD_SCALAR(n_tripwire_groups); PD_SCALAR(box_c2); PD_SCALAR(box_pad); PD_VEC(light_sep); PD_SCALAR(light_sep_levels);
    PD_VEC(isect); PD_VEC(shade); PD_VEC(lights); PD_VEC(materials); PD_VEC(images); PD_VEC(texels);
    D.bytes("srgb_lut", 256, P.srgb_lut, sizeof P.srgb_lut);
    PD_SCALAR(env_image); PD_VEC(figure_order); PD_VEC(light_order); PD_SCALAR(bvh_depth); PD_SCALAR(light_bvh_depth);
}
void digest_of(PreparedDigest &D, const rtamd::PreparedScene6 &P) {
    PD_VEC(nodes); PD_VEC(light_nodes); PD_VEC(fast_light_nodes); PD_VEC(tris); PD_VEC(lights); PD_VEC(fast_lights); PD_SCALAR(fast_light_bvh_depth);
    PD_VEC(light_ref); PD_VEC(light_sep); PD_VEC(ref_nodes); PD_VEC(ref_light_nodes); PD_VEC(ref_tris); PD_VEC(tri_box); PD_SCALAR(box_c2);
    PD_VEC(boxes8); PD_SCALAR(box_pad); PD_SCALAR(light_sep_levels); PD_VEC(materials); PD_VEC(figure_order); PD_VEC(light_order);
    PD_SCALAR(bvh_depth); PD_SCALAR(light_bvh_depth);
}
void digest_of(PreparedDigest &D, const rtamd::PreparedScene5 &P) {
    PD_VEC(nodes); PD_VEC(light_nodes); PD_VEC(ref_nodes); PD_VEC(ref_light_nodes); PD_VEC(figs); PD_VEC(lights); PD_VEC(figure_order);
    PD_VEC(light_order); PD_SCALAR(n_nonplanes); PD_SCALAR(bvh_depth); PD_SCALAR(light_bvh_depth);
}
void digest_of(PreparedDigest &D, const rtamd::PreparedSceneTxt &P) { // listed behind the hw5 members of the same scene
    D.vec("txt.prims", P.prims); D.vec("txt.lights", P.lights); D.vec("txt.light_prims", P.light_prims);
    const uint32_t has_triangles = P.has_triangles ? 1u : 0u;
    D.scalar("txt.has_triangles", has_triangles);
}
#undef PD_VEC
#undef PD_SCALAR

// A device buffer of the shading hooks: filled from `src` when there is one; ok() says whether every step so far succeeded.
struct HookBuf {
    void *d = nullptr;
    size_t bytes;
    bool good;
    HookBuf(const void *src, size_t bytes_) : bytes(bytes_) {
        good = hipMalloc(&d, bytes ? bytes : 1) == hipSuccess;
        if (good && src) good = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    ~HookBuf() { (void)hipFree(d); }
    HookBuf(const HookBuf &) = delete;
    HookBuf &operator=(const HookBuf &) = delete;
    template <class T> T *as() const { return (T *)d; }
    bool back(void *dst) const { return hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};
inline dim3 hook_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
} // namespace

extern "C" {
// rt_pt_queue.h bit helpers on the host (no GPU needed): out[i] = pt_nth_bit(v[i], n[i]) / pt_low_bits(v[i], n[i])
void rtt_pt_nth_bit(const uint32_t *v, const int *n, int *out, size_t count) { for (size_t i = 0; i < count; i++) out[i] = pt_nth_bit(v[i], n[i]); }
void rtt_pt_low_bits(const uint32_t *v, const int *n, uint32_t *out, size_t count) { for (size_t i = 0; i < count; i++) out[i] = pt_low_bits(v[i], n[i]); }
// k_pt_pop with `waves` (1..4) waves on a bitmap of nw <= 160 words; bitmap and count are updated in place.  got: waves x n_calls x 64,
// cursor_out and count_out: waves x n_calls.
int rtt_pt_pop(uint32_t *bitmap, uint32_t nw, int *count, uint32_t cursor, const unsigned long long *want, int n_calls, int from_start, int waves,
               uint32_t *got, uint32_t *cursor_out, int *count_out) {
    if (nw == 0 || nw > HOOK_POP_NW || cursor >= nw || n_calls <= 0 || waves < 1 || waves > 4) return -1;
    const size_t n_res = (size_t)waves * n_calls;
    uint32_t *d_bm = nullptr, *d_got = nullptr, *d_cur = nullptr; int *d_cnt = nullptr, *d_left = nullptr; unsigned long long *d_want = nullptr;
    int rc = -2;
    if (hipMalloc((void **)&d_bm, nw * 4) == hipSuccess && hipMalloc((void **)&d_cnt, 4) == hipSuccess && hipMalloc((void **)&d_want, (size_t)n_calls * 8) == hipSuccess &&
        hipMalloc((void **)&d_got, n_res * 256) == hipSuccess && hipMalloc((void **)&d_cur, n_res * 4) == hipSuccess && hipMalloc((void **)&d_left, n_res * 4) == hipSuccess &&
        hipMemcpy(d_bm, bitmap, nw * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_cnt, count, 4, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_want, want, (size_t)n_calls * 8, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(k_pt_pop, dim3(1), dim3(64 * waves), 0, 0, d_bm, d_cnt, nw, cursor, d_want, n_calls, from_start, d_got, d_cur, d_left);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(bitmap, d_bm, nw * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(count, d_cnt, 4, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(got, d_got, n_res * 256, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(cursor_out, d_cur, n_res * 4, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(count_out, d_left, n_res * 4, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
    }
    (void)hipFree(d_bm); (void)hipFree(d_cnt); (void)hipFree(d_want); (void)hipFree(d_got); (void)hipFree(d_cur); (void)hipFree(d_left);
    return rc;
}
// host/fold_nodes.h on host memory (no GPU needed): nodes = n two-box nodes of 64 bytes, grid_box = lo.xyz hi.xyz of what the grid must hold,
// out = room for cap wide nodes of 64 bytes, grid_out = the grid's lo[3], step[3], istep[3].  Returns the number of wide nodes, -1 on error.
int rtt_fold_nodes(const void *nodes, uint32_t n, const float *grid_box, void *out, uint32_t cap, uint32_t *depth_out, float *grid_out) {
    try {
        std::vector<rtamd::GpuNode> in((const rtamd::GpuNode *)nodes, (const rtamd::GpuNode *)nodes + n);
        const rtamd::NodeGrid G = rtamd::make_node_grid(grid_box, grid_box + 3);
        std::vector<rtamd::GpuNode4Q> wide;
        uint32_t depth = 0;
        rtamd::fold_nodes(in, G, wide, depth);
        if (wide.size() > cap) return -1;
        memcpy(out, wide.data(), wide.size() * sizeof(rtamd::GpuNode4Q));
        *depth_out = depth;
        for (int k = 0; k < 3; k++) { grid_out[k] = G.lo[k]; grid_out[3 + k] = G.step[k]; grid_out[6 + k] = G.istep[k]; }
        return (int)wide.size();
    } catch (...) { return -1; }
}
// walk_arrays_fit (rt_types.h), the bound that scene creation answers RT_ERR_LIMIT for, on counts of the test's own (no GPU needed): 1 = they fit
int rtt_walk_arrays_fit(uint64_t n_tris, uint64_t n_lights, uint64_t n_nodes, uint64_t n_light_nodes) { return rtamd::walk_arrays_fit(n_tris, n_lights, n_nodes, n_light_nodes) ? 1 : 0; }
// The light records of an hw8 scene as its persistent light walker reads them, the pair of arrays of rt_types.h LightRest, and the lights in the
// reference's order: n_lights records each into test_out (48 bytes each), rest_out (96) and lights_out (144), room for `cap` of them.
// Returns n_lights, -1 on error.
int rtt_light_walk_arrays(const rt_scene *scene, void *test_out, void *rest_out, void *lights_out, uint32_t cap) {
    if (!scene || scene->flavor != RT_INTEGRATOR_HW8) return -1;
    const rtamd::SceneView &V = scene->view;
    const size_t n = V.n_lights;
    if (n > cap) return -1;
    if (n && (hipMemcpy(test_out, V.lights_walk_test, n * sizeof(rtamd::TriIsect), hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(rest_out, V.lights_walk_rest, n * sizeof(rtamd::LightRest), hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(lights_out, V.lights, n * sizeof(rtamd::LightRec), hipMemcpyDeviceToHost) != hipSuccess)) return -1;
    return (int)n;
}
// shard_slot_to_frame_slot (rt_device.h) on the host (no GPU needed) for the n_slots slots of shard `shard` of `count` of a width x height frame
// in square tiles: frame_slot[s] = the slot in frame order, in_frame[s] = 0 for a slot in a padding sub-tile.
int rtt_shard_to_frame_slots(int width, int height, int tile, uint32_t shard, uint32_t count, uint32_t n_slots, uint32_t *frame_slot, uint8_t *in_frame) {
    if (width <= 0 || height <= 0 || tile <= 0 || (tile & 7) || count == 0) return -1;
    const int tiles_x = (width + tile - 1) / tile, sub_w = (width + 7) / 8, sub_h = (height + 7) / 8;
    for (uint32_t s = 0; s < n_slots; s++) in_frame[s] = shard_slot_to_frame_slot(tile, tiles_x, sub_w, sub_h, shard, count, s, frame_slot[s]) ? 1 : 0;
    return 0;
}
// grid_box: lo.xyz hi.xyz of what the grid must hold.  out bits: 1 float box entered, 2 grid box entered, 4 the box fits the grid, 8 grid entry <= float entry
int rtt_slab_q(const float *cases, const float *grid_box, uint32_t *out, size_t n) {
    const rtamd::NodeGrid G = rtamd::make_node_grid(grid_box, grid_box + 3);
    float *d_in = nullptr; uint32_t *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * 13 * 4) != hipSuccess || hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    int rc = -1;
    if (hipMemcpy(d_in, cases, n * 13 * 4, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(k_slab_q, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, G, d_out, n);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
    }
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
}
// the same cases: rcp = n x 3 reciprocals of the (clamped) direction components as the device forms them, entry = n unclamped grid entry distances
int rtt_slab_q_entry(const float *cases, const float *grid_box, float *rcp, float *entry, size_t n) {
    const rtamd::NodeGrid G = rtamd::make_node_grid(grid_box, grid_box + 3);
    float *d_in = nullptr, *d_rcp = nullptr, *d_entry = nullptr;
    int rc = -1;
    if (hipMalloc((void **)&d_in, n * 13 * 4) == hipSuccess && hipMalloc((void **)&d_rcp, n * 12) == hipSuccess && hipMalloc((void **)&d_entry, n * 4) == hipSuccess &&
        hipMemcpy(d_in, cases, n * 13 * 4, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(k_slab_q_entry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, G, d_rcp, d_entry, n);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(rcp, d_rcp, n * 12, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(entry, d_entry, n * 4, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
    }
    (void)hipFree(d_in); (void)hipFree(d_rcp); (void)hipFree(d_entry);
    return rc;
}
int rtt_gap_code(const float *t, const float *t2, float *floor_out, uint32_t *code_out, size_t n) {
    float *d_t = nullptr, *d_t2 = nullptr, *d_f = nullptr; uint32_t *d_c = nullptr;
    if (hipMalloc((void **)&d_t, n * 4) != hipSuccess || hipMalloc((void **)&d_t2, n * 4) != hipSuccess || hipMalloc((void **)&d_f, n * 4) != hipSuccess || hipMalloc((void **)&d_c, n * 4) != hipSuccess) return -1;
    (void)hipMemcpy(d_t, t, n * 4, hipMemcpyHostToDevice); (void)hipMemcpy(d_t2, t2, n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_gap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_t, d_t2, d_f, d_c, n);
    int rc = (hipMemcpy(floor_out, d_f, n * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(code_out, d_c, n * 4, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : -2;
    (void)hipFree(d_t); (void)hipFree(d_t2); (void)hipFree(d_f); (void)hipFree(d_c);
    return rc;
}
int rtt_hit_stands(const float *cases16, uint32_t *out, size_t n) {
    float *d_in = nullptr; uint32_t *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * 64) != hipSuccess || hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    (void)hipMemcpy(d_in, cases16, n * 64, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_stands, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    int rc = hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
}
// The intersection layer (k_ref_box .. k_slab_padded above; rows as documented there).  0, or -1 for a refused argument, -2 when a HIP call fails.
int rtt_ref_box_test(const float *rows12, uint32_t *out2, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(rows12, n * 12 * 4), b_out(nullptr, n * 2 * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_ref_box, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out2) ? 0 : -2;
}
// rows15: positions (data, data2, data3), o, d.  The triangle's record is the host's own (scene_prep.cpp make_isect).
int rtt_tri_test(const float *rows15, const float *keep_t, uint32_t *out8, size_t n) {
    if (n == 0) return -1;
    std::vector<rtamd::TriIsect> isect(n);
    std::vector<float> rays(n * 6);
    for (size_t i = 0; i < n; i++) {
        isect[i] = rtamd::isect_of_positions(rows15 + 15 * i);
        memcpy(&rays[6 * i], rows15 + 15 * i + 9, 6 * sizeof(float));
    }
    HookBuf b_isect(isect.data(), n * sizeof(rtamd::TriIsect)), b_rays(rays.data(), n * 6 * 4), b_keep(keep_t, n * 4), b_out(nullptr, n * 8 * 4);
    if (!b_isect.good || !b_rays.good || !b_keep.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_tri, hook_grid(n), dim3(256), 0, 0, b_isect.as<rtamd::TriIsect>(), b_rays.as<float>(), b_keep.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out8) ? 0 : -2;
}
// cases16 as rtt_hit_stands takes them.  rtt_box_robust: bit 1 pt_box_robust<true>, bit 2 pt_box_robust<false> at P = o + t d;
// rtt_any_hit_stands: rq_any_hit_stands with the row's gap read as tmax.
static int run_robust(const float *cases16, uint32_t *out, size_t n, uint32_t mask, int shift) {
    if (n == 0) return -1;
    HookBuf b_in(cases16, n * 64), b_out(nullptr, n * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_robust, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<uint32_t>(), n);
    if (hipDeviceSynchronize() != hipSuccess || !b_out.back(out)) return -2;
    for (size_t i = 0; i < n; i++) out[i] = (out[i] & mask) >> shift;
    return 0;
}
int rtt_box_robust(const float *cases16, uint32_t *out, size_t n) { return run_robust(cases16, out, n, 3u, 0); }
int rtt_any_hit_stands(const float *cases16, uint32_t *out, size_t n) { return run_robust(cases16, out, n, 4u, 2); }
// rows12 as rtt_ref_box_test takes them; every box is padded as a scene whose largest |coordinate| is max_coord pads its walkers' boxes
// (host/scene_prep.h walk_box_of).  flag: slab_test's answer at tbest (the walkers' RT_T_MAX when it is negative), tnear: its entry distance.
int rtt_slab_padded(const float *rows12, float max_coord, float tbest, uint32_t *flag, float *tnear, size_t n) {
    if (n == 0) return -1;
    std::vector<float> boxes(n * 6);
    for (size_t i = 0; i < n; i++) rtamd::walk_box_of(rows12 + 12 * i, rows12 + 12 * i + 3, max_coord, &boxes[6 * i], &boxes[6 * i + 3]);
    HookBuf b_box(boxes.data(), n * 6 * 4), b_in(rows12, n * 12 * 4), b_flag(nullptr, n * 4), b_near(nullptr, n * 4);
    if (!b_box.good || !b_in.good || !b_flag.good || !b_near.good) return -2;
    hipLaunchKernelGGL(k_slab_padded, hook_grid(n), dim3(256), 0, 0, b_box.as<float>(), b_in.as<float>(), tbest < 0.f ? RT_T_MAX : tbest, b_flag.as<uint32_t>(), b_near.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_flag.back(flag) && b_near.back(tnear) ? 0 : -2;
}
// The analytic layer (k_quad .. k_cosine_txt above).  rows24: type, data, data2, data3, position, rotation (x y z w), o, d, one unused; the
// device records are the host's own (scene_prep.cpp pack_prim / pack_fig5), so load_prim / load_fig5 and the layouts are under test too.
int rtt_quad(const float *abc, uint32_t *out4, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(abc, n * 3 * 4), b_out(nullptr, n * 4 * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_quad, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out4) ? 0 : -2;
}
int rtt_slabs(const float *rows9, uint32_t *out2, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(rows9, n * 9 * 4), b_out(nullptr, n * 2 * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_slabs, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out2) ? 0 : -2;
}
namespace {
struct FigureRows {
    std::vector<rtamd::GpuPrim> prims;
    std::vector<rtamd::GpuFig5> figs;
    std::vector<float> rays, xs;
    bool ok = true;
    FigureRows(const float *rows, size_t n, size_t stride = 24) : prims(n), figs(n), rays(n * 6), xs(n * 3) {
        for (size_t i = 0; i < n; i++) {
            const float *r = rows + stride * i;
            rt_primitive p;
            memset(&p, 0, sizeof p);
            p.type = (int32_t)r[0];
            if (p.type < RT_PRIM_ELLIPSOID || p.type > RT_PRIM_TRIANGLE) { ok = false; return; }
            for (int k = 0; k < 3; k++) { p.data[k] = r[1 + k]; p.data2[k] = r[4 + k]; p.data3[k] = r[7 + k]; p.position[k] = r[10 + k]; p.color[k] = 1.f; p.emission[k] = 1.f; }
            for (int k = 0; k < 4; k++) p.rotation[k] = r[13 + k];
            p.kind = RT_MAT_DIFFUSE; p.ior = 1.f;
            prims[i] = rtamd::pack_prim(p);
            figs[i] = rtamd::pack_fig5(p);
            memcpy(&rays[6 * i], r + 17, 6 * sizeof(float));
            memcpy(&xs[3 * i], r + 17, 3 * sizeof(float));
        }
    }
};
}
// which: 0 k_fig (out: 25 words per row), 1 k_lpdf (2 words)
static int run_figure_rows(int which, const float *rows24, uint32_t *out, size_t n) {
    if (n == 0) return -1;
    const FigureRows R(rows24, n);
    if (!R.ok) return -1;
    const size_t width = which == 0 ? 25 : 2;
    HookBuf b_prims(R.prims.data(), n * sizeof(rtamd::GpuPrim)), b_figs(R.figs.data(), n * sizeof(rtamd::GpuFig5)), b_rays(R.rays.data(), n * 6 * 4), b_out(nullptr, n * width * 4);
    if (!b_prims.good || !b_figs.good || !b_rays.good || !b_out.good) return -2;
    if (which == 0) hipLaunchKernelGGL(k_fig, hook_grid(n), dim3(256), 0, 0, b_prims.as<rtamd::GpuPrim>(), b_figs.as<rtamd::GpuFig5>(), b_rays.as<float>(), b_out.as<uint32_t>(), n);
    else hipLaunchKernelGGL(k_lpdf, hook_grid(n), dim3(256), 0, 0, b_prims.as<rtamd::GpuPrim>(), b_figs.as<rtamd::GpuFig5>(), b_rays.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
int rtt_fig(const float *rows24, uint32_t *out25, size_t n) { return run_figure_rows(0, rows24, out25, n); }
int rtt_lpdf(const float *rows24, uint32_t *out2, size_t n) { return run_figure_rows(1, rows24, out2, n); }
// rows30: a figure row with x = o and d, then y 3, yn 3
int rtt_pdf_one(const float *rows30, uint32_t *out2, size_t n) {
    if (n == 0) return -1;
    const FigureRows R(rows30, n, 30);
    if (!R.ok) return -1;
    std::vector<float> pts(n * 12);
    for (size_t i = 0; i < n; i++) { memcpy(&pts[12 * i], rows30 + 30 * i + 17, 6 * sizeof(float)); memcpy(&pts[12 * i + 6], rows30 + 30 * i + 24, 6 * sizeof(float)); }
    HookBuf b_prims(R.prims.data(), n * sizeof(rtamd::GpuPrim)), b_figs(R.figs.data(), n * sizeof(rtamd::GpuFig5)), b_pts(pts.data(), n * 12 * 4), b_out(nullptr, n * 2 * 4);
    if (!b_prims.good || !b_figs.good || !b_pts.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_pdf_one, hook_grid(n), dim3(256), 0, 0, b_prims.as<rtamd::GpuPrim>(), b_figs.as<rtamd::GpuFig5>(), b_pts.as<float>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out2) ? 0 : -2;
}
// aux3: seed, whether the normal cache holds a value, its bits.  x = the row's o.
int rtt_lsample(const float *rows24, const uint32_t *aux3, uint32_t *out13, size_t n) {
    if (n == 0) return -1;
    const FigureRows R(rows24, n);
    if (!R.ok) return -1;
    HookBuf b_prims(R.prims.data(), n * sizeof(rtamd::GpuPrim)), b_figs(R.figs.data(), n * sizeof(rtamd::GpuFig5)), b_xs(R.xs.data(), n * 3 * 4), b_aux(aux3, n * 3 * 4), b_out(nullptr, n * 13 * 4);
    if (!b_prims.good || !b_figs.good || !b_xs.good || !b_aux.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_lsample, hook_grid(n), dim3(256), 0, 0, b_prims.as<rtamd::GpuPrim>(), b_figs.as<rtamd::GpuFig5>(), b_xs.as<float>(), b_aux.as<uint32_t>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out13) ? 0 : -2;
}
int rtt_face_point(const float *s3, const uint32_t *seeds, uint32_t *out4, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(s3, n * 3 * 4), b_seed(seeds, n * 4), b_out(nullptr, n * 4 * 4);
    if (!b_in.good || !b_seed.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_face_point, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_seed.as<uint32_t>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out4) ? 0 : -2;
}
int rtt_cosine_txt(const float *normals, const uint32_t *aux3, uint32_t *out6, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(normals, n * 3 * 4), b_aux(aux3, n * 3 * 4), b_out(nullptr, n * 6 * 4);
    if (!b_in.good || !b_aux.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_cosine_txt, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_aux.as<uint32_t>(), b_out.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out6) ? 0 : -2;
}
int rtt_logf(const float *in, float *out, size_t n) {
    float *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * 4) != hipSuccess || hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    if (hipMemcpy(d_in, in, n * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_in); (void)hipFree(d_out); return -2; }
    hipLaunchKernelGGL(k_logf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    int rc = hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
}
int rtt_asinf(const float *in, float *out, size_t n) {
    float *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * 4) != hipSuccess || hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    if (hipMemcpy(d_in, in, n * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_in); (void)hipFree(d_out); return -2; }
    hipLaunchKernelGGL(k_asinf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    int rc = hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
}
int rtt_atan2f(const float *y, const float *x, float *out, size_t n) {
    float *d_y = nullptr, *d_x = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_y, n * 4) != hipSuccess || hipMalloc((void **)&d_x, n * 4) != hipSuccess ||
        hipMalloc((void **)&d_out, n * 4) != hipSuccess) { (void)hipFree(d_y); (void)hipFree(d_x); return -1; }
    if (hipMemcpy(d_y, y, n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_x, x, n * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d_y); (void)hipFree(d_x); (void)hipFree(d_out); return -2;
    }
    hipLaunchKernelGGL(k_atan2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_y, d_x, d_out, n);
    int rc = hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_y); (void)hipFree(d_x); (void)hipFree(d_out);
    return rc;
}
// the miss shader's environment-map uv (rt_kernels_hw8.h env_uv) for n directions: d n x 3, uv n x 2
int rtt_env_uv(const float *d, float *uv, size_t n) {
    float *d_d = nullptr, *d_uv = nullptr;
    if (hipMalloc((void **)&d_d, n * 12) != hipSuccess || hipMalloc((void **)&d_uv, n * 8) != hipSuccess) return -1;
    if (hipMemcpy(d_d, d, n * 12, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_d); (void)hipFree(d_uv); return -2; }
    hipLaunchKernelGGL(k_env_uv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_d, d_uv, n);
    int rc = hipMemcpy(uv, d_uv, n * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_d); (void)hipFree(d_uv);
    return rc;
}
// The shading layer (k_brdf .. k_disk_point above; rows as documented there).  0, or -1 for a refused argument, -2 when a HIP call fails.
int rtt_brdf(int variant, const float *in, float *out, size_t n) {
    if (variant < 0 || variant > 2 || n == 0) return -1;
    HookBuf b_in(in, n * 18 * 4), b_out(nullptr, n * 3 * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_brdf, hook_grid(n), dim3(256), 0, 0, variant, b_in.as<float>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
int rtt_vndf(int form, const uint32_t *seed, const float *in, float *out, uint32_t *state, size_t n) {
    if (form < 0 || form > 1 || n == 0) return -1;
    HookBuf b_seed(seed, n * 4), b_in(in, n * 7 * 4), b_out(nullptr, n * 5 * 4), b_state(nullptr, n * 4);
    if (!b_seed.good || !b_in.good || !b_out.good || !b_state.good) return -2;
    hipLaunchKernelGGL(k_vndf, hook_grid(n), dim3(256), 0, 0, form, b_seed.as<uint32_t>(), b_in.as<float>(), b_out.as<float>(), b_state.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) && b_state.back(state) ? 0 : -2;
}
int rtt_vndf_local(const float *in, float *out, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(in, n * 6 * 4), b_out(nullptr, n * 3 * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_vndf_local, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
int rtt_vndf_pdf(const float *in, float *out, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(in, n * 10 * 4), b_out(nullptr, n * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_vndf_pdf, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
int rtt_cosine(const uint32_t *seed, const float *in, float *out, uint32_t *state, size_t n) {
    if (n == 0) return -1;
    HookBuf b_seed(seed, n * 4), b_in(in, n * 3 * 4), b_out(nullptr, n * 5 * 4), b_state(nullptr, n * 4);
    if (!b_seed.good || !b_in.good || !b_out.good || !b_state.good) return -2;
    hipLaunchKernelGGL(k_cosine, hook_grid(n), dim3(256), 0, 0, b_seed.as<uint32_t>(), b_in.as<float>(), b_out.as<float>(), b_state.as<uint32_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) && b_state.back(state) ? 0 : -2;
}
int rtt_cosine_pdf(const float *in, float *out, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(in, n * 6 * 4), b_out(nullptr, n * 4);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_cosine_pdf, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
int rtt_tonemap(const float *in, uint8_t *out, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(in, n * 4), b_out(nullptr, n);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_tonemap, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<uint8_t>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out) ? 0 : -2;
}
// seeds seed0 .. seed0 + n - 1 (n < 2^31): u and t n x 2 floats, cs n x 2 doubles
// The texture layer (k_sample_texture, k_apply_normal_map above).  The scene is an hw8 scene WITH an environment map, which scene
// preparation puts behind the images: its slot is the number of images, and every slot[i] must lie in [-1, that number).
int rtt_sample_texture(const rt_scene *scene, int form, const int32_t *slot, const float *uv2, const int32_t *srgb, float *out3, size_t n) {
    if (!scene || scene->flavor != RT_INTEGRATOR_HW8 || scene->view.env_image < 0 || form < 0 || form > 1 || n == 0) return -1;
    for (size_t i = 0; i < n; i++) if (slot[i] < -1 || slot[i] >= scene->view.env_image) return -1;
    HookBuf b_slot(slot, n * 4), b_uv(uv2, n * 8), b_srgb(srgb, n * 4), b_out(nullptr, n * 12);
    if (!b_slot.good || !b_uv.good || !b_srgb.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_sample_texture, hook_grid(n), dim3(256), 0, 0, scene->view, form, b_slot.as<int32_t>(), b_uv.as<float>(), b_srgb.as<int32_t>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out3) ? 0 : -2;
}
int rtt_apply_normal_map(const float *in10, float *out3, size_t n) {
    if (n == 0) return -1;
    HookBuf b_in(in10, n * 40), b_out(nullptr, n * 12);
    if (!b_in.good || !b_out.good) return -2;
    hipLaunchKernelGGL(k_apply_normal_map, hook_grid(n), dim3(256), 0, 0, b_in.as<float>(), b_out.as<float>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_out.back(out3) ? 0 : -2;
}
int rtt_disk_point(uint32_t seed0, size_t n, float *u, float *t, double *cs) {
    if (n == 0 || n >= (1u << 31)) return -1;
    HookBuf b_u(nullptr, n * 8), b_t(nullptr, n * 8), b_cs(nullptr, n * 16);
    if (!b_u.good || !b_t.good || !b_cs.good) return -2;
    hipLaunchKernelGGL(k_disk_point, hook_grid(n), dim3(256), 0, 0, seed0, b_u.as<float>(), b_t.as<float>(), b_cs.as<double>(), n);
    return hipDeviceSynchronize() == hipSuccess && b_u.back(u) && b_t.back(t) && b_cs.back(cs) ? 0 : -2;
}
// k_rng_triple: out = n_seeds x 2 x 8 words
int rtt_rng_triple(uint32_t seed0, int n_seeds, int prior, uint32_t *out) {
    if (n_seeds <= 0 || prior < 0 || prior > 1) return -1;
    uint32_t *d_out = nullptr;
    const size_t n = (size_t)n_seeds * 16;
    if (hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_rng_triple, dim3((n_seeds + 63) / 64), dim3(64), 0, 0, seed0, n_seeds, prior, d_out);
    int rc = (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : -2;
    (void)hipFree(d_out);
    return rc;
}
// streams for seeds seed0 .. seed0+n_seeds-1: n_u uniforms then n_n normals each
int rtt_rng_streams(uint32_t seed0, int n_seeds, int n_u, int n_n, float *out) {
    float *d_out = nullptr;
    size_t n = (size_t)n_seeds * (n_u + n_n);
    if (hipMalloc((void **)&d_out, n * 4) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_rng, dim3((n_seeds + 63) / 64), dim3(64), 0, 0, seed0, n_seeds, n_u, n_n, d_out);
    int rc = hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
    (void)hipFree(d_out);
    return rc;
}
// k_frame_sum for n_roots trees of a table of n_nodes nodes (4 words each).  variant 0: depth 64, private stack; 1: depth 64, strided LDS view;
// 2: depth 128, private stack.  out: n_roots floats.
int rtt_frame_sum(const uint32_t *nodes, uint32_t n_nodes, const uint32_t *roots, int n_roots, int variant, float *out) {
    if (n_roots <= 0 || n_nodes == 0 || variant < 0 || variant > 2) return -1;
    uint4 *d_nodes = nullptr; uint32_t *d_roots = nullptr; float *d_out = nullptr;
    int rc = -2;
    if (hipMalloc((void **)&d_nodes, (size_t)n_nodes * 16) == hipSuccess && hipMalloc((void **)&d_roots, (size_t)n_roots * 4) == hipSuccess &&
        hipMalloc((void **)&d_out, (size_t)n_roots * 4) == hipSuccess &&
        hipMemcpy(d_nodes, nodes, (size_t)n_nodes * 16, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_roots, roots, (size_t)n_roots * 4, hipMemcpyHostToDevice) == hipSuccess) {
        const dim3 grid((unsigned)((n_roots + FS_BATCH - 1) / FS_BATCH)), block(FS_BATCH);
        if (variant == 0) hipLaunchKernelGGL((k_frame_sum<64, false>), grid, block, 0, 0, d_nodes, n_nodes, d_roots, n_roots, d_out);
        else if (variant == 1) hipLaunchKernelGGL((k_frame_sum<64, true>), grid, block, 0, 0, d_nodes, n_nodes, d_roots, n_roots, d_out);
        else hipLaunchKernelGGL((k_frame_sum<128, false>), grid, block, 0, 0, d_nodes, n_nodes, d_roots, n_roots, d_out);
        rc = (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, (size_t)n_roots * 4, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : -3;
    }
    (void)hipFree(d_nodes); (void)hipFree(d_roots); (void)hipFree(d_out);
    return rc;
}
// The on-device tree builder (host/device_build.h build_tree_on_device, the function rtamd_scene.hip calls) on n host boxes of 8 floats
// (lo.xyz, -, hi.xyz, -): nodes_out = room for node_cap two-box nodes of 64 bytes, order_out = n words, last_out = n bytes, depth_out = the
// deepest leaf.  Returns the number of nodes; -1 when the builder refuses or a HIP call fails, -2 for any other exception, -3 when the
// tree has more than node_cap nodes (nothing is written then).
int rtt_build_tree(const float *boxes8, uint32_t n, float abs_pad, uint32_t max_depth, void *nodes_out, uint32_t node_cap, uint32_t *order_out,
                   uint8_t *last_out, uint32_t *depth_out) {
    float *d_boxes = nullptr;
    rtamd::DeviceTree t;
    int rc;
    try {
        if (n) {
            HIP_CHECK(hipMalloc((void **)&d_boxes, (size_t)n * 32));
            HIP_CHECK(hipMemcpy(d_boxes, boxes8, (size_t)n * 32, hipMemcpyHostToDevice));
        }
        t = rtamd::build_tree_on_device(d_boxes, n, abs_pad, max_depth);
        if (t.n_nodes > node_cap) rc = -3;
        else {
            HIP_CHECK(hipMemcpy(nodes_out, t.nodes, (size_t)t.n_nodes * sizeof(rtamd::GpuNode), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(order_out, t.order, (size_t)n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(last_out, t.last, (size_t)n, hipMemcpyDeviceToHost));
            *depth_out = t.depth;
            rc = (int)t.n_nodes;
        }
    } catch (const std::exception &) { rc = -1; } catch (...) { rc = -2; }
    rtamd::free_device_tree(t);
    (void)hipFree(d_boxes);
    return rc;
}
// gather_records (host/device_build.h) on n host records of elem_bytes with a leaf order and leaf marks of the test's own: out = n records.
// mark_word: the index of the records' mark word, -1 for none.  Returns 0; -1 when gather_records refuses (a size that is no multiple of
// 16) or a HIP call fails, -2 for any other exception, -4 for an order entry or a mark word outside the records (not run).
int rtt_gather_records(const void *records, uint32_t n, uint32_t elem_bytes, const uint32_t *order, const uint8_t *last, int mark_word, int or_into_word, void *out) {
    if (n == 0 || elem_bytes == 0 || mark_word < -1 || (mark_word >= 0 && (uint32_t)mark_word >= elem_bytes / 4)) return -4;
    for (uint32_t i = 0; i < n; i++) if (order[i] >= n) return -4;
    void *d_in = nullptr, *d_out = nullptr;
    rtamd::DeviceTree t;
    int rc;
    try {
        const size_t bytes = (size_t)n * elem_bytes;
        HIP_CHECK(hipMalloc(&d_in, bytes)); HIP_CHECK(hipMalloc(&d_out, bytes));
        HIP_CHECK(hipMalloc((void **)&t.order, (size_t)n * 4)); HIP_CHECK(hipMalloc((void **)&t.last, n));
        HIP_CHECK(hipMemcpy(d_in, records, bytes, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_out, 0, bytes));
        HIP_CHECK(hipMemcpy(t.order, order, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(t.last, last, n, hipMemcpyHostToDevice));
        rtamd::gather_records(d_in, d_out, t, n, elem_bytes, mark_word, or_into_word != 0);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
        rc = 0;
    } catch (const std::exception &) { rc = -1; } catch (...) { rc = -2; }
    rtamd::free_device_tree(t);
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc;
}
// The guard of the C boundary (host/rt_guard.h) around a body that throws a HipError (kind 0), a std::bad_alloc (1), a std::runtime_error (2)
// or an int (3), or returns 5 (anything else): the guard's answer; the message is in the library's rt_last_error().  Host only.
// The decision of an adaptive slice (host/rt_adaptive_decide.h) on a table of the test's own: sub_w * sub_h entries in, their new flags out.
int rtt_adaptive_decide(const rt_adaptive_tile *tiles, const rt_adaptive_params *params, int32_t sub_w, int32_t sub_h, int32_t n_samples, uint32_t *flags) {
    if (!tiles || !params || !flags || sub_w < 1 || sub_h < 1) return RT_ERR_INVALID_ARG;
    rtamd::adaptive_decide(tiles, *params, sub_w, sub_h, n_samples, flags);
    return RT_OK;
}

// The planning step of an adaptive slice over a view set (host/rt_view_adaptive_plan.h) on tables of the test's own: n_views tables of
// sub_w * sub_h entries and their observed samples in; out, for a slice of n_samples, the flags the call decides before it launches
// (tile_mask: the stored flags), the ascending list of words view * tiles + sub-tile with its length, and the monitor's numbers per
// (view, sub-tile), 24 bytes each.  tile_mask != NULL is rt_view_adaptive_render_tiles' plan, else view_mask (nullable) is the policy's.
int rtt_view_adaptive_plan(const rt_adaptive_tile *tiles, const int32_t *observed, const rt_adaptive_params *params, int32_t sub_w, int32_t sub_h, int32_t n_views,
                           int32_t n_samples, const uint8_t *view_mask, const uint8_t *tile_mask, uint32_t *flags, uint32_t *list, uint32_t *n_list, void *args) {
    if (!tiles || !observed || !params || !flags || !list || !n_list || !args || sub_w < 1 || sub_h < 1 || n_views < 1) return RT_ERR_INVALID_ARG;
    const size_t per_view = (size_t)sub_w * (size_t)sub_h, n = per_view * (size_t)n_views;
    std::vector<uint32_t> l;
    if (tile_mask) {
        for (size_t G = 0; G < n; G++) flags[G] = tiles[G].flags;
        rtamd::view_adaptive_list_tiles(tile_mask, n, l);
    } else {
        rtamd::view_adaptive_decide(tiles, *params, sub_w, sub_h, n_views, n_samples, view_mask, flags);
        rtamd::view_adaptive_list_policy(flags, per_view, n_views, view_mask, l);
    }
    std::vector<rtamd::AdTileArgs> a;
    rtamd::adaptive_slice_args(tiles, observed, n, n_samples, l, a);
    memcpy(list, l.data(), l.size() * sizeof(uint32_t));
    *n_list = (uint32_t)l.size();
    memcpy(args, a.data(), a.size() * sizeof(rtamd::AdTileArgs));
    return RT_OK;
}

// The camera check of a view set (host/rt_views_camera.h): RT_OK, or RT_ERR_INVALID_ARG with the reason in `why` (cut to `capacity`).  Host only.
int rtt_views_camera_check(const rt_camera *camera, char *why, size_t capacity) {
    if (!camera) return RT_ERR_INVALID_ARG;
    const std::string reason = rtamd::views_camera_check(*camera);
    if (why && capacity) snprintf(why, capacity, "%s", reason.c_str());
    return reason.empty() ? RT_OK : RT_ERR_INVALID_ARG;
}

int rtt_guard_probe(int kind) {
    return rtamd::guarded("rtt_guard_probe: ", [&]() -> int {
        if (kind == 0) throw rtamd::HipError("hipProbe(): failed");
        if (kind == 1) throw std::bad_alloc();
        if (kind == 2) throw std::runtime_error("a runtime error");
        if (kind == 3) throw 7;
        return 5;
    });
}
// The preparation of `desc` as the integrator's flavour sees it (HW8 / HW7: prepare_scene, HW6: prepare_scene_hw6, HW5: prepare_scene_hw5 and
// then prepare_scene_txt), digested into `out` (PreparedDigest above).  Returns the text's length (the terminator not counted; nothing is
// written when it exceeds capacity - 1), or the guard's code with the preparation's refusal in rt_last_error().  Host only.
int rtt_prepared_digest(const rt_scene_desc *desc, int integrator, int tree_on_device, char *out, size_t capacity) {
    if (!desc || !out) return RT_ERR_INVALID_ARG;
    return rtamd::guarded("rtt_prepared_digest: ", [&]() -> int {
        PreparedDigest D;
        if (integrator == RT_INTEGRATOR_HW8 || integrator == RT_INTEGRATOR_HW7) { rtamd::PreparedScene P; rtamd::prepare_scene(*desc, P, tree_on_device != 0); digest_of(D, P); }
        else if (integrator == RT_INTEGRATOR_HW6) { rtamd::PreparedScene6 P; rtamd::prepare_scene_hw6(*desc, P, tree_on_device != 0); digest_of(D, P); }
        else if (integrator == RT_INTEGRATOR_HW5) {
            rtamd::PreparedScene5 P; rtamd::prepare_scene_hw5(*desc, P); digest_of(D, P);
            rtamd::PreparedSceneTxt T; rtamd::prepare_scene_txt(*desc, T); digest_of(D, T);
        } else return RT_ERR_UNSUPPORTED;
        if (D.text.size() + 1 <= capacity) memcpy(out, D.text.c_str(), D.text.size() + 1);
        return (int)D.text.size();
    });
}
}

// Batched ray queries (include/rtamd.h: rt_query_closest, rt_query_light_pdf): the two functions the render loop spends its time in, for
// rays of the caller's own.  BVH::intersect (hw8/src/include/bvh.h:111-142) and FiguresMix::getTotalPdf / size (distributions.h:122-165),
// bit for bit, over the trees and with the walkers, the gate and the reference-order walks the renders use: nothing here walks a tree
// in a way of its own.  Per chunk of rays:
//
//   rq_classify_kernel       every ray once: invalid (answered at once, never walked), fast list, or exact list
//   rq_closest_kernel        wf_walk_loop with the policy RqTraceWalk: WfTraceWalk's node step and leaf phase, the ray read from the ray
//                            array, the result (t, u, v, hit word with the gap code) left in a 16-byte record per ray
//   rq_resolve_kernel        the gate of pt_shade_item (pt_tripwire, pt_hit_stands): a hit that stands is final and its attributes are
//                            written; every other ray is appended to the exact list
//   rq_closest_exact_kernel  ref_closest_hit, one lane per ray of the exact list (RT_HIT_EXACT_WALK), as wf_trace_exact_kernel does
//   rq_light_kernel          wf_walk_loop with RqLightWalk (WfLightWalk's walk and merge); what it cannot finish goes on the exact list
//   rq_light_exact_kernel    the reference-order frame walk, as wf_light_exact_kernel does
// and for rt_query_occluded (the last section of this file): rq_classify_occluded_kernel, rq_any_kernel (wf_walk_loop with RqAnyWalk, a
// walk that ends at the first hit below the ray's bound), rq_any_resolve_kernel (the any-hit gate), rq_any_exact_kernel.
//
// What the gate covers, and the rule of the fast list.  The gate's margins (rt_exact.h) bound the rounding of the reference's slab test by
// 2^-23 |t| + 2^-24 |o - centre|_j / |d_j| per term, with c2 = 2^-20 max|coordinate| of scene and camera standing for |o - centre|: the ray
// starts no farther from a box than the scene is large.  Render rays start at the camera or on a surface; a caller's ray need not.  The
// bound is homogeneous in d (t scales with 1 / |d|), but the gate's reciprocals are clamped at |d_k| = 1e-30 and its products were only
// ever looked at for directions of about unit length.  So a valid ray takes the fast path only when
//     max_k |o_k| <= max|coordinate| of scene and camera,   every |d_k| >= 1e-30 (no exact zero),   1/16 <= |d| <= 16;
// every other valid ray goes straight to the exact list, where no margin is needed.  Too cautious costs speed only.  The four-wide grid
// nodes of the persistent kernels are not used: the grid holds only origins inside scene and camera.
// A ray with a non-finite component or d == 0 is invalid: a miss with RT_HIT_INVALID_RAY (light pdf: 0), never walked.
// A light tree deeper than the LDS stack columns has no lean walker with a gate (the renders' WfLightFrameWalk trusts the padded boxes):
// all its queries take the exact list.  A scene tree that deep takes RqTraceWalk's SPILL variant, as the renders do.
//
// Scenes without the reference's tree (RT_BUILD_DEVICE_BVH) or with the gate off (RTAMD_NO_EXACT_BOXES) have SceneView::exact_boxes == 0:
// every fast answer stands, and the exact list is walked by the plain walks over the padded boxes (closest_hit, light_pdf_sum), which
// give the same closest triangle with the tie rule in figure (there: load) order.
//
// Attributes of a hit: t, the geometric normal after the inside flip (geom_normal), texture coordinates, shading normal and tangent
// with the expressions of shade_fetch_attr (primitives.cpp:110-119); that function itself ends in the texture taps and the normal map
// and hands none of them out, so the four interpolations are restated here.  The reference's x86 build gives an invalid operation
// (0 x inf of a zero-length normalisation) the NaN with the sign bit set, the GPU the one without: rq_x86_nan sets it.
#pragma once
#include "rt_wavefront.h"
#include "rt_types_query.h"

namespace rtamd {
namespace dev {

// rt_hit::flags (include/rtamd.h)
#define RQ_HIT_INSIDE 1u
#define RQ_HIT_EXACT_WALK 2u
#define RQ_HIT_INVALID_RAY 4u

#define RQ_INVALID 0
#define RQ_FAST 1
#define RQ_EXACT 2

RT_DEV void rq_load_ray(const QueryView &Q, uint32_t i, F3 &o, F3 &d) { // rt_ray is only 4-byte aligned
    const float *p = Q.rays + 6 * (size_t)i;
    o = f3(p[0], p[1], p[2]); d = f3(p[3], p[4], p[5]);
}
RT_DEV bool rq_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
RT_DEV bool rq_valid_ray(F3 o, F3 d) { // every query's rule: finite, and d != 0
    if (!(rq_finite(o.x) && rq_finite(o.y) && rq_finite(o.z) && rq_finite(d.x) && rq_finite(d.y) && rq_finite(d.z))) return false;
    return fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)) > 0.f;
}
RT_DEV int rq_classify(const QueryView &Q, F3 o, F3 d) {
    if (!rq_valid_ray(o, d)) return RQ_INVALID;
    const float dmin = fminf(fminf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    if (Q.reference_walk) return RQ_EXACT;
    const float omax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)), l2 = len2(d);
    return omax <= Q.origin_bound && dmin >= 1e-30f && l2 >= 0.00390625f && l2 <= 256.f ? RQ_FAST : RQ_EXACT;
}

RT_DEV float rq_x86_nan(float v) { return v != v ? __uint_as_float(__float_as_uint(v) | 0x80000000u) : v; }
RT_DEV uint32_t rq_bits(float v) { return __float_as_uint(rq_x86_nan(v)); }
// -1. * v where the reference's build negates by flipping the sign bit, a NaN's included: x86's NaN first, then the flip.
RT_DEV uint32_t rq_bits_negated(float v) { return rq_bits(v) ^ 0x80000000u; }
// A light pdf that is a NaN became one in a term's fabs(d . normal) (distributions.h:68-70), which clears the sign; the additions and the
// division after it hand that NaN on as it is.
RT_DEV float rq_pdf_nan(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }

// One rt_hit: t | triangle | ng.xyz | texcoord.xy | ns.xyz | tangent.xyzw | flags | reserved.
RT_DEV void rq_write_hit(const SceneView &S, const QueryView &Q, uint32_t ray, float t, float u, float v, uint32_t hit, uint32_t flags) {
    uint4 *out = Q.hits + 4 * (size_t)ray;
    if (hit == WF_MISS) {
        out[0] = make_uint4(0u, 0xFFFFFFFFu, 0u, 0u); out[1] = make_uint4(0u, 0u, 0u, 0u); out[2] = make_uint4(0u, 0u, 0u, 0u);
        out[3] = make_uint4(0u, 0u, flags, 0u);
        return;
    }
    const uint32_t fig = hit & WF_INDEX_MASK;
    const bool inside = (hit & WF_INSIDE_BIT) != 0u;
    const F3 ng = geom_normal(load_tri_normal(S, fig), inside);                  // primitives.cpp:21-24,123
    const TriShadeHead H = load_shade_head(S, fig);
    const float tu = H.s4.z + u * H.s5.x + v * H.s5.z;                           // :111-114
    const float tv = H.s4.w + u * H.s5.y + v * H.s5.w;
    const float4 *q = reinterpret_cast<const float4 *>(S.tri_shade + fig);
    const float4 s0 = q[0], s1 = q[1], s2 = q[2], s3 = q[3];
    const F3 n3 = f3(s0.x, s0.y, s0.z), dn1 = f3(s0.w, s1.x, s1.y), dn2 = f3(s1.z, s1.w, s2.x);
    F3 sn = n3 + u * dn1 + v * dn2;                                               // :110
    sn = normalize(sn);                                                           // :117; the flip of :118-119 is made on the bits below
    const F3 t3 = f3(s2.y, s2.z, s2.w), dt1 = f3(s3.x, s3.y, s3.z), dt2 = f3(s3.w, H.s4.x, H.s4.y);
    F3 tg = t3 + u * dt1 + v * dt2;                                               // :115
    tg = normalize(tg);                                                           // :116
    out[0] = make_uint4(rq_bits(t), __float_as_uint(H.s6.z), rq_bits(ng.x), rq_bits(ng.y)); // TriShade::orig: figure order -> LOAD order
    out[1] = make_uint4(rq_bits(ng.z), rq_bits(tu), rq_bits(tv), inside ? rq_bits_negated(sn.x) : rq_bits(sn.x));
    out[2] = make_uint4(inside ? rq_bits_negated(sn.y) : rq_bits(sn.y), inside ? rq_bits_negated(sn.z) : rq_bits(sn.z), rq_bits(tg.x), rq_bits(tg.y));
    out[3] = make_uint4(rq_bits(tg.z), __float_as_uint(H.s6.x), flags | (inside ? RQ_HIT_INSIDE : 0u), 0u);
}

// ---- every ray once ---------------------------------------------------------------------------------------------------------------------
// LIGHT: the light-pdf query (an invalid ray answers 0, `all_exact` sends every valid ray to the exact list); else the closest hit (a
// scene without triangles answers every valid ray with a miss here: its tree has no node to walk).
template <bool LIGHT>
__global__ __launch_bounds__(256) void rq_classify_kernel(SceneView S, QueryView Q, uint32_t all_exact) {
    __shared__ uint32_t buf_f[WF_BUF], buf_e[WF_BUF];
    __shared__ uint32_t cnt_f, cnt_e, gbase;
    if (threadIdx.x == 0) { cnt_f = 0; cnt_e = 0; }
    __syncthreads();
    Pusher fast; fast.buf = buf_f; fast.cnt = &cnt_f;
    Pusher exact; exact.buf = buf_e; exact.cnt = &cnt_e;
    for (uint32_t base = blockIdx.x * 256u; base < Q.n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        if (i < Q.n) {
            F3 o, d;
            rq_load_ray(Q, i, o, d);
            const int kind = rq_classify(Q, o, d);
            if (kind == RQ_INVALID) {
                if (LIGHT) Q.pdf[i] = 0.f; else rq_write_hit(S, Q, i, 0.f, 0.f, 0.f, WF_MISS, RQ_HIT_INVALID_RAY);
                atomicAdd(Q.totals + RQ_TOTAL_INVALID, 1ull);
            } else if (!LIGHT && S.n_tris == 0u) rq_write_hit(S, Q, i, 0.f, 0.f, 0.f, WF_MISS, 0u);
            else if (kind == RQ_FAST && !all_exact) wf_push(fast, i);
            else wf_push(exact, i);
        }
        __syncthreads();
        if (cnt_f > WF_BUF - 256) wf_flush(fast, Q.q_fast, Q.ctr + RQ_CTR_FAST, &gbase);
        if (cnt_e > WF_BUF - 256) wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
    }
    __syncthreads();
    wf_flush(fast, Q.q_fast, Q.ctr + RQ_CTR_FAST, &gbase);
    wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
}

// ---- closest hit: WfTraceWalk's walk for a ray of the ray array ---------------------------------------------------------------------------
// The node step and the leaf phase are WfTraceWalk's, line for line (that struct reads its ray from a path record and publishes into
// one, in members its step calls; sharing them would put a template layer into the render kernels' walker, which must not change).
template <bool SPILL> struct RqTraceWalk : WfWalkRay {
    static constexpr int HIST = -1;
    static constexpr bool WAVE_STATS = false;
    const SceneView &S; const QueryView &Q; WfStack<SPILL> stk;
    WfClosest best;
    RT_DEV RqTraceWalk(const SceneView &S_, const QueryView &Q_, const WfView &W_, uint32_t (*stack)[64], int lds_limit) : S(S_), Q(Q_), stk(W_, stack, lds_limit) {}
    RT_DEV void begin(uint32_t item) { // item: the ray's index in the chunk
        slot = item;
        rq_load_ray(Q, item, o, d);
        ray = make_ray_inv(o, d);
        cur = 0; sp = 0;
        best.reset(S, d);
    }
    RT_DEV bool next() { // the walk goes on with what its stack holds, or leaves what WfClosest::store leaves: the gate needs the runner-up's gap
        if (sp == 0) {
            Q.rec[slot] = make_float4(best.best_t, best.best_u, best.best_v,
                                      __uint_as_float(S.exact_boxes && best.hit != WF_MISS ? best.hit | pt_gap_code(best.best_t, best.t2) : best.hit));
            return true;
        }
        cur = stk.pop(sp);
        return false;
    }
    template <bool COUNT> RT_DEV bool step(WfWalkStat<COUNT> &n) {
        const float4 *q = reinterpret_cast<const float4 *>(S.nodes + cur);
        float4 lo0 = q[0], hi0 = q[1], lo1 = q[2], hi1 = q[3];
        n.node();
        float n0, n1;
        bool h0 = slab_test(lo0, hi0, ray, best.cull_t, n0);
        bool h1 = slab_test(lo1, hi1, ray, best.cull_t, n1);
        uint32_t c0 = __float_as_uint(lo0.w), c1 = __float_as_uint(lo1.w);
        if (h0 & h1) {
            bool swap = n1 < n0;
            stk.push(sp, swap ? c0 : c1);
            cur = swap ? c1 : c0;
        } else {
            cur = h0 ? c0 : c1;
            if (!(h0 | h1)) return next();
        }
        return false;
    }
    template <bool COUNT> RT_DEV bool leaf(WfWalkStat<COUNT> &n) {
        if (cur != RT_EMPTY_LEAF) {
            uint32_t i = cur & ~RT_LEAF_BIT;
            for (;;) {
                TriIsect T = load_isect(S.tri_walk + i);
                n.tri();
                float t, u, v; bool inside;
                if (tri_test_closer(T, o, d, best.cull_t, t, u, v, inside)) best.offer(S, T.pad >> 1, t, u, v, inside);
                if (T.pad & 1u) break;
                i++;
            }
        }
        return next();
    }
};

template <bool SPILL>
__global__ __launch_bounds__(256) void rq_closest_kernel(SceneView S, QueryView Q, int refill, int leaf_batch, int dyn, int lds_limit) {
    __shared__ uint32_t lds_stack[4][WF_STACK][64];
    WfView W{};
    W.ovf = Q.ovf;
    RqTraceWalk<SPILL> w(S, Q, W, lds_stack[threadIdx.x >> 6], lds_limit);
    wf_walk_loop<false>(w, Q.q_fast, wf_slice(Q.ctr[RQ_CTR_FAST], Q.ctr + RQ_CTR_HEAD, dyn, 0u, gridDim.x, true), nullptr, refill, leaf_batch);
}

// The gate, as pt_shade_item applies it: a tripwire, or a hit that does not stand, sends the ray to the exact list.
__global__ __launch_bounds__(256) void rq_resolve_kernel(SceneView S, QueryView Q) {
    __shared__ uint32_t buf[WF_BUF];
    __shared__ uint32_t cnt, gbase;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    Pusher exact; exact.buf = buf; exact.cnt = &cnt;
    const uint32_t count = Q.ctr[RQ_CTR_FAST];
    for (uint32_t base = blockIdx.x * 256u; base < count; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        if (i < count) {
            const uint32_t ray = Q.q_fast[i];
            const float4 r = Q.rec[ray];
            const uint32_t hit = __float_as_uint(r.w);
            bool stands = true;
            if (S.exact_boxes) {
                F3 o, d;
                rq_load_ray(Q, ray, o, d);
                if (S.n_tripwire_groups && pt_tripwire(S, o, d)) stands = false;
                else if (hit != WF_MISS) {
                    const float4 *bx = reinterpret_cast<const float4 *>(S.tri_box) + 2 * (size_t)(hit & WF_INDEX_MASK);
                    const float4 lo = bx[0], hi = bx[1];
                    stands = pt_hit_stands(f3(lo.x, lo.y, lo.z), f3(hi.x, hi.y, hi.z), o, d, r.x, pt_gap_floor(hit, r.x), S.box_c2, S.box_c2x, S.cull_k);
                }
            }
            if (stands) rq_write_hit(S, Q, ray, r.x, r.y, r.z, hit, 0u);
            else wf_push(exact, ray);
        }
        __syncthreads();
        if (cnt > WF_BUF - 256) wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
    }
    __syncthreads();
    wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
}

// The exact list: the reference's own walk over its own tree, one lane per ray; the last kernel of a chunk, so it also adds the list's
// length to the call's total.
__global__ __launch_bounds__(64) void rq_closest_exact_kernel(SceneView S, QueryView Q) {
    const uint32_t count = Q.ctr[RQ_CTR_EXACT];
    uint32_t stack[RT_STACK_SIZE];
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const uint32_t ray = Q.q_exact[i];
        F3 o, d;
        rq_load_ray(Q, ray, o, d);
        float bt, bu, bv; uint32_t hit;
        if (S.exact_boxes == 1u) ref_closest_hit(S, o, d, stack, bt, bu, bv, hit);
        else {
            Counters cnt; cnt.closest = cnt.lightq = cnt.nodes = cnt.tris = 0;
            const HitRec h = closest_hit<false>(S, o, d, stack, cnt);
            bt = h.t; bu = h.u; bv = h.v;
            hit = h.idx < 0 ? WF_MISS : (uint32_t)h.idx | (h.inside ? WF_INSIDE_BIT : 0u);
        }
        rq_write_hit(S, Q, ray, bt, bu, bv, hit, RQ_HIT_EXACT_WALK);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(Q.totals + RQ_TOTAL_EXACT, (unsigned long long)count);
}

// ---- light pdf: WfLightWalk's walk and merge for a ray of the ray array -------------------------------------------------------------------
// As RqTraceWalk: the step and the leaf phase are WfLightWalk's; a sum that is complete goes to pdf[ray] divided by the light count as
// wf_add_light_pdf divides it (distributions.h:123), one that is not goes on the exact list.
struct RqLightWalk : WfWalkRay {
    static constexpr int HIST = -1;
    static constexpr bool WAVE_STATS = false;
    const SceneView &S; const QueryView &Q; uint32_t (*stack)[64];
    const int lane = threadIdx.x & 63;
    bool overflow = false;
    int k = 0;
    RT_DEV RqLightWalk(const SceneView &S_, const QueryView &Q_, uint32_t (*stack_)[64]) : S(S_), Q(Q_), stack(stack_) {}
    RT_DEV void begin(uint32_t item) {
        slot = item;
        rq_load_ray(Q, item, o, d);
        ray = make_ray_inv(o, d);
        cur = 0; sp = 0; k = 0; overflow = false;
    }
    RT_DEV bool next() {
        if (sp != 0) { cur = stack[--sp][lane]; return false; }
        if (overflow) Q.q_exact[atomicAdd(Q.ctr + RQ_CTR_EXACT, 1u)] = slot;
        else Q.pdf[slot] = rq_pdf_nan(wf_merge_light_hits(S, stack, lane, k) / S.n_lights_f);
        return true;
    }
    template <bool COUNT> RT_DEV bool step(WfWalkStat<COUNT> &n) {
        const float4 *q = reinterpret_cast<const float4 *>(S.light_nodes + cur);
        float4 lo0 = q[0], hi0 = q[1], lo1 = q[2], hi1 = q[3];
        n.node();
        float n0, n1;
        bool h0 = slab_test(lo0, hi0, ray, RT_T_MAX, n0);
        bool h1 = slab_test(lo1, hi1, ray, RT_T_MAX, n1);
        uint32_t c0 = __float_as_uint(lo0.w), c1 = __float_as_uint(lo1.w);
        if (h0 & h1) { stack[sp++][lane] = c1; cur = c0; if (sp + 2 * k >= WF_STACK) overflow = true; }
        else if (h0 | h1) cur = h0 ? c0 : c1;
        else return next();
        return false;
    }
    template <bool COUNT> RT_DEV bool leaf(WfWalkStat<COUNT> &n) {
        if (cur != RT_EMPTY_LEAF) {
            uint32_t i = cur & ~RT_LEAF_BIT;
            for (;;) {
                bool last, robust; uint32_t li;
                n.tri();
                float term = pt_light_pdf_one(S, S.lights + i, o, d, last, robust, li);
                if (term != 0.f) {
                    if (!robust || k >= WF_MAX_LIGHT_HITS || sp + 2 * k + 2 >= WF_STACK) overflow = true;
                    else { stack[WF_STACK - 1 - 2 * k][lane] = i; stack[WF_STACK - 2 - 2 * k][lane] = __float_as_uint(term); k++; }
                }
                if (last) break;
                i++;
            }
        }
        return next();
    }
};

__global__ __launch_bounds__(256) void rq_light_kernel(SceneView S, QueryView Q, int refill, int leaf_batch, int dyn) {
    __shared__ uint32_t lds_stack[4][WF_STACK][64];
    RqLightWalk w(S, Q, lds_stack[threadIdx.x >> 6]);
    wf_walk_loop<false>(w, Q.q_fast, wf_slice(Q.ctr[RQ_CTR_FAST], Q.ctr + RQ_CTR_HEAD, dyn, 0u, gridDim.x, true), nullptr, refill, leaf_batch);
}

__global__ __launch_bounds__(64) void rq_light_exact_kernel(SceneView S, QueryView Q) {
    const uint32_t count = Q.ctr[RQ_CTR_EXACT];
    uint32_t stack[RT_STACK_SIZE];
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const uint32_t ray = Q.q_exact[i];
        F3 x, d;
        rq_load_ray(Q, ray, x, d);
        Counters cnt; cnt.closest = cnt.lightq = cnt.nodes = cnt.tris = 0;
        const float v = S.exact_boxes == 1u ? ref_light_pdf_sum(S, x, d, stack) : light_pdf_sum<false>(S, x, d, stack, cnt);
        Q.pdf[ray] = rq_pdf_nan(v / S.n_lights_f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(Q.totals + RQ_TOTAL_EXACT, (unsigned long long)count);
}

// ---- occlusion: is anything in front of tmax? (rt_query_occluded) --------------------------------------------------------------------------
// Bit 0 of a ray's byte: the reference's BVH::intersect reports a hit with t < tmax (strict, float32).  The walk ends at the first
// triangle below the bound instead of looking for the closest, and the gate asks a smaller question than pt_hit_stands:
//   a miss stands     the walkers see a superset of what the reference's box test lets through (padded boxes, pruned only beyond the
//                     bound plus WfClosest's look-behind, so a reference hit in a face of a flat box stays in view); the triangles whose
//                     test accepts points far outside their box are the tripwires', and a ray that crosses one is walked exactly;
//   a hit X stands    when (a) every box above it passes the reference's slab test whatever the rounding (the `worst` and `exit_` terms
//                     of pt_hit_stands), so the reference reaches X unless it pruned X's leaf behind an earlier hit Y, and (b) such a
//                     Y is itself below the bound: the reference prunes only when t_Y < the rounded entry of X's box <= t_X + window
//                     (window = need - min a, rt_exact.h), so tmax - t_X > window puts t_Y < tmax.  Either way the reference ends
//                     with a hit below tmax.  A deep-inside hit has window <= 0 and stands at once.
// The runner-up, the tie tolerance and the `window <= seen` term belong to "which triangle is closest" and play no part.
// Every other ray goes on the exact list: the full closest walk of rq_closest_exact_kernel, compared with tmax (RQ_OCC_EXACT_WALK).
// A ray's tmax: Q.tmax[i], or +inf without the array.  NaN: the ray is invalid.  tmax <= 0: valid, not occluded, never walked.
#define RQ_OCC_OCCLUDED 1u
#define RQ_OCC_EXACT_WALK 2u
#define RQ_OCC_INVALID_RAY 4u

RT_DEV float rq_load_tmax(const QueryView &Q, uint32_t i) { return Q.tmax ? Q.tmax[i] : __uint_as_float(0x7f800000u); }

__global__ __launch_bounds__(256) void rq_classify_occluded_kernel(SceneView S, QueryView Q) {
    __shared__ uint32_t buf_f[WF_BUF], buf_e[WF_BUF];
    __shared__ uint32_t cnt_f, cnt_e, gbase;
    if (threadIdx.x == 0) { cnt_f = 0; cnt_e = 0; }
    __syncthreads();
    Pusher fast; fast.buf = buf_f; fast.cnt = &cnt_f;
    Pusher exact; exact.buf = buf_e; exact.cnt = &cnt_e;
    for (uint32_t base = blockIdx.x * 256u; base < Q.n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        if (i < Q.n) {
            F3 o, d;
            rq_load_ray(Q, i, o, d);
            const float tmax = rq_load_tmax(Q, i);
            const int kind = tmax != tmax ? RQ_INVALID : rq_classify(Q, o, d);
            if (kind == RQ_INVALID) {
                Q.occ[i] = (uint8_t)RQ_OCC_INVALID_RAY;
                atomicAdd(Q.totals + RQ_TOTAL_INVALID, 1ull);
            } else if (!(tmax > 0.f) || S.n_tris == 0u) Q.occ[i] = 0;
            else if (kind == RQ_FAST) wf_push(fast, i);
            else wf_push(exact, i);
        }
        __syncthreads();
        if (cnt_f > WF_BUF - 256) wf_flush(fast, Q.q_fast, Q.ctr + RQ_CTR_FAST, &gbase);
        if (cnt_e > WF_BUF - 256) wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
    }
    __syncthreads();
    wf_flush(fast, Q.q_fast, Q.ctr + RQ_CTR_FAST, &gbase);
    wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
}

// RqTraceWalk's node step and stack; no best hit is kept, so the pruning bound is fixed for the walk: lim = min(tmax, RT_T_MAX) plus the
// look-behind WfClosest gives a best hit at lim.  The record per ray is 8 bytes of Q.rec: t and the hit word, or a miss.
template <bool SPILL> struct RqAnyWalk : WfWalkRay {
    static constexpr int HIST = -1;
    static constexpr bool WAVE_STATS = false;
    const SceneView &S; const QueryView &Q; WfStack<SPILL> stk;
    float tmax = 0.f, lim = 0.f, cull_t = 0.f;
    RT_DEV RqAnyWalk(const SceneView &S_, const QueryView &Q_, const WfView &W_, uint32_t (*stack)[64], int lds_limit) : S(S_), Q(Q_), stk(W_, stack, lds_limit) {}
    RT_DEV void begin(uint32_t item) {
        slot = item;
        rq_load_ray(Q, item, o, d);
        ray = make_ray_inv(o, d);
        cur = 0; sp = 0;
        tmax = rq_load_tmax(Q, item);
        lim = fminf(tmax, RT_T_MAX);
        cull_t = lim + fmaxf(S.cull_k * lim, S.exact_boxes ? pt_look_behind_abs(d, S.box_c2x) : 0.f);
    }
    // One 64-bit store.  As two words the compiler sinks the miss record's second word and next()'s `cur = pop` into one store through a
    // phi of the two addresses, which takes this walker's address: walker and both views then live in scratch (552 B/lane).
    RT_DEV void leave(float t, uint32_t hit) { reinterpret_cast<unsigned long long *>(Q.rec)[slot] = (unsigned long long)hit << 32 | __float_as_uint(t); }
    RT_DEV bool next() {
        if (sp == 0) { leave(0.f, WF_MISS); return true; }
        cur = stk.pop(sp);
        return false;
    }
    template <bool COUNT> RT_DEV bool step(WfWalkStat<COUNT> &n) {
        const float4 *q = reinterpret_cast<const float4 *>(S.nodes + cur);
        float4 lo0 = q[0], hi0 = q[1], lo1 = q[2], hi1 = q[3];
        n.node();
        float n0, n1;
        bool h0 = slab_test(lo0, hi0, ray, cull_t, n0);
        bool h1 = slab_test(lo1, hi1, ray, cull_t, n1);
        uint32_t c0 = __float_as_uint(lo0.w), c1 = __float_as_uint(lo1.w);
        if (h0 & h1) {
            bool swap = n1 < n0;
            stk.push(sp, swap ? c0 : c1);
            cur = swap ? c1 : c0;
        } else {
            cur = h0 ? c0 : c1;
            if (!(h0 | h1)) return next();
        }
        return false;
    }
    template <bool COUNT> RT_DEV bool leaf(WfWalkStat<COUNT> &n) {
        if (cur != RT_EMPTY_LEAF) {
            uint32_t i = cur & ~RT_LEAF_BIT;
            for (;;) {
                TriIsect T = load_isect(S.tri_walk + i);
                n.tri();
                float t, u, v; bool inside;
                if (tri_test_closer(T, o, d, lim, t, u, v, inside) && t < tmax) { // the walk ends here, whatever its stack still holds
                    leave(t, (T.pad >> 1) | (inside ? WF_INSIDE_BIT : 0u));
                    return true;
                }
                if (T.pad & 1u) break;
                i++;
            }
        }
        return next();
    }
};

template <bool SPILL>
__global__ __launch_bounds__(256) void rq_any_kernel(SceneView S, QueryView Q, int refill, int leaf_batch, int dyn, int lds_limit) {
    __shared__ uint32_t lds_stack[4][WF_STACK][64];
    WfView W{};
    W.ovf = Q.ovf;
    RqAnyWalk<SPILL> w(S, Q, W, lds_stack[threadIdx.x >> 6], lds_limit);
    wf_walk_loop<false>(w, Q.q_fast, wf_slice(Q.ctr[RQ_CTR_FAST], Q.ctr + RQ_CTR_HEAD, dyn, 0u, gridDim.x, true), nullptr, refill, leaf_batch);
}

__global__ __launch_bounds__(256) void rq_any_resolve_kernel(SceneView S, QueryView Q) {
    __shared__ uint32_t buf[WF_BUF];
    __shared__ uint32_t cnt, gbase;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    Pusher exact; exact.buf = buf; exact.cnt = &cnt;
    const uint32_t count = Q.ctr[RQ_CTR_FAST];
    for (uint32_t base = blockIdx.x * 256u; base < count; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        if (i < count) {
            const uint32_t ray = Q.q_fast[i];
            const float2 r = reinterpret_cast<const float2 *>(Q.rec)[ray];
            const uint32_t hit = __float_as_uint(r.y);
            bool stands = true;
            if (S.exact_boxes) {
                F3 o, d;
                rq_load_ray(Q, ray, o, d);
                if (S.n_tripwire_groups && pt_tripwire(S, o, d)) stands = false;
                else if (hit != WF_MISS) {
                    const float4 *bx = reinterpret_cast<const float4 *>(S.tri_box) + 2 * (size_t)(hit & WF_INDEX_MASK);
                    const float4 lo = bx[0], hi = bx[1];
                    stands = rq_any_hit_stands(f3(lo.x, lo.y, lo.z), f3(hi.x, hi.y, hi.z), o, d, r.x, rq_load_tmax(Q, ray), S.box_c2);
                }
            }
            if (stands) Q.occ[ray] = (uint8_t)(hit != WF_MISS ? RQ_OCC_OCCLUDED : 0u);
            else wf_push(exact, ray);
        }
        __syncthreads();
        if (cnt > WF_BUF - 256) wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
    }
    __syncthreads();
    wf_flush(exact, Q.q_exact, Q.ctr + RQ_CTR_EXACT, &gbase);
}

// The exact list: rq_closest_exact_kernel's walk, left as the full closest walk (it is the referee, and rare), its t compared with tmax.
__global__ __launch_bounds__(64) void rq_any_exact_kernel(SceneView S, QueryView Q) {
    const uint32_t count = Q.ctr[RQ_CTR_EXACT];
    uint32_t stack[RT_STACK_SIZE];
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const uint32_t ray = Q.q_exact[i];
        F3 o, d;
        rq_load_ray(Q, ray, o, d);
        float bt, bu, bv; uint32_t hit;
        if (S.exact_boxes == 1u) ref_closest_hit(S, o, d, stack, bt, bu, bv, hit);
        else {
            Counters cnt; cnt.closest = cnt.lightq = cnt.nodes = cnt.tris = 0;
            const HitRec h = closest_hit<false>(S, o, d, stack, cnt);
            bt = h.t;
            hit = h.idx < 0 ? WF_MISS : (uint32_t)h.idx;
        }
        Q.occ[ray] = (uint8_t)(RQ_OCC_EXACT_WALK | (hit != WF_MISS && bt < rq_load_tmax(Q, ray) ? RQ_OCC_OCCLUDED : 0u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(Q.totals + RQ_TOTAL_EXACT, (unsigned long long)count);
}

} // namespace dev
} // namespace rtamd

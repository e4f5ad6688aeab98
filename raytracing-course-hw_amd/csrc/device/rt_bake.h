// The light-map and probe baker under the C-ABI (include/rtamd.h: rt_bake_rays, rt_bake): the first caller of the query layer, kept a
// composition of its public calls.  Per sample of a slot: a ray from the slot's engine (rq_bake_make_ray), rt_trace_paths' rounds over
// it -- the launches of rt_query.h, rt_query_surface.h and rt_query_scatter.h, untouched -- then the fold, the accumulation and the
// slot's next ray from the engine as the scatter left it.  No kernel here walks a tree.
//
//   rq_bake_rays_kernel     one lane per record: classify, then o = p + eps * n, d = cosine_sample (irradiance) or o = p, d = a uniform
//                           direction (SH9).  rt_bake starts a chunk with it (BakeView::left set): accumulators zeroed, samples left = q.
//   rq_bake_advance_kernel  one lane per slot after a round's queries: rq_path_advance_kernel's end-or-keep step; where the slot's path is
//                           over -- at once, or under RT_BAKE_LOCKSTEP in the round that spends the depth -- fold, accumulate, make the
//                           next ray and reset the path state, or park the slot as an invalid ray when no sample is left.
//   rq_bake_resolve_kernel  one lane per float of the answer: the sum over a point's streams in order, times the scale; an invalid
//                           point answers zeros.
//
// A record is classified before any dependent work: a NaN or an infinity in p, (irradiance) in n, n == 0, or an engine state outside
// 1 .. 2^31-2 in any of the point's streams makes the point invalid; it draws nothing, its engines stay, it rides along as an invalid
// ray.  Nothing is indexed by a caller's word.  One lane owns a slot: no float atomics; the counters are integer atomicAdds, one per wave.
#pragma once
#include "rt_query_scatter.h"

namespace rtamd {
namespace dev {

#define RQ_BAKE_IRRADIANCE 0
#define RQ_BAKE_SH9 1

// ctr[which] += the number of active lanes with `flag`, one atomic per wave.  Every active lane of the wave calls it.
RT_DEV void rq_bake_count(unsigned long long *ctr, int which, bool flag) {
    const unsigned long long mask = __ballot(flag);
    if (flag && (uint32_t)(__ffsll((long long)mask) - 1) == (threadIdx.x & 63u)) atomicAdd(ctr + which, (unsigned long long)__popcll(mask));
}

// Point `point` of `points` and whether its numbers are valid (its engines: rq_bake_point); n is read in irradiance mode only.  Shared with
// the path source of the persistent kernel (rt_path_source.h).
RT_DEV bool rq_bake_point_read(const float *points, uint32_t point, int32_t mode, F3 &p, F3 &n) {
    const float *q = points + 6 * (size_t)point;
    p = f3(q[0], q[1], q[2]);
    n = f3(0.f, 0.f, 0.f);
    bool ok = rq_finite(p.x) && rq_finite(p.y) && rq_finite(p.z);
    if (mode == RQ_BAKE_IRRADIANCE) {
        n = f3(q[3], q[4], q[5]);
        ok = ok && rq_valid_ray(p, n);                       // finite, and n != 0
    }
    return ok;
}
// The point of record i and whether it is valid.
RT_DEV bool rq_bake_point(const BakeView &B, uint32_t i, F3 &p, F3 &n) {
    const uint32_t point = i / B.streams;
    bool ok = rq_bake_point_read(B.points, point, B.mode, p, n);
    const uint4 *e = B.rng + (size_t)point * B.streams;
    for (uint32_t k = 0; k < B.streams; k++) ok = ok && rq_rng_valid(e[k].x);
    return ok;
}

// The ray (o, d) of one sample at a point, drawn from `rng`, which advances: the one place these expressions stand (rq_bake_make_ray below,
// PtSource of rt_path_source.h).
RT_DEV void rq_bake_ray(int32_t mode, Rng &rng, F3 p, F3 n, F3 &o, F3 &d) {
    if (mode == RQ_BAKE_IRRADIANCE) {
        o = p + RQ_EPS * n;
        d = cosine_sample(rng, n);
    } else {
        float a, b, c;
        rng_n01x3(rng, a, b, c);                             // cosine_sample's first line: a uniform direction
        o = p;
        d = normalize(f3(a, b, c));
    }
}
// ... from the slot's engine record, which is written back as the scatter writes it.
RT_DEV void rq_bake_make_ray(const BakeView &B, uint32_t i, F3 p, F3 n, float *ray) {
    const uint4 e = B.rng[i];                                // x saved has_saved reserved
    Rng rng; rng.x = e.x; rng.saved = __uint_as_float(e.y); rng.has_saved = e.z != 0u;
    F3 o, d;
    rq_bake_ray(B.mode, rng, p, n, o, d);
    B.rng[i] = make_uint4(rng.x, rng.has_saved ? __float_as_uint(rng.saved) : 0u, rng.has_saved ? 1u : 0u, e.w);
    rq_store_ray(ray, o, d);
    if (B.dir0) { float *q = B.dir0 + 3 * (size_t)i; q[0] = d.x; q[1] = d.y; q[2] = d.z; }
}

__global__ __launch_bounds__(256) void rq_bake_rays_kernel(SceneView S, BakeView B) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < B.n; i += gridDim.x * 256u) {
        F3 p, n;
        const bool ok = rq_bake_point(B, i, p, n);
        float *ray = B.rays + 6 * (size_t)i;
        if (B.left) {                                        // rt_bake: the slot's state at the start of a chunk
            for (uint32_t j = 0; j < B.floats; j++) B.acc[(size_t)j * B.n + i] = 0.f;
            B.left[i] = ok ? B.per_stream : 0u;
            rq_bake_count(B.ctr, RQ_BAKE_CTR_SLOTS, ok);
            rq_bake_count(B.ctr, RQ_BAKE_CTR_INVALID_POINTS, !ok && i % B.streams == 0u);
        } else if (!ok) atomicAdd(B.totals + RQ_TOTAL_INVALID, 1ull);
        if (!ok) { rq_store_no_ray(ray); continue; }
        rq_bake_make_ray(B, i, p, n, ray);
    }
}

// acc_k += L (irradiance) or acc_k[m][c] = acc_k[m][c] + (Y_m(d) * L[c]) with d the sample's first direction (SH9).
RT_DEV void rq_bake_accumulate(const BakeView &B, uint32_t i, F3 L) {
    float *a = B.acc + i;
    const size_t n = B.n;
    const float Lc[3] = {L.x, L.y, L.z};
    if (B.mode == RQ_BAKE_IRRADIANCE) {
        for (int c = 0; c < 3; c++) a[c * n] = a[c * n] + Lc[c];
        return;
    }
    const float *q = B.dir0 + 3 * (size_t)i;
    const float x = q[0], y = q[1], z = q[2];
    const float Y[9] = {0.282095f, 0.488603f * y, 0.488603f * z, 0.488603f * x, 1.092548f * (x * y), 1.092548f * (y * z),
                        0.315392f * ((3.0f * (z * z)) - 1.0f), 1.092548f * (x * z), 0.546274f * ((x * x) - (y * y))};
    for (int m = 0; m < 9; m++)
        for (int c = 0; c < 3; c++) a[(size_t)(3 * m + c) * n] = a[(size_t)(3 * m + c) * n] + (Y[m] * Lc[c]);
}

__global__ __launch_bounds__(256) void rq_bake_advance_kernel(SceneView S, PathView V, BakeView B) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        uint32_t left = B.left[i];
        if (!left) continue;                                 // parked: an invalid point, or every sample of the slot is in
        float4 st = V.state[i];
        uint32_t word = __float_as_uint(st.w);
        float *ray = V.rays + 6 * (size_t)i;
        const bool live = !(word & RQ_PATH_ENDED);           // this round's closest-hit query was one of a live path
        rq_bake_count(B.ctr, RQ_BAKE_CTR_LIVE_RAY_SLOTS, live);
        if (live) {
            F3 tail;
            rq_path_end_or_keep(S, V, i, ray, word, tail);
            st = make_float4(tail.x, tail.y, tail.z, __uint_as_float(word));
        }
        const bool over = B.lockstep ? B.last != 0u : (word & RQ_PATH_ENDED) != 0u || (word & 0xFFu) == B.depth;
        if (!over) {
            if (live) V.state[i] = st;
            continue;
        }
        rq_bake_accumulate(B, i, rq_path_fold(V, i, word, f3(st.x, st.y, st.z)));
        left--;
        B.left[i] = left;
        if (left) {                                          // the slot's next sample, from the engine as the scatter left it
            F3 p, n;
            rq_bake_point(B, i, p, n);
            rq_bake_make_ray(B, i, p, n, ray);
            V.state[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            rq_store_no_ray(ray);
            V.state[i] = make_float4(0.f, 0.f, 0.f, __uint_as_float(RQ_PATH_ENDED));
        }
        rq_bake_count(B.ctr, RQ_BAKE_CTR_PARKED, left == 0u);
    }
}

// scale * (((a_0 + a_1) + a_2) ...) over the `streams` sums of a point, `stride` floats apart; the bits as the answer keeps them.  Shared with
// rq_source_unpack_kernel (rt_path_source.h), whose sums lie in the slots' state.
RT_DEV uint32_t rq_bake_stream_sum(const float *a, size_t stride, uint32_t streams, float scale) {
    float sum = a[0];
    for (uint32_t k = 1; k < streams; k++) sum = sum + a[k * stride];
    return rq_bits(scale * sum);
}
// out[point][j] = scale * (((acc_0 + acc_1) + acc_2) ...) over the point's streams; B.n counts the floats of the chunk's answer.
__global__ __launch_bounds__(256) void rq_bake_resolve_kernel(SceneView S, BakeView B) {
    const uint32_t slots = B.n / B.floats * B.streams;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < B.n; t += gridDim.x * 256u) {
        const uint32_t point = t / B.floats, j = t % B.floats;
        uint32_t *out = reinterpret_cast<uint32_t *>(B.out) + t;
        F3 p, n;
        if (!rq_bake_point(B, point * B.streams, p, n)) { *out = 0u; continue; }
        const float *a = B.acc + (size_t)j * slots + (size_t)point * B.streams;
        *out = rq_bake_stream_sum(a, 1u, B.streams, B.scale);
    }
}

} // namespace dev
} // namespace rtamd

// The path source of the persistent hw8 kernel (include/rtamd.h: rt_render_paths, rt_render_bake): rt_render, rt_trace_paths and rt_bake
// differ in where a sample's first ray comes from and where a slot's sum and engine go when it has no sample left.  A kernel compiled
// with WF_FEAT_SOURCE takes the first ray from RenderView::src_* instead of the camera,
//   src_mode 1   the caller's ray src_rays[gslot], used as given (not normalised); the engine does not advance for it; one sample per slot
//   src_mode 2   rq_bake_ray (rt_bake.h) on point gslot / src_streams, drawn from the slot's engine; `samples` samples per slot
// and keeps sum, engine and end of slot as a resumable render has them (RenderView::accum, 24 bytes per slot): the slice of a resumable
// frame whose pixel slots are the record indices.  A kernel with the bit is only ever launched with src_mode 1 or 2.
//
// SH9 probes (include/rtamd.h: rt_render_probes) are a kernel of their own, compiled with WF_FEAT_SOURCE | WF_FEAT_PROBES and only ever
// launched with
//   src_mode 3   rq_bake_ray(RQ_BAKE_SH9) on point gslot / src_streams: o = p, d = a uniform direction; `samples` samples per slot
// so that the kernels of modes 1 and 2 hold no branch for it.  What does not fit the path record lives in RenderView::src_sh, 30 floats
// (120 bytes) per slot: the first direction of the sample in flight, then the 27 accumulators [m][c].  PtSource::first / ::ray store the
// direction they draw; PtSource::sample, called by wf_finish_path between the fold and wf_end_sample (which draws the next sample's ray
// and so overwrites the direction), adds Y_m(d0) * L[c] with rq_bake_accumulate's expressions.  The slot's rgb sum and its way back to
// the state are as in mode 2; the sum is simply not the answer.
// Layout: slot-major, not plane-major as rt_bake's `acc`.  rt_bake's advance kernel has lane i on slot i, so a plane is read in whole
// lines.  Here a shader lane holds whatever path it popped, its neighbours' slots are unrelated, and no layout makes a wave's access
// contiguous: slot-major keeps a lane's 120 bytes within two 128-byte lines where plane-major would touch 30.  120 is a multiple of 8,
// so the lane moves them as fifteen 8-byte words.  One lane owns a slot from its first ray to its last sample: no atomics.
//
// The pixels of another frame (include/rtamd.h: rt_adaptive_*) are a kernel of their own too, compiled with WF_FEAT_SOURCE |
// WF_FEAT_PIXELS and only ever launched with
//   src_mode 4   wf_camera_ray's expressions for pixel src_pixels[gslot] = x | y << 16 of the frame src_frame[0] x src_frame[1] with
//                src_tan_fov_x, drawn from the slot's engine; `samples` samples per slot
// The strip's slots are the pixel slots of the active 8x8 sub-tiles of that frame, gathered by ad_gather_kernel (rt_adaptive.h), which
// also works the pixel out, so that no division on the real geometry runs here.  A slot whose engine word is 0 is the padding of a
// border sub-tile (accum_seed_kernel) or lies beyond the list: it starts no path and is NOT counted, as padding never was.  Its rays
// are camera rays, which the walkers were derived for: the shader looks at the tripwires only, as the camera kernels' seed_wire does
// (rt_persistent.h), not at pt_source_exact.  The pixels are the same either way (the exact role and the walkers agree on every ray
// the gate lets the walkers keep); the camera kernels' rule is the cheaper one and the one rt_render itself runs.
//
// A batch of cameras over one scene (include/rtamd.h: rt_views_*) is the fifth kernel, compiled with WF_FEAT_SOURCE | WF_FEAT_VIEWS and only
// ever launched with
//   src_mode 5   wf_camera_ray's expressions for pixel src_pixels[gslot] = x | y << 16 of a frame of src_wh = width | height << 16 pixels,
//                the camera's values from record src_cameras[v], v = src_pixels[src_n + gslot / 64] the view behind the slot's 64-slot
//                group (src_n is a multiple of 64); drawn from the slot's engine; `samples` samples per slot
// The strip's slots are the pixel slots of the active views' 8x8 sub-tiles, gathered by vw_gather_kernel (rt_views.h), which works pixel
// and view out.  Padding is an engine word of 0 as in mode 4.  The record is read for every first ray, 64 bytes as four 16-byte words,
// and is dead once the ray is in the path record: no camera lives in registers across the path.  A view's camera may lie anywhere, so
// UNLIKE mode 4 this source keeps pt_source_exact for every first ray: a camera outside the node grid or beyond the origin bound
// sends its rays to the exact role, one inside both takes the walkers as the scene's own camera does.
//
// The frame.  An unsharded strip 8 pixels wide and 8 * ceil(n / 64) high: its tiles are the 8x8 sub-tiles themselves, one per row of the
// tile grid, so slot_to_pixel (rt_device.h) maps sub-tile s, pixel (x, y) of it to slot 64 s + 8 y + x -- gslot IS the record index.  The
// pixel coordinates are never used (no camera ray, no pixel store).
//
// A slot with no path: gslot >= src_n, or a record the composed calls refuse (rt_trace_paths: rq_valid_ray, rq_rng_valid; rt_bake:
// rq_bake_point -- a point's numbers and ALL of its streams' engines).  It starts no path, its state is not touched, and it is counted
// in CNT_SRC_NO_PATH (mode 1: every such record below src_n; mode 2: once per point, by its first slot).
//
// First rays the walkers were not derived for (pt_source_exact) belong to the exact role from the start: an origin outside the 16-bit
// node grid (rt_device.h RayGrid: its error budget holds for |o'| <= 65,536 cells), a ray off the fast list of rt_query.h (rq_classify),
// or one that pierces a tripwire.  Bounce rays start on surfaces and are the render's own.
//
//   rq_source_pack_kernel    one lane per slot: the caller's rt_rng -> the slot's state, sum 0 (a slot beyond n: zeros, which is no engine)
//   rq_source_unpack_kernel  one lane per slot: state -> rt_rng (saved = 0 whenever has_saved is 0, `reserved` handed through; an invalid
//                            record's engine is not written) and the answer: the slot's sum (mode 1) or rq_bake_stream_sum over the
//                            point's slots (mode 2, by the point's first slot), through rq_bits; an invalid record answers zeros
#pragma once
#include "rt_bake.h"

namespace rtamd {
namespace dev {

#define PT_SRC_CAMERA 0u
#define PT_SRC_RAYS 1u
#define PT_SRC_BAKE 2u
#define PT_SRC_PROBES 3u
#define PT_SRC_PIXELS 4u
#define PT_SRC_VIEWS 5u
#define PT_SH_FLOATS 30u // per slot of RenderView::src_sh: d0.xyz, then acc[9][3]

RT_DEV void pt_source_load_ray(const float *rays, uint32_t i, F3 &o, F3 &d) { // rt_ray is only 4-byte aligned
    const float *p = rays + 6 * (size_t)i;
    o = f3(p[0], p[1], p[2]); d = f3(p[3], p[4], p[5]);
}
// The engine word of slot j in the state of a resumable render (accum_enter's layout).
RT_DEV uint32_t pt_source_engine(const uint32_t *state, uint32_t j) { return state[4 * (size_t)j + 3]; }
// Mode 2: the point of slot `gslot` and whether it is valid.  The engines of the point's other slots are read from the state while those
// slots may be running: a valid engine stays one however far it has advanced, and an invalid one is never written.
template <int32_t MODE> RT_DEV bool pt_source_point(const RenderView &R, uint32_t gslot, F3 &p, F3 &n) {
    const uint32_t point = gslot / R.src_streams;
    bool ok = rq_bake_point_read(R.src_points, point, MODE, p, n);
    for (uint32_t k = 0; k < R.src_streams; k++) ok = ok && rq_rng_valid(pt_source_engine(R.accum, point * R.src_streams + k));
    return ok;
}
// Whether a slot without a path counts (once per invalid record / point; the padding of the last 64-slot group does not).
template <int FEAT> RT_DEV bool pt_source_counts(const RenderView &R, uint32_t gslot) {
    if constexpr ((FEAT & (WF_FEAT_PIXELS | WF_FEAT_VIEWS)) != 0) return false; // mode 4 and 5: a slot without a path is padding
    if constexpr ((FEAT & WF_FEAT_PROBES) != 0) return gslot < R.src_n && gslot % R.src_streams == 0u;
    else return gslot < R.src_n && (R.src_mode != PT_SRC_BAKE || gslot % R.src_streams == 0u);
}
// Whether the first ray (o, d) of a sample goes to the exact role (PT_Q_XTRACE) instead of the walkers.  Too cautious costs speed only.
RT_DEV bool pt_source_exact(const SceneView &S, F3 o, F3 d) {
    QueryView Q{};
    Q.origin_bound = S.box_c2 * 1048576.f;                  // as rtamd_query.hip's walk_view sets it
    if (rq_classify(Q, o, d) != RQ_FAST) return true;
    const NodeGrid &G = S.grid;
    const float cx = (o.x - G.lo[0]) * G.istep[0], cy = (o.y - G.lo[1]) * G.istep[1], cz = (o.z - G.lo[2]) * G.istep[2];
    if (!(cx >= 0.f && cx <= 65536.f && cy >= 0.f && cy <= 65536.f && cz >= 0.f && cz <= 65536.f)) return true;
    return pt_tripwire(S, o, d);
}

// Mode 3: the slot's first direction, and a finished sample's value L projected onto the nine basis functions at that direction:
// acc[m][c] = acc[m][c] + (Y_m(d0) * L[c]), the Y_m spelled as rq_bake_accumulate (rt_bake.h) spells them.
RT_DEV void pt_source_store_dir(const RenderView &R, uint32_t gslot, F3 d) {
    float *s = R.src_sh + (size_t)PT_SH_FLOATS * gslot;
    *reinterpret_cast<float2 *>(s) = make_float2(d.x, d.y);
    s[2] = d.z;
}
RT_DEV void pt_source_project(const RenderView &R, uint32_t gslot, F3 L) {
    float2 *s = reinterpret_cast<float2 *>(R.src_sh + (size_t)PT_SH_FLOATS * gslot);
    float v[PT_SH_FLOATS];
#pragma unroll
    for (int j = 0; j < (int)PT_SH_FLOATS / 2; j++) { const float2 w = s[j]; v[2 * j] = w.x; v[2 * j + 1] = w.y; }
    const float x = v[0], y = v[1], z = v[2];
    const float Lc[3] = {L.x, L.y, L.z};
    const float Y[9] = {0.282095f, 0.488603f * y, 0.488603f * z, 0.488603f * x, 1.092548f * (x * y), 1.092548f * (y * z),
                        0.315392f * ((3.0f * (z * z)) - 1.0f), 1.092548f * (x * z), 0.546274f * ((x * x) - (y * y))};
#pragma unroll
    for (int m = 0; m < 9; m++)
#pragma unroll
        for (int c = 0; c < 3; c++) v[3 + 3 * m + c] = v[3 + 3 * m + c] + (Y[m] * Lc[c]);
#pragma unroll
    for (int j = 1; j < (int)PT_SH_FLOATS / 2; j++) s[j] = make_float2(v[2 * j], v[2 * j + 1]); // word 1 holds d0.z next to acc[0][0]: rewritten as read
}

// Mode 4: the camera ray of the real frame's pixel behind strip slot `gslot`.
RT_DEV void pt_source_pixel_ray(const SceneView &S, const RenderView &R, uint32_t gslot, Rng &rng, F3 &o, F3 &d) {
    const uint32_t xy = R.src_pixels[gslot];
    wf_camera_ray_of(S, R.src_tan_fov_x, R.src_frame[0], R.src_frame[1], rng, (int)(xy & 0xffffu), (int)(xy >> 16), o, d);
}

// Mode 5: the ray of the camera of the slot's view through the pixel behind strip slot `gslot`.
RT_DEV void pt_source_view_ray(const RenderView &R, uint32_t gslot, Rng &rng, F3 &o, F3 &d) {
    const uint32_t xy = R.src_pixels[gslot], view = R.src_pixels[R.src_n + (gslot >> 6)];
    const float4 *c = reinterpret_cast<const float4 *>(R.src_cameras + view);
    const float4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3]; // pos.xyz right.x | right.yz up.xy | up.z fwd.xyz | tan_fov_x tan_fov_y
    wf_camera_ray_from(f3(c0.x, c0.y, c0.z), f3(c0.w, c1.x, c1.y), f3(c1.z, c1.w, c2.x), f3(c2.y, c2.z, c2.w), c3.x, c3.y,
                       (int)(R.src_wh & 0xffffu), (int)(R.src_wh >> 16), rng, (int)(xy & 0xffffu), (int)(xy >> 16), o, d);
}

template <int FEAT> struct PtSource {
    // The first ray of slot `gslot`, whose engine `rng` comes from the state; false: the slot has no path.
    static RT_DEV bool first(const SceneView &S, const RenderView &R, uint32_t gslot, Rng &rng, F3 &o, F3 &d) {
        if (gslot >= R.src_n) return false;
        if constexpr ((FEAT & WF_FEAT_VIEWS) != 0) {
            if (!rq_rng_valid(rng.x)) return false;          // engine word 0: padding of a border sub-tile
            pt_source_view_ray(R, gslot, rng, o, d);
            return true;
        }
        if constexpr ((FEAT & WF_FEAT_PIXELS) != 0) {
            if (!rq_rng_valid(rng.x)) return false;          // engine word 0: padding of a border sub-tile
            pt_source_pixel_ray(S, R, gslot, rng, o, d);
            return true;
        }
        if constexpr ((FEAT & WF_FEAT_PROBES) != 0) {
            F3 p, n;
            if (!pt_source_point<RQ_BAKE_SH9>(R, gslot, p, n)) return false;
            rq_bake_ray(RQ_BAKE_SH9, rng, p, n, o, d);
            pt_source_store_dir(R, gslot, d);
            return true;
        }
        if (R.src_mode == PT_SRC_BAKE) {
            F3 p, n;
            if (!pt_source_point<RQ_BAKE_IRRADIANCE>(R, gslot, p, n)) return false;
            rq_bake_ray(RQ_BAKE_IRRADIANCE, rng, p, n, o, d);
            return true;
        }
        pt_source_load_ray(R.src_rays, gslot, o, d);
        return rq_valid_ray(o, d) && rq_rng_valid(rng.x);
    }
    // The first ray of the slot's sample `next` (wf_finish_path): the slot has a path, so its record is valid.
    static RT_DEV void ray(const SceneView &S, const RenderView &R, Rng &rng, uint32_t gslot, int x, int y, uint32_t next, F3 &o, F3 &d) {
        if constexpr ((FEAT & WF_FEAT_VIEWS) != 0) {
            pt_source_view_ray(R, gslot, rng, o, d);
        } else if constexpr ((FEAT & WF_FEAT_PIXELS) != 0) {
            pt_source_pixel_ray(S, R, gslot, rng, o, d);
        } else if constexpr ((FEAT & WF_FEAT_PROBES) != 0) {
            F3 p, n;
            rq_bake_point_read(R.src_points, gslot / R.src_streams, RQ_BAKE_SH9, p, n);
            rq_bake_ray(RQ_BAKE_SH9, rng, p, n, o, d);
            pt_source_store_dir(R, gslot, d);
        } else if constexpr ((FEAT & WF_FEAT_SOURCE) != 0) {
            if (R.src_mode == PT_SRC_BAKE) {
                F3 p, n;
                rq_bake_point_read(R.src_points, gslot / R.src_streams, RQ_BAKE_IRRADIANCE, p, n);
                rq_bake_ray(RQ_BAKE_IRRADIANCE, rng, p, n, o, d);
            } else pt_source_load_ray(R.src_rays, gslot, o, d); // (mode 1 has one sample per slot: never reached)
        } else WfCameraSource::ray(S, R, rng, gslot, x, y, next, o, d);
    }
    // The value of the slot's finished sample, before ray() draws the next one.
    static RT_DEV void sample(const RenderView &R, uint32_t gslot, F3 L) {
        if constexpr ((FEAT & WF_FEAT_PROBES) != 0) pt_source_project(R, gslot, L);
    }
};

__global__ __launch_bounds__(256) void rq_source_pack_kernel(SourceView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n_pixslots; i += gridDim.x * 256u) {
        const uint4 e = i < V.n ? V.rng[i] : make_uint4(0u, 0u, 0u, 0u); // x saved has_saved reserved
        reinterpret_cast<uint4 *>(V.state)[i] = make_uint4(0u, 0u, 0u, e.x);
        reinterpret_cast<uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[i] = make_uint2(e.y, e.z != 0u ? 1u : 0u);
    }
}

__global__ __launch_bounds__(256) void rq_source_unpack_kernel(SourceView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const uint4 a = reinterpret_cast<const uint4 *>(V.state)[i];
        const uint2 b = reinterpret_cast<const uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[i];
        bool ok;
        if (V.mode == PT_SRC_BAKE) {
            BakeView B{};
            B.points = V.points; B.rng = V.rng; B.streams = V.streams; B.mode = RQ_BAKE_IRRADIANCE;
            F3 p, n;
            ok = rq_bake_point(B, i, p, n);                  // the caller's engines: written below by other lanes, valid before and after
            if (i % V.streams == 0u) {
                uint32_t *out = reinterpret_cast<uint32_t *>(V.out) + 3 * (size_t)(i / V.streams);
                const float *sums = reinterpret_cast<const float *>(V.state) + 4 * (size_t)i;
                for (int j = 0; j < 3; j++) out[j] = ok ? rq_bake_stream_sum(sums + j, 4u, V.streams, V.scale) : 0u;
            }
        } else {
            F3 o, d;
            pt_source_load_ray(V.rays, i, o, d);
            ok = rq_valid_ray(o, d) && rq_rng_valid(a.w);
            uint32_t *out = reinterpret_cast<uint32_t *>(V.out) + 3 * (size_t)i;
            out[0] = rq_bits(__uint_as_float(a.x)); out[1] = rq_bits(__uint_as_float(a.y)); out[2] = rq_bits(__uint_as_float(a.z)); // an invalid record's sum is the 0 it was packed with
        }
        if (ok) V.rng[i] = make_uint4(a.w, b.y ? b.x : 0u, b.y ? 1u : 0u, V.rng[i].w);
    }
}

// Mode 3, siblings of the two kernels above (which stay the code they were):
//   rq_probes_pack_kernel    rq_source_pack_kernel's engines and sums, then zeros over the chunk's src_sh in whole 8-byte words
//   rq_probes_unpack_kernel  one lane per slot: the engine back, as above; then one lane per float of the answer, as rq_bake_resolve_kernel:
//                            out[point][j] = rq_bake_stream_sum over accumulator j of the point's K slots, zeros for an invalid point.
//                            Validity is read from the caller's engines while other lanes write them back: valid before and after.
__global__ __launch_bounds__(256) void rq_probes_pack_kernel(SourceView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n_pixslots; i += gridDim.x * 256u) {
        const uint4 e = i < V.n ? V.rng[i] : make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4 *>(V.state)[i] = make_uint4(0u, 0u, 0u, e.x);
        reinterpret_cast<uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[i] = make_uint2(e.y, e.z != 0u ? 1u : 0u);
    }
    const size_t words = (size_t)V.n_pixslots * (PT_SH_FLOATS / 2u);
    for (size_t w = blockIdx.x * 256u + threadIdx.x; w < words; w += (size_t)gridDim.x * 256u) reinterpret_cast<float2 *>(V.sh)[w] = make_float2(0.f, 0.f);
}

__global__ __launch_bounds__(256) void rq_probes_unpack_kernel(SourceView V) {
    BakeView B{};
    B.points = V.points; B.rng = V.rng; B.streams = V.streams; B.mode = RQ_BAKE_SH9;
    F3 p, n;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const uint4 a = reinterpret_cast<const uint4 *>(V.state)[i];
        const uint2 b = reinterpret_cast<const uint2 *>(V.state + 4 * (size_t)V.n_pixslots)[i];
        if (rq_bake_point(B, i, p, n)) V.rng[i] = make_uint4(a.w, b.y ? b.x : 0u, b.y ? 1u : 0u, V.rng[i].w);
    }
    const uint32_t floats = V.n / V.streams * 27u;           // below 2^31: a chunk has at most 2,073,600 slots
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < floats; t += gridDim.x * 256u) {
        const uint32_t point = t / 27u, j = t % 27u;
        uint32_t *out = reinterpret_cast<uint32_t *>(V.out) + t;
        if (!rq_bake_point(B, point * V.streams, p, n)) { *out = 0u; continue; }
        *out = rq_bake_stream_sum(V.sh + (size_t)PT_SH_FLOATS * point * V.streams + 3u + j, PT_SH_FLOATS, V.streams, V.scale);
    }
}

} // namespace dev
} // namespace rtamd

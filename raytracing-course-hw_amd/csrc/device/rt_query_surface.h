// The first-hit layer over the batched ray queries (include/rtamd.h: rt_query_surface, rt_query_environment, rt_camera_rays,
// rt_render_guides): what Scene::getColor knows about a hit before it samples a direction (hw8/src/scene.cpp:99-149), what a ray that
// misses sees (:90-97), the ray Scene::getCameraRay shoots through a point of the image plane (:179-186), and the three composed into
// guide images.  No kernel here walks a tree: the hits come from rt_query.h's launches.
//
//   rq_material_table_kernel  once per scene: the material index of every triangle in LOAD order (TriShade is in figure order)
//   rq_surface_kernel         one lane per rt_hit: 64 bytes in, 64 bytes out, the texture taps and the normal map in between
//   rq_environment_kernel     one lane per ray: miss_color for the direction as given
//   rq_camera_rays_kernel     one lane per ray: wf_camera_ray's expressions for a point (nx, ny) of the caller's, or the pixel centres
//   rq_guides_kernel          one lane per pixel of a chunk: hit, surface and ray into the planes
//
// The surface is shade_fetch_attr's second half (rt_kernels_hw8.h) with the same device functions: the material's three quads, the four
// image descriptors together, sample_texture, apply_normal_map, smax(0.08f, .) squared.  Its first half -- the interpolation at (u, v) --
// is what rq_write_hit left in the rt_hit, so the record stands in for the ray: texcoord, ns (already flipped towards the ray's side)
// and tangent are taken from it as they are, and a caller may have altered them.  What is read through the record is classified
// before any dependent load, as rq_classify treats rays: a triangle index beyond the scene or a non-finite attribute answers the blank
// record and is counted; a miss answers the blank record.  With finite texture coordinates sample_texture stays inside its image
// (load_texel answers the one texel past the last row with 0), and the material and image indices were checked at scene preparation.
#pragma once
#include "rt_query.h"

namespace rtamd {
namespace dev {

#define RQ_NO_TRIANGLE 0xFFFFFFFFu

__global__ __launch_bounds__(256) void rq_material_table_kernel(SceneView S, uint32_t *table) {
    const uint32_t fig = blockIdx.x * 256u + threadIdx.x;
    if (fig >= S.n_tris) return;
    const float4 s6 = reinterpret_cast<const float4 *>(S.tri_shade + fig)[6]; // tanw material orig pad
    const uint32_t orig = __float_as_uint(s6.z);
    if (orig < S.n_tris) table[orig] = __float_as_uint(s6.y);
}

// One rt_surface: color.xyz alpha | emission.xyz metallic | sn.xyz material | base_color.xyz base_metallic.
RT_DEV void rq_write_no_surface(uint4 *out) {
    out[0] = make_uint4(0u, 0u, 0u, 0u); out[1] = make_uint4(0u, 0u, 0u, 0u);
    out[2] = make_uint4(0u, 0u, 0u, RQ_NO_TRIANGLE); out[3] = make_uint4(0u, 0u, 0u, 0u);
}
RT_DEV bool rq_finite_word(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void rq_surface_kernel(SceneView S, SurfaceView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const uint4 *in = V.hits + 4 * (size_t)i;
        const uint4 h0 = in[0], h1 = in[1], h2 = in[2], h3 = in[3]; // t triangle ng.xy | ng.z texcoord.xy ns.x | ns.yz tangent.xy | tangent.zw flags reserved
        uint4 *out = V.out + 4 * (size_t)i;
        const uint32_t tri = h0.y;
        const bool finite = rq_finite_word(h1.y) && rq_finite_word(h1.z) && rq_finite_word(h1.w) && rq_finite_word(h2.x) && rq_finite_word(h2.y) &&
                            rq_finite_word(h2.z) && rq_finite_word(h2.w) && rq_finite_word(h3.x) && rq_finite_word(h3.y);
        if (tri == RQ_NO_TRIANGLE || tri >= V.n_tris || !finite) {
            if (tri != RQ_NO_TRIANGLE) atomicAdd(V.totals + RQ_TOTAL_INVALID, 1ull);
            rq_write_no_surface(out);
            continue;
        }
        const float tu = __uint_as_float(h1.y), tv = __uint_as_float(h1.z);
        const uint32_t mat = V.tri_material[tri];
        const float4 *qm = reinterpret_cast<const float4 *>(S.materials + mat);
        const float4 m0 = qm[0], m1 = qm[1], m2 = qm[2];
        const int tex_color = (int)__float_as_uint(m2.x), tex_emis = (int)__float_as_uint(m2.y);
        const int tex_mr = (int)__float_as_uint(m2.z), tex_nrm = (int)__float_as_uint(m2.w);
        // the four image descriptors go out together, as in shade_fetch_attr (slot 0 stands in for an absent texture: the load is then unused)
        const GpuImage im_c = S.images[tex_color >= 0 ? tex_color : 0], im_e = S.images[tex_emis >= 0 ? tex_emis : 0];
        const GpuImage im_m = S.images[tex_mr >= 0 ? tex_mr : 0], im_n = S.images[tex_nrm >= 0 ? tex_nrm : 0];
        F3 color = f3(1.f, 1.f, 1.f), emission = f3(m1.x, m1.y, m1.z), mr = f3(1.f, 1.f, 1.f), nsample = f3(0.5f, 0.5f, 1.f);
        if (tex_color >= 0) color = sample_texture(S, im_c, tu, tv, true);                     // scene.cpp:107-115
        if (tex_emis >= 0) emission = emission * sample_texture(S, im_e, tu, tv, true);        // :117-125
        if (tex_mr >= 0) mr = sample_texture(S, im_m, tu, tv, false);                          // :127-135
        if (tex_nrm >= 0) nsample = sample_texture(S, im_n, tu, tv, false);                    // :137-145
        const F3 ns = f3(__uint_as_float(h1.w), __uint_as_float(h2.x), __uint_as_float(h2.y));
        const F3 tg = f3(__uint_as_float(h2.z), __uint_as_float(h2.w), __uint_as_float(h3.x));
        const F3 sn = apply_normal_map(ns, tg, __uint_as_float(h3.y), nsample);                // :146
        const float rr = smax(0.08f, m1.w * mr.y);
        out[0] = make_uint4(rq_bits(color.x), rq_bits(color.y), rq_bits(color.z), rq_bits(rr * rr)); // :148 pow(., 2.0) == exact square
        out[1] = make_uint4(rq_bits(emission.x), rq_bits(emission.y), rq_bits(emission.z), rq_bits(mr.z)); // :149
        out[2] = make_uint4(rq_bits(sn.x), rq_bits(sn.y), rq_bits(sn.z), mat);
        out[3] = make_uint4(__float_as_uint(m0.x), __float_as_uint(m0.y), __float_as_uint(m0.z), __float_as_uint(m0.w));
    }
}

// What a ray that misses sees: the background colour or the equirect lookup for d as it is (a d.y beyond +-1 gives the reference's NaN);
// an invalid ray (rq_valid_ray: the rule of the closest-hit query) sees 0, 0, 0.
RT_DEV F3 rq_environment(const SceneView &S, F3 o, F3 d, bool &valid) {
    valid = rq_valid_ray(o, d);
    if (!valid) return f3(0.f, 0.f, 0.f);
    const F3 c = miss_color(S, d);
    return f3(rq_x86_nan(c.x), rq_x86_nan(c.y), rq_x86_nan(c.z));
}

__global__ __launch_bounds__(256) void rq_environment_kernel(SceneView S, EnvironmentView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const float *p = V.rays + 6 * (size_t)i;
        bool valid;
        const F3 c = rq_environment(S, f3(p[0], p[1], p[2]), f3(p[3], p[4], p[5]), valid);
        if (!valid) atomicAdd(V.totals + RQ_TOTAL_INVALID, 1ull);
        float *out = V.rgb + 3 * (size_t)i;
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
    }
}

// Scene::getCameraRay for the point (nx, ny) of the image plane in pixel units: wf_camera_ray's expressions without its two random
// draws.  xy == nullptr: the centre of pixel first_pixel + i in frame order (nx = x + 0.5f, ny = y + 0.5f).
__global__ __launch_bounds__(256) void rq_camera_rays_kernel(SceneView S, CameraView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        float nx, ny;
        if (V.xy) { nx = V.xy[2 * (size_t)i]; ny = V.xy[2 * (size_t)i + 1]; }
        else {
            const uint32_t pixel = V.first_pixel + i;
            nx = (float)(pixel % (uint32_t)V.width) + 0.5f;
            ny = (float)(pixel / (uint32_t)V.width) + 0.5f;
        }
        const float cx = V.tan_fov_x * (2 * nx / (float)V.width - 1);   // scene.cpp:183-184
        const float cy = S.tan_fov_y * (2 * ny / (float)V.height - 1);
        const F3 d = normalize(cx * f3(S.cam_right) - cy * f3(S.cam_up) + f3(S.cam_fwd));
        float *out = V.rays + 6 * (size_t)i;
        out[0] = S.cam_pos[0]; out[1] = S.cam_pos[1]; out[2] = S.cam_pos[2];
        out[3] = d.x; out[4] = d.y; out[5] = d.z;
    }
}

// The planes of a chunk of pixels from what the three queries answered for them.  Hit: albedo = base_color * color, normal = sn,
// depth = t, emission.  Miss: albedo = the environment's answer for the ray, the rest 0.
__global__ __launch_bounds__(256) void rq_guides_kernel(SceneView S, GuidesView V) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.n; i += gridDim.x * 256u) {
        const uint4 h0 = V.hits[4 * (size_t)i];
        F3 albedo, normal = f3(0.f, 0.f, 0.f), emission = f3(0.f, 0.f, 0.f);
        float depth = 0.f;
        if (h0.y != RQ_NO_TRIANGLE) {
            const uint4 *s = V.surfaces + 4 * (size_t)i;
            const uint4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
            albedo = f3(__uint_as_float(s3.x), __uint_as_float(s3.y), __uint_as_float(s3.z)) * f3(__uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z));
            normal = f3(__uint_as_float(s2.x), __uint_as_float(s2.y), __uint_as_float(s2.z));
            emission = f3(__uint_as_float(s1.x), __uint_as_float(s1.y), __uint_as_float(s1.z));
            depth = __uint_as_float(h0.x);
        } else {
            const float *p = V.rays + 6 * (size_t)i;
            bool valid;
            albedo = rq_environment(S, f3(p[0], p[1], p[2]), f3(p[3], p[4], p[5]), valid);
        }
        if (V.albedo) { float *q = V.albedo + 3 * (size_t)i; q[0] = albedo.x; q[1] = albedo.y; q[2] = albedo.z; }
        if (V.normal) { float *q = V.normal + 3 * (size_t)i; q[0] = normal.x; q[1] = normal.y; q[2] = normal.z; }
        if (V.depth) V.depth[i] = depth;
        if (V.emission) { float *q = V.emission + 3 * (size_t)i; q[0] = emission.x; q[1] = emission.y; q[2] = emission.z; }
    }
}

} // namespace dev
} // namespace rtamd

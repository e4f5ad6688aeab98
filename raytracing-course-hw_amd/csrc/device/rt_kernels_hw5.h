// Kernel for the hw5 snapshot: analytic primitives + TRIANGLE figures with per-figure position/rotation, a BVH over the
// non-plane figures, Mix{Cosine, FiguresMix{box | ellipsoid | triangle lights behind their own BVH}} and one
// minstd_rand(y*W+x) per pixel — the reference's own seeding from this snapshot on, so the HIP path is checked for the
// same pixels as the reference program (hw5/src/scene.cpp:8-126, primitives.cpp:12-222, bvh.h:18-141,
// distributions.h:15-302, sceneio.cpp:103-123).
//
// `eps` is a long double in this snapshot (primitives.h:9): (t + eps) is an 80-bit sum narrowed to float.  The device has
// no 80-bit type; the sum is formed in double, which can differ from the reference in the last float bit only when the
// exact sum lies within ~1e-20 of a float rounding boundary (probability ~1e-9 per evaluation).
#pragma once
#include "rt_types_hw5.h"
#include "rt_kernels_hw4.h"
#include "rt_ref_walk.h"

namespace rtamd {
namespace dev {

#define RT5_STACK 64

struct FigRegs { PrimRegs P; F3 data2, data3; bool last; };
RT_DEV FigRegs load_fig5(const GpuFig5 *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6];
    FigRegs F;
    F.P.data = f3(q0.x, q0.y, q0.z); F.P.type = (int)__float_as_uint(q0.w);
    F.P.position = f3(q1.x, q1.y, q1.z); F.P.kind = (int)__float_as_uint(q1.w);
    F.P.rot.v = f3(q2.x, q2.y, q2.z); F.P.rot.w = q2.w;
    F.P.color = f3(q3.x, q3.y, q3.z); F.P.ior = q3.w;
    F.P.emission = f3(q4.x, q4.y, q4.z); F.last = __float_as_uint(q4.w) != 0u;
    F.data2 = f3(q5.x, q5.y, q5.z);
    F.data3 = f3(q6.x, q6.y, q6.z);
    return F;
}

// Figure::intersect (primitives.cpp:13-35); the triangle branch is intersectAsTriangle (:143-166)
RT_DEV bool fig_hit5(const FigRegs &F, F3 o, F3 d, float &t, F3 &norma, bool &inside) {
    if (F.P.type != RT_PRIM_TRIANGLE) return prim_hit<false, true>(F.P, o, d, t, norma, inside);
    F3 to = qtransform(F.P.rot, o - F.P.position), td = qtransform(F.P.rot, d);
    F3 a = F.data3, b = F.P.data - a, c = F.data2 - a;
    F3 n = crossr(b, c);
    F3 oa = to - a;
    float dn = dot(td, n);
    t = -dot(oa, n) / dn;
    if (!(t > 0 && t < 1e4f)) return false;
    inside = dn > 0;
    F3 p = oa + t * td;
    if (dot(crossr(b, p), n) < 0) return false;
    if (dot(crossr(p, c), n) < 0) return false;
    if (dot(crossr(c - b, p - b), n) < 0) return false;
    norma = normalize(qtransform(qconj(F.P.rot), inside ? neg(n) : n));
    return true;
}

struct Hit5 { int idx; float t; F3 n; bool inside; };
// Scene::intersect (scene.cpp:25-45): planes first (strict '<' keeps the first), then the BVH, whose result replaces
// the plane hit only when strictly nearer.
RT_DEV Hit5 closest_hit5(const SceneView5 &S, F3 o, F3 d, uint32_t *stack) {
    Hit5 best; best.idx = -1; best.t = RT_T_MAX; best.n = f3(0.f, 0.f, 0.f); best.inside = false;
    for (uint32_t i = S.n_nonplanes; i < S.n_figs; i++) {
        FigRegs F = load_fig5(S.figs + i);
        float t; F3 n; bool inside;
        if (fig_hit5(F, o, d, t, n, inside) && (best.idx < 0 || t < best.t)) { best.idx = (int)i; best.t = t; best.n = n; best.inside = inside; }
    }
    if (S.n_nonplanes == 0) return best;
    // BVH::intersect_ (bvh.h:111-141) with the reference's own box test on its unpadded boxes (AABB::intersect, primitives.cpp:221-223 ->
    // intersectBoxAndRay, :92-116: ref_box_test of rt_ref_walk.h is the same code), as an iterative left-first walk.  The recursion's
    // `curBest` at a node is the smallest t of the plane hit and of everything found before the node in this order (every level hands
    // its left result on to its right child), so one running value prunes (`curBest < t_box && !inside`); the result is the first
    // figure with the smallest t (a leaf and a parent both replace on strict '<' only), and it replaces the plane hit when strictly nearer.
    // hw5's scenes are a handful of figures: the exact test at every node costs nothing that matters, and no gate is needed.
    bool have_cur = best.idx >= 0;
    float cur_best = best.t;
    Hit5 bvh; bvh.idx = -1; bvh.t = RT_T_MAX; bvh.n = f3(0.f, 0.f, 0.f); bvh.inside = false;
    int sp = 0;
    uint32_t cur = 0;
    for (;;) {
        const RefNodeView n = load_ref_node(S.ref_nodes + cur);
        float tb; bool inside_box;
        if (ref_box_test(n.mn, n.mx, o, d, tb, inside_box) && !(have_cur && cur_best < tb && !inside_box)) {
            if (n.left == 0) {
                for (uint32_t i = n.first; i < n.last; i++) {
                    FigRegs F = load_fig5(S.figs + i);
                    float t; F3 nn; bool inside;
                    if (fig_hit5(F, o, d, t, nn, inside) && (bvh.idx < 0 || t < bvh.t)) { bvh.idx = (int)i; bvh.t = t; bvh.n = nn; bvh.inside = inside; }
                }
                if (bvh.idx >= 0 && (!have_cur || bvh.t < cur_best)) { have_cur = true; cur_best = bvh.t; }
            } else if (sp < RT5_STACK) { stack[sp++] = n.right; cur = n.left; continue; }
        }
        if (sp == 0) break;
        cur = stack[--sp];
    }
    if (bvh.idx >= 0 && (best.idx < 0 || bvh.t < best.t)) best = bvh;
    return best;
}

// pdfOne of the three light kinds (distributions.h:69-71, :117-119, :150-155)
RT_DEV float pdf_one5(const FigRegs &F, F3 x, F3 d, F3 y, F3 yn) {
    if (F.P.type != RT_PRIM_TRIANGLE) return pdf_one4(F.P, x, d, y, yn);
    F3 a = F.data3, b = F.P.data - a, c = F.data2 - a;
    float pointProb = (float)(1.0 / (0.5 * (double)len(crossr(b, c))));       // :121-127
    return (float)((double)(pointProb * len2(x - y)) / fabs((double)dot(d, yn)));
}
// FiguresMix::pdfOneFigureLight, distributions.h:219-254
RT_DEV float light_pdf_one5(const FigRegs &F, F3 x, F3 d) {
    float t1; F3 n1; bool in1;
    if (!fig_hit5(F, x, d, t1, n1, in1)) return 0.f;
    if (t1 != t1) return __builtin_inff();
    float ans = pdf_one5(F, x, d, x + t1 * d, n1);
    if (F.P.type == RT_PRIM_TRIANGLE) return ans;
    float t2; F3 n2; bool in2;
    if (!fig_hit5(F, x + (float)((double)t1 + 1e-4) * d, d, t2, n2, in2)) return ans;
    F3 y2 = x + (float)((double)t1 + 1e-4 + (double)t2) * d;
    return ans + pdf_one5(F, x, d, y2, n2);
}
// FiguresMix::getTotalPdf, distributions.h:256-274: total(left) + total(right), sequential sum inside a leaf, the reference's own box
// test at every node — frame_sum of rt_ref_walk.h over the reference's nodes.
RT_DEV float light_pdf_sum5(const SceneView5 &S, F3 x, F3 d, uint32_t *stack) {
    return frame_sum<RT5_STACK>(stack, [&](uint32_t cur, uint32_t &l, uint32_t &r, float &v) {
        return ref_node(S.ref_light_nodes, x, d, cur, l, r, v, [&](uint32_t first, uint32_t last) {
            float result = 0.f;
            for (uint32_t i = first; i < last; i++) {
                FigRegs F = load_fig5(S.lights + i);
                result += light_pdf_one5(F, x, d);
            }
            return result;
        });
    });
}

// One light's sample: TriangleLight, BoxLight or EllipsoidLight of the figure F
RT_DEV F3 light_sample5(const FigRegs &F, Rng &rng, F3 x) {
    if (F.P.type == RT_PRIM_TRIANGLE) {                                        // TriangleLight::sample :129-142
        F3 a = F.data3, b = F.P.data - a, c = F.data2 - a;
        float u = rng_u01(rng);
        float v = rng_u01(rng);
        if ((double)(u + v) > 1.) { u = 1 - u; v = 1 - v; }
        F3 point = F.P.position + qtransform(qconj(F.P.rot), a + u * b + v * c);
        return normalize(point - x);
    }
    return light_sample_reject(F.P, x, [&]() {                                 // BoxLight::sample :84-105, EllipsoidLight::sample :160-171 (the pixel's shared n01)
        if (F.P.type == RT_PRIM_BOX) return box_face_point(rng, F.P.data);
        float a = rng_n01(rng), b = rng_n01(rng), c = rng_n01(rng);
        return F.P.data * normalize(f3(a, b, c));
    }, [&](F3 dir) { float t; F3 nn; bool inside; return fig_hit5(F, x, dir, t, nn, inside); });
}
// Mix::sample (distributions.h:283-290) -> Cosine::sample (:43-53) or FiguresMix::sample (:200-209) -> one light's sample
RT_DEV F3 mix_sample5(const SceneView5 &S, Rng &rng, F3 x, F3 n) {
    float comps = S.n_lights ? 2.f : 1.f;
    int distNum = (int)(rng_u01(rng) * comps);
    if (distNum == 0) return cosine_sample_txt(rng, n);
    int li = (int)(rng_u01(rng) * (float)S.n_lights);
    FigRegs F = load_fig5(S.lights + li);
    return light_sample5(F, rng, x);
}
// Mix::pdf :292-302 with FiguresMix::pdf :211-213
RT_DEV float mix_pdf5(const SceneView5 &S, F3 x, F3 n, F3 d, uint32_t *stack) {
    float ans = 0.f;
    ans += smax(0.f, dot(d, n) / RT4_PI);
    if (S.n_lights == 0) return ans / 1.f;
    ans += light_pdf_sum5(S, x, d, stack) / (float)S.n_lights;
    return ans / 2.f;
}

// Scene::getColor, hw5/src/scene.cpp:47-103: trace_tree over the planes and the BVH, with this snapshot's Mix
struct TreePolicy5 {
    const SceneView5 &S;
    uint32_t *stack;
    RT_DEV int closest(F3 o, F3 d, float &t, F3 &n, bool &inside) const {
        Hit5 c = closest_hit5(S, o, d, stack);
        t = c.t; n = c.n; inside = c.inside;
        return c.idx;
    }
    RT_DEV PrimRegs material(int idx) const { return load_fig5(S.figs + idx).P; }
    RT_DEV bool diffuse(const Hit3 &h, F3 x, Rng &rng, Frame3 &f, F3 &o, F3 &d) const {
        return mix_diffuse(h, x, f, o, d, [&](F3 xs, F3 n) { return mix_sample5(S, rng, xs, n); }, [&](F3 xs, F3 n, F3 w) { return mix_pdf5(S, xs, n, w, stack); });
    }
};

#ifndef RT_DEVICE_FUNCTIONS_ONLY // set by a translation unit that wants the RT_DEV functions above without a second copy of the kernel
__global__ __launch_bounds__(64) void render_hw5_kernel(SceneView5 S, RenderView R, float tan_fov_y, uint32_t n_work) {
    uint32_t stack[RT5_STACK];
    for_each_pixel(R, n_work, [&](int x, int y) {
        return average_samples(R, x, y, [&](Rng &rng, float fx, float fy) { // seed: hw5/src/sceneio.cpp:110
            F3 o, d;
            camera_ray_float(S, tan_fov_y, R.width, R.height, fx, fy, o, d);
            TreePolicy5 policy{S, stack};
            return trace_tree(policy, S.bg, R.ray_depth, rng, o, d);
        });
    });
}
#endif

} // namespace dev
} // namespace rtamd

// Kernel for the hw4 snapshot: hw3's path tracer over the flat primitive list with importance sampling,
// Mix{Cosine, Mix{BoxLight | EllipsoidLight ...}} (hw4/src/scene.cpp:10-122, hw4/src/include/distributions.h:13-204).
//
// Like hw3 the reference draws the whole frame from one file-static engine, which cannot be replayed in parallel; here
// each pixel owns an engine(y*W+x) and fresh distribution objects, so parity with the reference is statistical and the
// arithmetic is checked exactly against the oracle run with the same per-pixel streams (tests/test_gpu_hw4.py).
// Every distribution object of the reference owns its own std::normal_distribution (the cached second value is per
// object): Cosine uses Rng::saved, each EllipsoidLight a slot of LightNormals.
#pragma once
#include "rt_kernels_txt.h"

namespace rtamd {
namespace dev {

#define RT4_MAX_DEPTH RT3_MAX_DEPTH // hw4 and hw5 run trace_tree's frames
#define RT4_MAX_LIGHTS 32
#define RT4_MAX_REJECTIONS 1000000 // the reference loops forever when a light cannot be hit; a GPU wave must not
#define RT4_PI 3.14159274101257324f // const float PI = acos(-1), distributions.h:9

struct LightNormals { float saved[RT4_MAX_LIGHTS]; uint32_t has; };

RT_DEV float rng_n01_slot(Rng &r, LightNormals &N, int slot) {
    float s0 = r.saved; bool h0 = r.has_saved;
    r.saved = N.saved[slot]; r.has_saved = (N.has >> slot) & 1u;
    float v = rng_n01(r);
    N.saved[slot] = r.saved;
    N.has = (N.has & ~(1u << slot)) | ((r.has_saved ? 1u : 0u) << slot);
    r.saved = s0; r.has_saved = h0;
    return v;
}

// distributions.h:115-118 (box) and :159-164 (ellipsoid): solid-angle density of one surface point
RT_DEV float pdf_one4(const PrimRegs &P, F3 x, F3 d, F3 y, F3 yn) {
    if (P.type == RT_PRIM_BOX) {
        float sx = P.data.x, sy = P.data.y, sz = P.data.z;
        float sTotal = 8 * (sy * sz + sx * sz + sx * sy);
        return (float)((double)len2(x - y) / ((double)sTotal * fabs((double)dot(d, yn))));
    }
    F3 r = P.data;
    F3 n = div3(qtransform(P.rot, y - P.position), r);
    float pointProb = (float)(1. / (double)(4 * RT4_PI * len(f3(n.x * r.y * r.z, r.x * n.y * r.z, r.x * r.y * n.z))));
    return (float)((double)(pointProb * len2(x - y)) / fabs((double)dot(d, yn)));
}
// FigureLight::pdf, distributions.h:85-107: first hit, plus the second one behind it
RT_DEV float light_pdf4(const PrimRegs &P, F3 x, F3 d) {
    float t1; F3 n1; bool in1;
    if (!prim_hit<false, true>(P, x, d, t1, n1, in1)) return 0.f;
    if (t1 != t1) return __builtin_inff();
    float ans = pdf_one4(P, x, d, x + t1 * d, n1);
    float t2; F3 n2; bool in2;
    if (!prim_hit<false, true>(P, x + (float)((double)t1 + 0.0001) * d, d, t2, n2, in2)) return ans;
    F3 y2 = x + (float)((double)t1 + 0.0001 + (double)t2) * d;
    return ans + pdf_one4(P, x, d, y2, n2);
}
// BoxLight::sample :125-151: a face by area, its sign, a point on it.
RT_DEV F3 box_face_point(Rng &rng, F3 s) {
    float wx = s.y * s.z, wy = s.x * s.z, wz = s.x * s.y;
    float u = rng_u01(rng) * (wx + wy + wz);
    float flip = (double)rng_u01(rng) > 0.5 ? 1.f : -1.f;
    // Vec3(a, b, c): g++ evaluates constructor-call arguments right to left, so the last coordinate draws first
    if (u < wx) { float c = (2 * rng_u01(rng) - 1) * s.z; float b = (2 * rng_u01(rng) - 1) * s.y; return f3(flip * s.x, b, c); }
    if (u < wx + wy) { float c = (2 * rng_u01(rng) - 1) * s.z; float a = (2 * rng_u01(rng) - 1) * s.x; return f3(a, flip * s.y, c); }
    float b = (2 * rng_u01(rng) - 1) * s.y; float a = (2 * rng_u01(rng) - 1) * s.x; return f3(a, b, flip * s.z);
}
// The loop of BoxLight::sample and EllipsoidLight::sample (:169-180), hw4 and hw5: point() draws a point on the figure in its own frame,
// hit(dir) asks whether the ray from x towards it meets the figure; the direction stands when it does.
template <class POINT, class HIT>
RT_DEV F3 light_sample_reject(const PrimRegs &P, F3 x, POINT point, HIT hit) {
    F3 dir = f3(0.f, 1.f, 0.f);
    for (int attempt = 0; attempt < RT4_MAX_REJECTIONS; attempt++) {
        F3 actual = qtransform(qconj(P.rot), point()) + P.position;
        dir = normalize(actual - x);
        if (hit(dir)) break;
    }
    return dir;
}
// Cosine::sample :55-67, with the pixel's own normal_distribution
RT_DEV F3 cosine_sample_txt(Rng &rng, F3 n) {
    float a = rng_n01(rng), b = rng_n01(rng), c = rng_n01(rng);
    F3 d = normalize(f3(a, b, c)) + n;
    float l = len(d);
    if (l <= 1e-9f || dot(d, n) <= 1e-9f || l != l) return n;
    return (float)(1. / (double)l) * d;
}
// BoxLight::sample :125-151 and EllipsoidLight::sample :169-180 of light li, the figure P
RT_DEV F3 light_sample4(const PrimRegs &P, Rng &rng, LightNormals &N, int li, F3 x) {
    return light_sample_reject(P, x, [&]() {
        if (P.type == RT_PRIM_BOX) return box_face_point(rng, P.data);
        float a = rng_n01_slot(rng, N, li), b = rng_n01_slot(rng, N, li), c = rng_n01_slot(rng, N, li); // each EllipsoidLight its own normal_distribution
        return P.data * normalize(f3(a, b, c));
    }, [&](F3 dir) { float t; F3 nn; bool inside; return prim_hit<false, true>(P, x, dir, t, nn, inside); });
}
// Mix::sample :194-197 (outer {Cosine, lights}, then the inner light choice)
RT_DEV F3 mix_sample4(const SceneViewTxt &S, Rng &rng, LightNormals &N, F3 x, F3 n) {
    float comps = S.n_light_prims ? 2.f : 1.f;
    int distNum = (int)(rng_u01(rng) * comps);
    if (distNum == 0) return cosine_sample_txt(rng, n);
    int li = (int)(rng_u01(rng) * (float)S.n_light_prims);
    PrimRegs P = load_prim(S.prims + S.light_prims[li]);
    return light_sample4(P, rng, N, li, x);
}
// Mix::pdf :199-205
RT_DEV float mix_pdf4(const SceneViewTxt &S, F3 x, F3 n, F3 d) {
    float ans = 0.f;
    ans += smax(0.f, dot(d, n) / RT4_PI);
    if (S.n_light_prims == 0) return ans / 1.f;
    float inner = 0.f;
    for (uint32_t k = 0; k < S.n_light_prims; k++) inner += light_pdf4(load_prim(S.prims + S.light_prims[k]), x, d);
    ans += inner / (float)S.n_light_prims;
    return ans / 2.f;
}

struct Hit3 { PrimRegs P; float t; F3 n; bool inside; }; // the closest figure (of P: material only), distance, normal, side

// Scene::getColor of hw4 and hw5 (hw4/src/scene.cpp:51-112, hw5/src/scene.cpp:47-103) as an explicit frame machine, hw3's (trace_tree3) with its two differences as a policy: one
// random branch per hit, so a frame is "emission + mult * (value of the continued ray)"; a dielectric frame draws its Schlick choice on the
// way back and may then continue with the refracted ray.  What the two snapshots differ in is the policy's:
//   closest(o, d, t, n, inside) -> int      the nearest figure along the ray: its index (-1: none), distance, normal and side
//   material(index) -> PrimRegs             that figure (the machine reads kind, color, emission and ior)
//   diffuse(hit, x, rng, frame, o, d) -> bool   a diffuse hit at x: the frame and the next ray; false: the path ends here with the emission
template <class POLICY>
RT_DEV F3 trace_tree(POLICY &policy, const float *bg, int ray_depth, Rng &rng, F3 o, F3 d) {
    Frame3 frames[RT3_MAX_DEPTH];
    int fp = 0;
    F3 ret = f3(0.f, 0.f, 0.f);
    bool evaluating = true;
    for (;;) {
        if (evaluating) {
            if (fp >= ray_depth) { ret = f3(0.f, 0.f, 0.f); evaluating = false; continue; }
            Hit3 h;
            int pos = policy.closest(o, d, h.t, h.n, h.inside);
            if (pos < 0) { ret = f3(bg); evaluating = false; continue; }
            h.P = policy.material(pos);
            F3 x = o + h.t * d;
            Frame3 &f = frames[fp];
            if (h.P.kind == RT_MAT_DIFFUSE) {
                if (!policy.diffuse(h, x, rng, f, o, d)) { ret = h.P.emission; evaluating = false; continue; }
                fp++;
                continue;
            }
            F3 dn = normalize(d);
            F3 refl = dn - (float)(2. * (double)dot(h.n, dn)) * h.n;    // hw3/src/scene.cpp:53,57
            f.emission = h.P.emission; f.mult = h.P.color; f.x = x; f.dn = dn; f.norma = h.n; f.inside = h.inside; f.ior = h.P.ior;
            f.kind = h.P.kind == RT_MAT_METALLIC ? F3_MUL : F3_DIEL_REFLECT;
            fp++;
            o = x + RT3_EPS * refl; d = refl;
        } else {
            if (fp == 0) break;
            Frame3 &f = frames[--fp];
            if (f.kind == F3_MUL) { ret = f.emission + f.mult * ret; continue; }
            if (f.kind == F3_DIEL_REFRACT) {
                F3 refracted = ret;
                if (!f.inside) refracted = refracted * f.mult;
                ret = f.emission + refracted;
                continue;
            }
            float eta1 = 1.f, eta2 = f.ior;                             // hw3/src/scene.cpp:61-85
            if (f.inside) { float tmp = eta1; eta1 = eta2; eta2 = tmp; }
            F3 l = neg(f.dn);
            float nl = dot(f.norma, l);
            float sinTheta2 = (float)((double)(eta1 / eta2) * sqrt((double)(1 - nl * nl)));
            if (fabs((double)sinTheta2) > 1.) { ret = f.emission + ret; continue; }
            float rr = (eta1 - eta2) / (eta1 + eta2);
            float r0 = rr * rr;
            double om = (double)(1 - nl), om2 = om * om;
            float r = (float)((double)r0 + (double)(1 - r0) * (om2 * om2 * om));
            if (rng_u01(rng) < r) { ret = f.emission + ret; continue; }
            float cosTheta2 = sqrtf(1 - sinTheta2 * sinTheta2);
            F3 refr = (eta1 / eta2) * neg(l) + (eta1 / eta2 * nl - cosTheta2) * f.norma;
            f.kind = F3_DIEL_REFRACT;
            fp++;
            o = f.x + RT3_EPS * refr; d = refr;
            evaluating = true;
        }
    }
    return ret;
}

// The diffuse hit of hw4 and hw5 (hw4/src/scene.cpp:67-74): a direction from the snapshot's Mix, sample(xs, n), weighted by its density
// pdf(xs, n, w); a direction below the surface ends the path.
template <class SAMPLE, class PDF>
RT_DEV bool mix_diffuse(const Hit3 &h, F3 x, Frame3 &f, F3 &o, F3 &d, SAMPLE sample, PDF pdf) {
    F3 xs = x + RT3_EPS * h.n;
    F3 w = sample(xs, h.n);
    if (dot(w, h.n) < 0) return false;
    float p = pdf(xs, h.n, w);
    f.kind = F3_MUL; f.emission = h.P.emission;
    f.mult = (float)(1. / (double)(RT4_PI * p) * (double)dot(w, h.n)) * h.P.color;
    o = x + RT3_EPS * w; d = w;
    return true;
}
// Scene::getColor, hw4/src/scene.cpp:51-112: trace_tree over the flat list, planes cut at T_MAX
struct TreePolicy4 {
    const SceneViewTxt &S;
    LightNormals &N;
    RT_DEV int closest(F3 o, F3 d, float &t, F3 &n, bool &inside) const { return closest_prim<false, true>(S, o, d, t, n, inside); }
    RT_DEV PrimRegs material(int pos) const { return load_prim(S.prims + pos); }
    RT_DEV bool diffuse(const Hit3 &h, F3 x, Rng &rng, Frame3 &f, F3 &o, F3 &d) const {
        return mix_diffuse(h, x, f, o, d, [&](F3 xs, F3 n) { return mix_sample4(S, rng, N, xs, n); }, [&](F3 xs, F3 n, F3 w) { return mix_pdf4(S, xs, n, w); });
    }
};

// hw4/src/scene.cpp:114-132, hw5/src/scene.cpp:105-126: all-float camera ray, no half-pixel offset, direction not normalised
template <class SCENE>
RT_DEV void camera_ray_float(const SCENE &S, float tan_fov_y, int width, int height, float fx, float fy, F3 &o, F3 &d) {
    float nx = S.tan_fov_x * (2 * fx / (float)width - 1);
    float ny = tan_fov_y * (2 * fy / (float)height - 1);
    o = f3(S.cam_pos);
    d = nx * f3(S.cam_right) - ny * f3(S.cam_up) + f3(S.cam_fwd);
}

#ifndef RT_DEVICE_FUNCTIONS_ONLY // set by a translation unit that wants the RT_DEV functions above without a second copy of the kernel
__global__ __launch_bounds__(64) void render_hw4_kernel(SceneViewTxt S, RenderView R, float tan_fov_y, uint32_t n_work) {
    for_each_pixel(R, n_work, [&](int x, int y) {
        LightNormals N;
        N.has = 0u;
        TreePolicy4 policy{S, N};
        return average_samples(R, x, y, [&](Rng &rng, float fx, float fy) {
            F3 o, d;
            camera_ray_float(S, tan_fov_y, R.width, R.height, fx, fy, o, d);
            return trace_tree(policy, S.bg, R.ray_depth, rng, o, d);
        });
    });
}
#endif

} // namespace dev
} // namespace rtamd

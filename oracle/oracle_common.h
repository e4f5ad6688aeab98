// ORACLE — TEST INFRASTRUCTURE ONLY.
// CPU restatement of the reference renderer's arithmetic, used solely as the checker in tests/,
// __graft_entry__.smoke() and bench.py's cpu_baseline leg.  Nothing under
// raytracing-course-hw_amd/ may include, link or call this.
//
// What every snapshot's restatement shares: small float-vector helpers with exactly the reference's operator semantics
// (reference: hw8/src/include/vec3.h:31-80, quaternion.h:31-46), the tonemap, cosine sampling, the specular tail of getColor, the
// render parameters of one call (Frame) and the pixel loop (render_rect).  The tree is in oracle_bvh.h.  Build with
// -O3 -ffp-contract=off and NO -ffast-math / -march, like hw8/CMakeLists.txt:4-11 (Release).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <vector>
#include <algorithm>
#include <random>
#include <omp.h>
#include "../include/rtamd.h"

namespace rto {

struct V3 {
    float x = 0, y = 0, z = 0;
};
// vec3.h:33-47
static inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
static inline V3 operator/(V3 a, V3 b) { return {a.x / b.x, a.y / b.y, a.z / b.z}; }
// vec3.h:74-76 — the scalar is a float parameter: double expressions are narrowed first.
static inline V3 operator*(float k, V3 p) { return {k * p.x, k * p.y, k * p.z}; }
// vec3.h:53-55
static inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// vec3.h:57-59 — NEGATED conventional cross product.
static inline V3 crossr(V3 a, V3 o) { return {a.z * o.y - a.y * o.z, a.x * o.z - a.z * o.x, a.y * o.x - a.x * o.y}; }
static inline float len2(V3 a) { return dot(a, a); }
// vec3.h:65-67 — unqualified sqrt on a float resolves to ::sqrt(double); result narrowed to float.
static inline float len(V3 a) { return (float)std::sqrt((double)len2(a)); }
// vec3.h:78-80 — 1. / len() is a double division, narrowed when passed to operator*(float, Vec3).
static inline V3 normalize(V3 a) { return (float)(1. / (double)len(a)) * a; }
static inline V3 neg1(V3 a) { return (float)(-1.) * a; } // "-1. * v"

struct Quat {
    V3 v;
    float w = 1;
};
// quaternion.h:36-38
static inline Quat qmul(Quat a, Quat b) {
    return {a.w * b.v + b.w * a.v + crossr(a.v, b.v), a.w * b.w - dot(a.v, b.v)};
}
static inline Quat qconj(Quat q) { return {(float)(-1.) * q.v, q.w}; }
// quaternion.h:44-46
static inline V3 qtransform(Quat q, V3 p) { return qmul(qmul(q, Quat{p, 0.f}), qconj(q)).v; }

// libstdc++ std::min / std::max semantics (NaN behaviour matters in the slab test).
static inline float smin(float a, float b) { return (b < a) ? b : a; }
static inline float smax(float a, float b) { return (a < b) ? b : a; }

typedef std::minstd_rand rng_t; // hw8/src/include/scene.h:13
typedef std::uniform_real_distribution<float> U01;
typedef std::normal_distribution<float> N01;
static inline V3 v3(const float *p) { return {p[0], p[1], p[2]}; }

// hw4..hw6 distributions.h:9-11 define a float PI = acos(-1); hw8/src/include/distributions.h:56 divides by (float)M_PI.  Same float.
static const float PI = std::acos(-1);
static_assert((float)__builtin_acos(-1.) == (float)M_PI, "cosine_pdf shares one constant between hw4..hw6 and hw8");

// Render parameters of one call.  Not scene state: the scenes are const during a render.
struct Frame { int width, height, samples, ray_depth; };
// Query counters of the counting oracles (hw6, hw8); also the layout of the rto_hw{6,8}_render `cnt` argument.
struct Counters { uint64_t closest = 0, lightq = 0, boxes = 0, tris = 0; };

// color.cpp:4-31 — epilogue
static inline V3 aces_tonemap(V3 x) {
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    V3 num = x * (a * x + V3{b, b, b});
    V3 den = x * (c * x + V3{d, d, d}) + V3{e, e, e};
    V3 q = num / den;
    return {smin(1.f, smax(0.f, q.x)), smin(1.f, smax(0.f, q.y)), smin(1.f, smax(0.f, q.z))};
}
static inline V3 gamma_corrected(V3 x) {
    float gamma = 1. / 2.2;
    return {(float)std::pow((double)x.x, (double)gamma), (float)std::pow((double)x.y, (double)gamma),
            (float)std::pow((double)x.z, (double)gamma)};
}
static inline void to_extern(V3 c, uint8_t out[3]) {
    out[0] = (uint8_t)std::round((double)(255 * c.x));
    out[1] = (uint8_t)std::round((double)(255 * c.y));
    out[2] = (uint8_t)std::round((double)(255 * c.z));
}


// Cosine::sample — hw4/src/include/distributions.h:55-67, hw5 :43-53, hw6 :42-58, hw8 :42-52.  hw4 keeps one normal_distribution per
// Cosine object (its cached second value survives between calls), hw5+ one per pixel: the caller owns n01 either way.
static inline V3 cosine_sample(N01 &n01, rng_t &rng, V3 n) {
    float a = n01(rng), b = n01(rng), c = n01(rng); // braced init: left to right
    V3 d = normalize(V3{a, b, c});
    d = d + n;
    float l = len(d);
    const float ceps = 1e-9;
    if (l <= ceps || dot(d, n) <= ceps || std::isnan(l)) return n;
    return (float)(1. / l) * d;
}
// Cosine::pdf — hw4 distributions.h:69-72, hw5/hw6 after their sample, hw8 :54-57
static inline float cosine_pdf(V3 n, V3 d) { return smax(0.f, dot(d, n) / PI); }

// The specular tail of getColor: mirror reflection for METALLIC, else the dielectric — reflected branch first, total internal
// reflection, Schlick's Fresnel term, the reflect-or-refract draw, the tint on entry only
// (hw3/src/scene.cpp:52-87, hw4/src/scene.cpp:73-108, hw5/src/scene.cpp:70-105, hw6/src/scene.cpp:70-105).
// epsf is the offset along the new direction as each snapshot computes it: (float)0.0001 in hw3/hw4, (float) of the long double
// constant in hw5/hw6.  u() draws the uniform number where the reference does; get_color(o, d) is the recursion one level down.
template <class Draw, class GetColor>
static inline V3 specular_tail(float t, V3 norma, bool inside, V3 ro, V3 rd, V3 color, V3 emission, int kind, float ior, float epsf,
                               Draw &&u, GetColor &&get_color) {
    V3 dn = normalize(rd);
    V3 refl = dn - (float)(2. * dot(norma, dn)) * norma;
    V3 o = ro + t * rd + epsf * refl;
    if (kind == RT_MAT_METALLIC) return emission + color * get_color(o, refl);
    V3 reflected = get_color(o, refl);
    float eta1 = 1., eta2 = ior;
    if (inside) std::swap(eta1, eta2);
    V3 l = neg1(normalize(rd));
    float sinTheta2 = eta1 / eta2 * std::sqrt((double)(1 - dot(norma, l) * dot(norma, l)));
    if (std::fabs((double)sinTheta2) > 1.) return emission + reflected;
    float r0 = std::pow((double)((eta1 - eta2) / (eta1 + eta2)), 2.);
    float r = r0 + (1 - r0) * std::pow((double)(1 - dot(norma, l)), 5.);
    if (u() < r) return emission + reflected;
    float cosTheta2 = std::sqrt((double)(1 - sinTheta2 * sinTheta2));
    V3 refr = (eta1 / eta2) * neg1(l) + (eta1 / eta2 * dot(norma, l) - cosTheta2) * norma;
    V3 refracted = get_color(ro + t * rd + epsf * refr, refr);
    if (!inside) refracted = refracted * color;
    return emission + refracted;
}

// The pixel loop of every path-tracing snapshot: rectangle [x0,x0+w) x [y0,y0+h) of the frame, row-major; float radiance and
// tonemapped bytes (hw5/src/sceneio.cpp:103-123, hw6/src/sceneio.cpp:280-284, hw8/src/sceneio.cpp:387-396).  sampler_for(x, y) gives the pixel its random stream — a fresh
// one per pixel (hw5+: engine(y*W+x)), or a reference to the one stream of the whole call with serial = true (hw3 / hw4 as the
// reference runs them: pixels strictly in order).  pixel(S, x, y) is getPixel.  counters() is the calling thread's tally, which
// the counting oracles (hw6, hw8) bump while tracing; its sum over the rectangle is returned.
struct NoCounters { Counters *operator()() const { return nullptr; } };
template <class SamplerFor, class Pixel, class Cnt = NoCounters>
static inline Counters render_rect(bool serial, int nthreads, int x0, int y0, int w, int h, float *out_rgb, uint8_t *out8,
                                   SamplerFor &&sampler_for, Pixel &&pixel, Cnt &&counters = Cnt()) {
    auto one = [&](int j, uint64_t &c0, uint64_t &c1, uint64_t &c2, uint64_t &c3) {
        Counters *c = counters();
        if (c) *c = Counters{};
        int x = x0 + j % w, y = y0 + j / w;
        auto &&S = sampler_for(x, y);
        V3 px = pixel(S, x, y);
        if (out_rgb) { out_rgb[3 * j] = px.x; out_rgb[3 * j + 1] = px.y; out_rgb[3 * j + 2] = px.z; }
        if (out8) to_extern(gamma_corrected(aces_tonemap(px)), out8 + 3 * j);
        if (c) { c0 += c->closest; c1 += c->lightq; c2 += c->boxes; c3 += c->tris; }
    };
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (serial) {
        for (int j = 0; j < w * h; j++) one(j, c0, c1, c2, c3);
    } else {
        if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 8) num_threads(nthreads) reduction(+ : c0, c1, c2, c3)
        for (int j = 0; j < w * h; j++) one(j, c0, c1, c2, c3);
    }
    Counters total;
    total.closest = c0; total.lightq = c1; total.boxes = c2; total.tris = c3;
    return total;
}

} // namespace rto

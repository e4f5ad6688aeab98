// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
// Analytic primitives of the hw3 / hw4 / hw5 snapshots (<cmath> flavour: unqualified sqrt/fabs on floats are the double
// C functions, results narrowed) shared by oracle_txt.cpp (hw3), oracle_hw4.cpp and oracle_hw5.cpp,
// and the box / ellipsoid light emitters that hw4 and hw5 share.
#pragma once
#include "oracle_common.h"

namespace rtot {
using namespace rto;

struct Prim {
    int type; V3 data, position; Quat rotation; V3 color, emission; int kind; float ior;
};
struct Hit { float t; V3 norma; bool inside; };

// hw3/src/primitives.cpp:28-47 (hw1: :33-52 without the inside flag)
static inline bool smallest_root(float a, float b, float c, float &t, bool &inside) {
    float d = b * b - 4 * a * c;
    if (d <= 0) return false;
    float x1 = (-b - std::sqrt((double)d)) / (2 * a);
    float x2 = (-b + std::sqrt((double)d)) / (2 * a);
    if (x1 > x2) std::swap(x1, x2);
    if (x2 < 0) return false;
    if (x1 < 0) { t = x2; inside = true; } else { t = x1; inside = false; }
    return true;
}
// hw3/src/primitives.cpp:81-123
static inline bool box_local(V3 s, V3 o, V3 d, Hit &h) {
    V3 ts1 = (neg1(s) - o) / d, ts2 = (s - o) / d;
    float t1x = smin(ts1.x, ts2.x), t2x = smax(ts1.x, ts2.x);
    float t1y = smin(ts1.y, ts2.y), t2y = smax(ts1.y, ts2.y);
    float t1z = smin(ts1.z, ts2.z), t2z = smax(ts1.z, ts2.z);
    float t1 = smax(smax(t1x, t1y), t1z), t2 = smin(smin(t2x, t2y), t2z);
    if (t1 > t2 || t2 < 0) return false;
    float t; bool inside;
    if (t1 < 0) { inside = true; t = t2; } else { inside = false; t = t1; }
    V3 p = o + t * d;
    V3 n = p / s;
    float mx = smax(smax((float)std::fabs((double)n.x), (float)std::fabs((double)n.y)), (float)std::fabs((double)n.z));
    if (std::fabs((double)n.x) != mx) n.x = 0;
    if (std::fabs((double)n.y) != mx) n.y = 0;
    if (std::fabs((double)n.z) != mx) n.z = 0;
    if (inside) n = neg1(n);
    h = Hit{t, n, inside};
    return true;
}
// hw3/src/primitives.cpp:8-26
// plane_tmax: hw4+ reject plane hits at t >= T_MAX = 1e4 (hw4/src/primitives.cpp:8,74)
static inline bool prim_ray3(const Prim &f, V3 o, V3 d, Hit &h, bool plane_tmax = false) {
    V3 to = qtransform(f.rotation, o - f.position), td = qtransform(f.rotation, d);
    bool ok;
    if (f.type == RT_PRIM_ELLIPSOID) {                                     // :49-67
        V3 r = f.data;
        float c = len2(to / r) - 1;
        float b = 2. * dot(to / r, td / r);
        float a = len2(td / r);
        float t; bool inside;
        ok = smallest_root(a, b, c, t, inside);
        if (ok) {
            V3 point = to + t * td;
            V3 n = point / (r * r);
            if (inside) n = neg1(n);
            h = Hit{t, normalize(n), inside};
        }
    } else if (f.type == RT_PRIM_PLANE) {                                   // :69-79 (no T_MAX in hw3)
        V3 n = f.data;
        float t = -dot(to, n) / dot(td, n);
        ok = t > 0 && (!plane_tmax || t < 1e4f);
        if (ok) h = dot(td, n) > 0 ? Hit{t, neg1(n), true} : Hit{t, n, false};
    } else ok = box_local(f.data, to, td, h);
    if (!ok) return false;
    h.norma = normalize(qtransform(qconj(f.rotation), h.norma));
    return true;
}

// ---- the box and ellipsoid emitters of hw4 and hw5 (hw4/src/include/distributions.h:115-180, hw5 :69-171) ------------------------
// Templated on the figure type (Prim / rto5::Fig: type, data, position, rotation) and on the figure's ray test
// ray(fig, o, d, Hit &) — prim_ray3(.., true) in hw4, fig_ray in hw5.  The light pdf's second-hit term stays with each snapshot.
// The two samplers are rejection loops: kept out of line, as they were, because inlined into getColor they slow its recursion down
// (hw5 render +10 %, profiles/r16_oracle_shared.txt).

// BoxLight::pdfOne — hw4 :115-118, hw5 :69-71 (sTotal as the constructor computes it, hw5 :74-82)
template <class Fig> static inline float box_emitter_pdf_one(const Fig &f, V3 x, V3 d, V3 y, V3 yn) {
    float sx = f.data.x, sy = f.data.y, sz = f.data.z;
    float sTotal = 8 * (sy * sz + sx * sz + sx * sy);
    return (double)len2(x - y) / ((double)sTotal * std::fabs((double)dot(d, yn)));
}
// EllipsoidLight::pdfOne — hw4 :159-164, hw5 :150-155
template <class Fig> static inline float ellipsoid_emitter_pdf_one(const Fig &f, V3 x, V3 d, V3 y, V3 yn) {
    V3 r = f.data;
    V3 n = qtransform(f.rotation, y - f.position) / r;
    float pointProb = 1. / (double)(4 * PI * len(V3{n.x * r.y * r.z, r.x * n.y * r.z, r.x * r.y * n.z}));
    return (double)(pointProb * len2(x - y)) / std::fabs((double)dot(d, yn));
}
// One round of BoxLight::sample's loop up to its point — hw4 :134-144, hw5 :88-98: face pick by area, sign flip, a point on the face in
// the box's own frame.  s: the half-sizes.
static inline V3 box_emitter_point(V3 s, U01 &u01, rng_t &rng) {
    float sx = s.x, sy = s.y, sz = s.z;
    float wx = sy * sz, wy = sx * sz, wz = sx * sy;
    float u = u01(rng) * (wx + wy + wz);
    float flipSign = (double)u01(rng) > 0.5 ? 1 : -1;
    // Vec3(a, b, c) is a constructor call: g++ evaluates its arguments right to left, so the LAST
    // coordinate's random number is drawn first (pinned against the compiled reference).
    if (u < wx) { float c = (2 * u01(rng) - 1) * sz; float b = (2 * u01(rng) - 1) * sy; return V3{flipSign * sx, b, c}; }
    if (u < wx + wy) { float c = (2 * u01(rng) - 1) * sz; float a = (2 * u01(rng) - 1) * sx; return V3{a, flipSign * sy, c}; }
    float b = (2 * u01(rng) - 1) * sy; float a = (2 * u01(rng) - 1) * sx; return V3{a, b, flipSign * sz};
}
// BoxLight::sample — hw4 :125-151, hw5 :84-105: rejection until the figure is hit from x.
template <class Fig, class Ray> static __attribute__((noinline)) V3 box_emitter_sample(const Fig &f, U01 &u01, rng_t &rng, V3 x, Ray &&ray) {
    for (;;) {
        V3 point = box_emitter_point(f.data, u01, rng);
        V3 actual = qtransform(qconj(f.rotation), point) + f.position;
        Hit h;
        if (ray(f, x, normalize(actual - x), h)) return normalize(actual - x);
    }
}
// EllipsoidLight::sample — hw4 :169-180 (one normal_distribution per light object), hw5 :160-171 (the pixel's): the caller's n01.
template <class Fig, class Ray> static __attribute__((noinline)) V3 ellipsoid_emitter_sample(const Fig &f, N01 &n01, rng_t &rng, V3 x, Ray &&ray) {
    for (;;) {
        float a = n01(rng), b = n01(rng), c = n01(rng);
        V3 point = f.data * normalize(V3{a, b, c});
        V3 actual = qtransform(qconj(f.rotation), point) + f.position;
        Hit h;
        if (ray(f, x, normalize(actual - x), h)) return normalize(actual - x);
    }
}

static inline Prim prim_from_abi(const rt_primitive &p) {
    Prim f;
    f.type = p.type; f.data = v3(p.data); f.position = v3(p.position);
    f.rotation = Quat{v3(p.rotation), p.rotation[3]};
    f.color = v3(p.color); f.emission = v3(p.emission); f.kind = p.kind; f.ior = p.ior;
    return f;
}

// ---- the function-level entry points (rto_hw*_quad / _fig / _lpdf / _pdf_one / _lsample / _cosine, rto_box_face_point; tests/analytic_cases.py has the rows) --------
// A figure row is 24 floats: type, data 3, data2 3, data3 3, position 3, rotation 4 (x y z w), o 3, d 3, one unused.  Answers are
// 32-bit words: flags (1 hit | 2 inside), then float bits; all 0 for a miss.  The layout is oracle/ref/ref_txt_funcs.cpp's.
enum { ROW = 24, R_TYPE = 0, R_DATA = 1, R_DATA2 = 4, R_DATA3 = 7, R_POS = 10, R_ROT = 13, R_O = 17, R_D = 20 };
static inline uint32_t word(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline Prim prim_of_row(const float *r) {
    Prim f;
    f.type = (int)r[R_TYPE]; f.data = v3(r + R_DATA); f.position = v3(r + R_POS);
    f.rotation = Quat{v3(r + R_ROT), r[R_ROT + 3]};
    f.color = V3{1, 1, 1}; f.emission = V3{1, 1, 1}; f.kind = RT_MAT_DIFFUSE; f.ior = 1;
    return f;
}
static inline void put_hit(bool ok, const Hit &h, uint32_t *o) {
    memset(o, 0, 20);
    if (ok) { o[0] = 1u | (h.inside ? 2u : 0u); o[1] = word(h.t); o[2] = word(h.norma.x); o[3] = word(h.norma.y); o[4] = word(h.norma.z); }
}
template <class Root> static inline void quad_rows(const float *abc, size_t n, uint32_t *out, Root &&root) {
    for (size_t i = 0; i < n; i++) {
        float t = 0; bool inside = false;
        const bool ok = root(abc[3 * i], abc[3 * i + 1], abc[3 * i + 2], t, inside);
        out[2 * i] = ok ? (1u | (inside ? 2u : 0u)) : 0u; out[2 * i + 1] = ok ? word(t) : 0u;
    }
}
// A normal_distribution as a distribution object of a running render holds it: fresh (prime == 0), or with the second value of one
// polar round of engine(prime) cached.
static inline N01 primed(uint32_t prime) {
    N01 n01(0.f, 1.f);
    if (prime) { rng_t p(prime); (void)n01(p); }
    return n01;
}
// out2: whether a value is cached, and its bits (a copy asked for one value leaves its engine alone exactly when it had one cached)
static inline void cache_of(N01 n01, uint32_t *out2) {
    rng_t e(1), e0(1);
    const float v = n01(e);
    out2[0] = e == e0 ? 1u : 0u;
    out2[1] = out2[0] ? word(v) : 0u;
}
static inline uint32_t state_of(rng_t rng) { // the state x of a minstd_rand from its next output 48271 x mod (2^31 - 1)
    return (uint32_t)((uint64_t)rng() * 1899818559ull % 2147483647ull);
}
// 8 words: direction 3, engine state after, cache after 2, cache before 2
static inline void put_sample(V3 d, const rng_t &rng, const N01 &after, const N01 &before, uint32_t *o) {
    o[0] = word(d.x); o[1] = word(d.y); o[2] = word(d.z); o[3] = state_of(rng);
    cache_of(after, o + 4); cache_of(before, o + 6);
}
// The figure test of a rejection loop, counted: the reference loops for ever on a light that cannot be hit; a case table must not.
struct TooManyAttempts {};
template <class Ray> struct CountedRay {
    Ray ray; uint32_t left;
    template <class Fig> bool operator()(const Fig &f, V3 o, V3 d, Hit &h) { if (left-- == 0) throw TooManyAttempts(); return ray(f, o, d, h); }
};
} // namespace rtot

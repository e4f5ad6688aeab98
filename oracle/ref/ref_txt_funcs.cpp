// ORACLE TOOLING — builds ONLY where the reference's sources are; output goes to oracle/_ref/libref_funcs_hw{1..5}.so.
// Function-level harness around one .txt snapshot's own sources (-DREF_HW=1..5, compiled where they lie, nothing copied): the
// figure test, the quadratic, the light pdf, one point's density (pdfOne) and the samplers on their own, n rows per call (tests/analytic_cases.py has the rows).
//
// A figure row is 24 floats: type, data 3, data2 3, data3 3, position 3, rotation 4 (x y z w, as parsed), o 3, d 3, one unused.
// Answers are 32-bit words: flags (1 hit | 2 inside), then float bits; all 0 for a miss.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <random>
#include <sstream>
#include <variant>
#include <vector>
// FigureLight::pdfOne, FiguresMix::pdfOneFigureLight and the distributions' own normal_distribution objects are private; this
// translation unit alone reads the headers with them opened (no layout changes: the reference's .cpp files are compiled as they are).
#define private public
#define protected public
#if REF_HW >= 4
#include "distributions.h"
#endif
#include "primitives.h"
#undef private
#undef protected

#if REF_HW == 1
typedef Point Vec3;
std::optional<float> smallestPositiveRootOfSquareEquation(float a, float b, float c);
#elif REF_HW <= 4
std::optional<std::pair<float, bool>> smallestPositiveRootOfSquareEquation(float a, float b, float c);
#else
std::optional<std::pair<float, bool>> smallestPositiveRootOfQuadraticEquation(float a, float b, float c);
#endif

namespace {
Vec3 v3(const float *p) { return Vec3(p[0], p[1], p[2]); }
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
enum { ROW = 24, R_TYPE = 0, R_DATA = 1, R_DATA2 = 4, R_DATA3 = 7, R_POS = 10, R_ROT = 13, R_O = 17, R_D = 20 };

#if REF_HW <= 2
// hw1 / hw2: one class per shape.  Plane::Plane normalises in hw2 (the loader's doing, not the test's): n is set as the row has it.
struct Holder {
    Ellipsoid e; Plane p; Box b; Figure *f;
    explicit Holder(const float *r) {
        const int type = (int)r[R_TYPE];
        if (type == 0) { e = Ellipsoid(v3(r + R_DATA)); f = &e; }
        else if (type == 1) { p.n = v3(r + R_DATA); f = &p; }
        else { b = Box(v3(r + R_DATA)); f = &b; }
        f->position = v3(r + R_POS);
        f->rotation = Quaternion(r[R_ROT], r[R_ROT + 1], r[R_ROT + 2], r[R_ROT + 3]);
    }
};
#else
Figure make_figure(const float *r) {
    const int type = (int)r[R_TYPE];
#if REF_HW == 5
    Figure f(type == 0 ? FigureType::ELLIPSOID : type == 1 ? FigureType::PLANE : type == 2 ? FigureType::BOX : FigureType::TRIANGLE,
             v3(r + R_DATA), v3(r + R_DATA2), v3(r + R_DATA3));
#else
    Figure f(type == 0 ? FigureType::ELLIPSOID : type == 1 ? FigureType::PLANE : FigureType::BOX, v3(r + R_DATA));
#endif
    f.position = v3(r + R_POS);
    f.rotation = Quaternion(r[R_ROT], r[R_ROT + 1], r[R_ROT + 2], r[R_ROT + 3]);
    f.emission = {1, 1, 1};
    return f;
}
#endif

#if REF_HW >= 4
typedef std::normal_distribution<float> N01;
// A normal_distribution as a distribution object of a running render holds it: fresh (prime == 0), or with the second value of one
// polar round of engine(prime) cached.
N01 primed(uint32_t prime) {
    N01 n01(0.f, 1.f);
    if (prime) { rng_type p(prime); (void)n01(p); }
    return n01;
}
// out2: whether a value is cached, and its bits (a copy is asked for one value: it leaves its engine alone exactly when it had one cached)
void cache_of(N01 n01, uint32_t *out2) {
    rng_type e(1), e0(1);
    const float v = n01(e);
    out2[0] = e == e0 ? 1u : 0u;
    out2[1] = out2[0] ? bits(v) : 0u;
}
uint32_t state_of(const rng_type &rng) { std::ostringstream s; s << rng; return (uint32_t)std::stoul(s.str()); }
void put_sample(Vec3 d, const rng_type &rng, const N01 &after, const N01 &before, uint32_t *o) {
    o[0] = bits(d.x); o[1] = bits(d.y); o[2] = bits(d.z); o[3] = state_of(rng);
    cache_of(after, o + 4); cache_of(before, o + 6);
}
#endif
}

extern "C" {
#pragma GCC visibility push(default)
int reff_hw(void) { return REF_HW; }

// abc: 3 floats per row; out: 2 words (flags, t)
void reff_quad(const float *abc, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *p = abc + 3 * i;
        uint32_t *o = out + 2 * i;
#if REF_HW == 1
        auto r = smallestPositiveRootOfSquareEquation(p[0], p[1], p[2]);
        o[0] = r.has_value() ? 1u : 0u; o[1] = r.has_value() ? bits(r.value()) : 0u;
#else
#if REF_HW <= 4
        auto r = smallestPositiveRootOfSquareEquation(p[0], p[1], p[2]);
#else
        auto r = smallestPositiveRootOfQuadraticEquation(p[0], p[1], p[2]);
#endif
        o[0] = r.has_value() ? (1u | (r.value().second ? 2u : 0u)) : 0u; o[1] = r.has_value() ? bits(r.value().first) : 0u;
#endif
    }
}

// Figure::intersect.  out: 5 words (flags, t, the normal); hw1 has no side and no normal: flags 1, t, zeros.
void reff_fig(const float *rows, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        uint32_t *o = out + 5 * i;
        memset(o, 0, 20);
        const Ray ray(v3(r + R_O), v3(r + R_D));
#if REF_HW == 1
        Holder h(r);
        auto res = h.f->intersect(ray);
        if (res.has_value()) { o[0] = 1u; o[1] = bits(res.value().first); }
#else
#if REF_HW == 2
        Holder h(r);
        auto res = h.f->intersect(ray);
#else
        const Figure f = make_figure(r);
        auto res = f.intersect(ray);
#endif
        if (res.has_value()) {
            const Intersection &x = res.value();
            o[0] = 1u | (x.is_inside ? 2u : 0u); o[1] = bits(x.t); o[2] = bits(x.norma.x); o[3] = bits(x.norma.y); o[4] = bits(x.norma.z);
        }
#endif
    }
}

#if REF_HW == 5
// intersectBoxAndRay(s, ray) without the normal, through AABB(-s, s).intersect: 0.5 * (s - -s) is s and o - 0.5 * (-s + s) is o, exactly.
// rows9: s, o, d; out: 2 words (flags, t)
void reff_slabs(const float *rows9, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *p = rows9 + 9 * i;
        auto r = AABB(Vec3(-p[0], -p[1], -p[2]), v3(p)).intersect(Ray(v3(p + 3), v3(p + 6)));
        out[2 * i] = r.has_value() ? (1u | (r.value().is_inside ? 2u : 0u)) : 0u;
        out[2 * i + 1] = r.has_value() ? bits(r.value().t) : 0u;
    }
}
#endif

#if REF_HW >= 4
// FigureLight::pdf (hw4) / FiguresMix::pdfOneFigureLight (hw5) of the row's figure as a light, x = o.  out: 1 word (the pdf's bits)
void reff_lpdf(const float *rows, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        const Figure f = make_figure(r);
        const Vec3 x = v3(r + R_O), d = v3(r + R_D), nrm(0, 0, 1);
#if REF_HW == 4
        rng_type rng(1);
        std::unique_ptr<FigureLight> L;
        if ((int)r[R_TYPE] == 2) L.reset(new BoxLight(rng, f)); else L.reset(new EllipsoidLight(rng, f));
        out[i] = bits(L->pdf(x, nrm, d));
#else
        FiguresMix mix(std::vector<Figure>{f});
        out[i] = bits(mix.pdfOneFigureLight(mix.figures_[0], x, nrm, d));
#endif
    }
}

// pdfOne(x, d, y, yn) of the row's figure as a light, with a y and yn of the row's own (30 floats: the figure row, then y 3, yn 3).
// out: 1 word (the density's bits); hw4 has no triangle light: 0.
void reff_pdf_one(const float *rows30, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows30 + 30 * i;
        const Figure f = make_figure(r);
        const int type = (int)r[R_TYPE];
        const Vec3 x = v3(r + R_O), d = v3(r + R_D), y = v3(r + 24), yn = v3(r + 27);
#if REF_HW == 4
        rng_type rng(1);
        if (type == 2) out[i] = bits(BoxLight(rng, f).pdfOne(x, d, y, yn));
        else if (type == 0) out[i] = bits(EllipsoidLight(rng, f).pdfOne(x, d, y, yn));
        else out[i] = 0u;
#else
        out[i] = bits(type == 2 ? BoxLight(f).pdfOne(x, d, y, yn) : type == 0 ? EllipsoidLight(f).pdfOne(x, d, y, yn) : TriangleLight(f).pdfOne(x, d, y, yn));
#endif
    }
}

// The light's sample(x) with an engine seeded aux[0] and the normal_distribution it draws from primed by aux[1] (hw4: the
// EllipsoidLight's own; hw5: the caller's).  out: 8 words (direction 3, engine state after, cache after 2, cache before 2).
void reff_lsample(const float *rows, const uint32_t *aux, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        const Figure f = make_figure(r);
        const int type = (int)r[R_TYPE];
        const Vec3 x = v3(r + R_O), nrm(0, 0, 1);
        rng_type rng(aux[2 * i]);
        const N01 before = primed(aux[2 * i + 1]);
        N01 after = before;
        Vec3 d;
#if REF_HW == 4
        if (type == 2) { BoxLight L(rng, f); d = L.sample(x, nrm); }
        else { EllipsoidLight L(rng, f); L.n01 = before; d = L.sample(x, nrm); after = L.n01; }
#else
        std::uniform_real_distribution<float> u01(0.0, 1.0);
        if (type == 2) { BoxLight L(f); d = L.sample(u01, rng, x, nrm); }
        else if (type == 0) { EllipsoidLight L(f); d = L.sample(after, rng, x, nrm); }
        else { TriangleLight L(f); d = L.sample(u01, rng, x, nrm); }
#endif
        put_sample(d, rng, after, before, out + 8 * i);
    }
}

// Cosine::sample(n) with an engine seeded aux[0] and its normal_distribution primed by aux[1].  out as reff_lsample.
void reff_cosine(const float *normals, const uint32_t *aux, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        rng_type rng(aux[2 * i]);
        const N01 before = primed(aux[2 * i + 1]);
        N01 after = before;
#if REF_HW == 4
        Cosine c(rng);
        c.n01 = before;
        const Vec3 d = c.sample(Vec3(0, 0, 0), v3(normals + 3 * i));
        after = c.n01;
#else
        Cosine c;
        const Vec3 d = c.sample(after, rng, Vec3(0, 0, 0), v3(normals + 3 * i));
#endif
        put_sample(d, rng, after, before, out + 8 * i);
    }
}
#endif
#pragma GCC visibility pop
}

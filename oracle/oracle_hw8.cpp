// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the hw8 render path of volivan239/raytracing-course-hw in exact-replay
// semantics: per-pixel std::minstd_rand(y*W+x), libstdc++ uniform_real/normal distributions,
// the reference's float/double expression mix and evaluation order.  Every function cites the
// reference lines it follows.  Pinned against the compiled reference by tests/test_oracle_ref.py
// (oracle/_ref harnesses, fixtures in tests/golden/); see DESIGN.md "Oracle pinning" for what is
// pinned by which fixture and the two glue functions that are "parity unpinned".
#include "oracle_bvh.h"
#include <optional>
#include <utility>
#include <atomic>
#include <cstdio>

namespace rto {

static const float T_MAX = 1e4;               // primitives.cpp:12
static const long double eps_ld = 1e-4;       // primitives.h:9
static const size_t CLAMP_HACK = 6;           // scene.cpp:7

struct Vertex {                                // primitives.h:25-34
    V3 coords;
    float tu = 0, tv = 0;
    V3 normals;
    V3 tan;
    float tanw = 0;
};
struct Fig {                                   // primitives.h:57-74 (triangle only)
    Vertex d, d2, d3;
    uint32_t mat = 0;
    uint32_t orig = 0; // index in LOAD order (bookkeeping, not in the reference)
};
struct Hit {                                   // primitives.h:48-55
    float t;
    V3 ng;
    float tu, tv;
    V3 ns;
    V3 tan;
    float tanw;
    bool inside;
};
static thread_local Counters tl_cnt;
static thread_local std::vector<float> *tl_trace = nullptr; // diagnostic query log of one pixel (rto_hw8_trace_pixel)
static bool g_debug_bruteforce = false;

// ---- primitives.cpp ---------------------------------------------------------------------------
// primitives.cpp:18-27
static inline bool plane_ray(V3 n, V3 o, V3 d, float &t, V3 &ng, bool &inside) {
    t = -dot(o, n) / dot(d, n);
    if (t > 0 && t < T_MAX) {
        if (dot(d, n) > 0) { ng = neg1(n); inside = true; }
        else { ng = n; inside = false; }
        return true;
    }
    return false;
}
// primitives.cpp:76-80
static inline void solve2(float a1, float b1, float c1, float a2, float b2, float c2, float &x, float &y) {
    y = (c1 * a2 - c2 * a1) / (b1 * a2 - a1 * b2);
    x = a2 == 0 ? (c1 - b1 * y) / a1 : (c2 - b2 * y) / a2;
}
static const float magic1[] = {0.239, 0.419, 0.533};        // primitives.cpp:82
static const float magic2[] = {0.35743, 0.66682, 0.69695};  // primitives.cpp:83

// primitives.cpp:85-125
static bool tri_ray(const Fig &f, V3 o, V3 d, Hit &h) {
    tl_cnt.tris++;
    V3 a = f.d3.coords;
    V3 b = f.d.coords - a;
    V3 c = f.d2.coords - a;
    V3 n = crossr(b, c);
    float t; V3 ng; bool inside;
    if (!plane_ray(n, o - a, d, t, ng, inside)) return false;
    V3 p = o - a + t * d;
    float a1 = magic1[0] * b.x + magic1[1] * b.y + magic1[2] * b.z;
    float b1 = magic1[0] * c.x + magic1[1] * c.y + magic1[2] * c.z;
    float c1 = magic1[0] * p.x + magic1[1] * p.y + magic1[2] * p.z;
    float a2 = magic2[0] * b.x + magic2[1] * b.y + magic2[2] * b.z;
    float b2 = magic2[0] * c.x + magic2[1] * c.y + magic2[2] * c.z;
    float c2 = magic2[0] * p.x + magic2[1] * p.y + magic2[2] * p.z;
    float u, v;
    solve2(a1, b1, c1, a2, b2, c2, u, v);
    if (u < 0 || v < 0 || u + v > 1) return false;
    V3 sn = f.d3.normals + u * (f.d.normals - f.d3.normals) + v * (f.d2.normals - f.d3.normals);
    float tu = f.d3.tu + u * (f.d.tu - f.d3.tu) + v * (f.d2.tu - f.d3.tu);
    float tv = f.d3.tv + u * (f.d.tv - f.d3.tv) + v * (f.d2.tv - f.d3.tv);
    V3 tg = f.d3.tan + u * (f.d.tan - f.d3.tan) + v * (f.d2.tan - f.d3.tan);
    tg = normalize(tg);
    sn = normalize(sn);
    if (inside) sn = neg1(sn);
    ng = normalize(ng);
    h = Hit{t, ng, tu, tv, sn, tg, f.d.tanw, inside};
    return true;
}

// ---- bvh.h: the shared builder, sorted on the third corner (bvh.h:60-65) ------------------------
struct Tree8 {
    typedef rto::Hit Hit;
    // primitives.cpp:130-141
    static Box box_of(const Fig &f) {
        Box b;
        b.mn = {smin(f.d3.coords.x, smin(f.d.coords.x, f.d2.coords.x)), smin(f.d3.coords.y, smin(f.d.coords.y, f.d2.coords.y)),
                smin(f.d3.coords.z, smin(f.d.coords.z, f.d2.coords.z))};
        b.mx = {smax(f.d3.coords.x, smax(f.d.coords.x, f.d2.coords.x)), smax(f.d3.coords.y, smax(f.d.coords.y, f.d2.coords.y)),
                smax(f.d3.coords.z, smax(f.d.coords.z, f.d2.coords.z))};
        return b;
    }
    static V3 key(const Fig &f) { return f.d3.coords; }
    static bool hit(const Fig &f, V3 o, V3 d, Hit &h) { return tri_ray(f, o, d, h); }
    static void count_box() { tl_cnt.boxes++; }
};
typedef Bvh<Fig, Tree8> Bvh8;

// ---- material.h ---------------------------------------------------------------------------------
struct MaterialModel {
    float baseMetallic; V3 baseColor;
    // material.h:11-17
    float distributionTerm(V3 h, V3 n, float alpha2) const {
        float dotHN = dot(h, n);
        if (dotHN <= 0) return 0;
        return alpha2 / (M_PI * std::pow((double)smax(0.f, (alpha2 - 1) * dotHN * dotHN + 1), 2.0));
    }
    // material.h:19-21
    float v1(V3 n, V3 x, float alpha2) const {
        return 1. / (std::fabs((double)dot(n, x)) + std::sqrt((double)smax(0.f, alpha2 + (1 - alpha2) * dot(n, x) * dot(n, x))));
    }
    // material.h:23-29
    float specularBrdf(V3 l, V3 v, V3 n, float alpha2) const {
        V3 h = normalize(l + v);
        if (dot(h, l) < 1e-4 || dot(h, v) < 1e-4) return 0;
        return distributionTerm(h, n, alpha2) * v1(n, l, alpha2) * v1(n, v, alpha2);
    }
    // material.h:31-33
    V3 diffuseBrdf(V3 color) const { return (float)(1. / M_PI) * color; }
    // material.h:35-37
    V3 fresnelTerm(V3 f0, V3 f90, V3 v, V3 h) const {
        return f0 + (float)std::pow((double)smax(0.f, (float)(1.f - std::fabs((double)dot(v, h)))), 5.0) * (f90 - f0);
    }
    // material.h:42-65
    V3 brdf(V3 l, V3 v, V3 n, V3 color, float metallic, float alpha) const {
        V3 h = normalize(l + v);
        float specular = specularBrdf(l, v, n, alpha * alpha);
        V3 metalBrdf, dielectricBrdf;
        metallic *= baseMetallic;
        if (metallic > 0 && dot(v, n) >= 0 && dot(l, n) >= 0) {
            V3 ft = fresnelTerm(baseColor * color, V3{1, 1, 1}, v, h);
            metalBrdf = specular * ft;
        }
        if (metallic < 1) {
            V3 diffuse;
            if (dot(l, n) >= 0) diffuse = diffuseBrdf(baseColor * color);
            V3 ft = fresnelTerm(V3{0.04, 0.04, 0.04}, V3{1, 1, 1}, v, h);
            dielectricBrdf = diffuse * (V3{1, 1, 1} - ft) + specular * ft;
        }
        return (float)(1.0 - metallic) * dielectricBrdf + metallic * metalBrdf;
    }
    // hw7/src/include/material.h:44-61 — hw7 form (per-material alpha2/metallic, no texture inputs, no
    // v.n / l.n gates); used only to pin the shared integrator structure against the compiled hw7 reference.
    V3 brdf_hw7(V3 l, V3 v, V3 n, float alpha2) const {
        V3 h = normalize(l + v);
        float specular = specularBrdf(l, v, n, alpha2);
        V3 metalBrdf, dielectricBrdf;
        float metallic = baseMetallic;
        if (metallic > 0) {
            V3 ft = fresnelTerm(baseColor, V3{1, 1, 1}, v, h);
            metalBrdf = specular * ft;
        }
        if (metallic < 1) {
            V3 diffuse = diffuseBrdf(baseColor);
            V3 ft = fresnelTerm(V3{0.04, 0.04, 0.04}, V3{1, 1, 1}, v, h);
            dielectricBrdf = diffuse * (V3{1, 1, 1} - ft) + specular * ft;
        }
        return (float)(1.0 - metallic) * dielectricBrdf + metallic * metalBrdf;
    }
};

// ---- distributions.h ----------------------------------------------------------------------------
struct TriLight {                              // distributions.h:60-95
    float pointProb;
    Fig fig;
    explicit TriLight(const Fig &f) : fig(f) {
        V3 a = fig.d3.coords, b = fig.d.coords - a, c = fig.d2.coords - a;
        V3 n = crossr(b, c);
        pointProb = 1.0 / (0.5 * len(n));
    }
    float pdfOne(V3 x, V3 d, V3 y, V3 yn) const { return pointProb * len2(x - y) / std::fabs((double)dot(d, yn)); }
    V3 sample(U01 &u01, rng_t &rng, V3 x) const {
        V3 a = fig.d3.coords, b = fig.d.coords - a, c = fig.d2.coords - a;
        float u = u01(rng);
        float v = u01(rng);
        if (u + v > 1.) { u = 1 - u; v = 1 - v; }
        V3 point = a + u * b + v * c;
        return normalize(point - x);
    }
};

struct FiguresMix {                            // distributions.h:97-166
    std::vector<TriLight> lights;
    Bvh8 bvh;
    bool hw7_geom_normal = false;              // hw7/src/include/distributions.h:140-145 uses yn (geometric)
    float pdf_one(const TriLight &tl, V3 x, V3 d) const { // distributions.h:131-146
        Hit h;
        if (!tri_ray(tl.fig, x, d, h)) return 0.;
        if (std::isnan(h.t)) return INFINITY;
        V3 y = x + h.t * d;
        return tl.pdfOne(x, d, y, hw7_geom_normal ? h.ng : h.ns);
    }
    float pdf(V3 x, V3 d) const { // :122-124
        tl_cnt.lightq++;
        float r = bvh.total_pdf(0, x, d, [&](uint32_t i) { return pdf_one(lights[i], x, d); }) / lights.size(); // getTotalPdf :148-165
        if (g_debug_bruteforce) { // diagnostic: lights whose triangle test hits but whose BVH boxes the reference's slab test rejects
            float brute = 0; int nh = 0;
            for (const TriLight &tl : lights) { float p = pdf_one(tl, x, d); if (p != 0) nh++; brute += p; }
            brute /= lights.size();
            if (brute != r && !(brute != brute && r != r)) {
                fprintf(stderr, "[oracle] light pdf via BVH %.9g, brute force over all lights %.9g (%d hit)\n", r, brute, nh);
                for (size_t li = 0; li < lights.size(); li++) {
                    if (pdf_one(lights[li], x, d) == 0) continue;
                    uint32_t pos = 0; // walk root -> leaf of light li, report the first rejecting box
                    for (;;) {
                        const Node &n = bvh.nodes[pos];
                        float t; bool inside;
                        Tree8::count_box();
                        bool ok = aabb_ray(n.aabb, x, d, t, inside);
                        if (!ok) {
                            V3 s = 0.5f * (n.aabb.mx - n.aabb.mn), o = x - 0.5f * (n.aabb.mn + n.aabb.mx);
                            V3 ts1 = (neg1(s) - o) / d, ts2 = (s - o) / d;
                            fprintf(stderr, "   light %zu pdf %.6g rejected at node %u [%u,%u) box (%.9g %.9g %.9g)-(%.9g %.9g %.9g)\n      o' (%.9g %.9g %.9g) d (%.9g %.9g %.9g) ts1 (%.9g %.9g %.9g) ts2 (%.9g %.9g %.9g)\n",
                                    li, pdf_one(lights[li], x, d), pos, n.first, n.last, n.aabb.mn.x, n.aabb.mn.y, n.aabb.mn.z, n.aabb.mx.x, n.aabb.mx.y, n.aabb.mx.z,
                                    o.x, o.y, o.z, d.x, d.y, d.z, ts1.x, ts1.y, ts1.z, ts2.x, ts2.y, ts2.z);
                            break;
                        }
                        if (n.left == 0) break;
                        pos = (li < bvh.nodes[n.right].first) ? n.left : n.right;
                    }
                }
            }
        }
        return r;
    }
    V3 sample(U01 &u01, rng_t &rng, V3 x) const {                                             // :117-120
        int k = u01(rng) * lights.size();
        return lights[k].sample(u01, rng, x);
    }
};

// distributions.h:168-246
struct Vndf {
    // :180-184, the two draws and the point on the disk; nothing before them in sample_ draws or depends on them
    static void disk_point(U01 &u01, rng_t &rng, float &t1, float &t2) {
        float u1 = u01(rng), u2 = u01(rng);
        float r = std::sqrt((double)u1);
        float phi = 2.0 * M_PI * u2;
        t1 = r * std::cos((double)phi);
        t2 = r * std::sin((double)phi);
    }
    static V3 sample_(U01 &u01, rng_t &rng, V3 v, float alpha) {
        float t1, t2;
        disk_point(u01, rng, t1, t2);
        return sample_local(t1, t2, v, alpha);
    }
    // :170-194 without the draws
    static V3 sample_local(float t1, float t2, V3 v, float alpha) {
        V3 vh = normalize(V3{alpha * v.x, alpha * v.y, v.z});
        float lensq = vh.x * vh.x + vh.y * vh.y;
        V3 T1 = lensq > 0 ? (float)(1. / std::sqrt((double)lensq)) * V3{-vh.y, vh.x, 0} : V3{1, 0, 0};
        V3 T2 = crossr(T1, vh);
        float s = 0.5 * (1.0 + vh.z);
        t2 = (1.0 - s) * std::sqrt((double)(1.f - t1 * t1)) + s * t2;
        V3 nh = t1 * T1 + t2 * T2 + (float)std::sqrt((double)std::max<float>(0.f, 1.0 - t1 * t1 - t2 * t2)) * vh;
        V3 ne = normalize(V3{alpha * nh.x, alpha * nh.y, std::max<float>(0.0, nh.z)});
        return (2 * dot(ne, v)) * ne - v;
    }
    static float D(V3 n, float a) {
        return 1. / (M_PI * a * a * std::pow((double)(n.x * n.x / (a * a) + n.y * n.y / (a * a) + n.z * n.z), 2.0));
    }
    static float G1(V3 v, float a) {
        float lambda = 0.5 * (-1 + std::sqrt((double)(1 + (a * a * v.x * v.x + a * a * v.y * v.y) / (v.z * v.z))));
        return 1. / (1 + lambda);
    }
    static float pdf_(V3 d, V3 v, float a) {
        V3 ni = normalize(v + d);
        float dv = G1(v, a) * smax(0.f, dot(v, ni)) * D(ni, a) / std::fabs((double)v.z);
        float res = dv / (4 * dot(v, ni));
        return res;
    }
    static Quat getQ(V3 n) {
        V3 newN = {0, 0, 1};
        if (dot(n, newN) > 0.9999) return Quat{};
        if (dot(n, newN) < -0.9999) return Quat{V3{0, 0, 0}, -1};
        V3 a = crossr(n, newN);
        float w = std::sqrt((double)len2(n)) + dot(n, newN); // double sum, narrowed once
        float l = std::sqrt((double)(len2(a) + w * w));
        return Quat{(float)(1. / l) * a, w / l};
    }
    static V3 sample(U01 &u01, rng_t &rng, V3 n, V3 v, float alpha) {
        v = neg1(v);
        Quat q = getQ(n);
        V3 vT = qtransform(q, v);
        V3 dT = sample_(u01, rng, vT, alpha);
        return qtransform(qconj(q), dT);
    }
    static float pdf(V3 n, V3 d, V3 v, float alpha) {
        v = neg1(v);
        Quat q = getQ(n);
        return pdf_(qtransform(q, d), qtransform(q, v), alpha);
    }
};

// ---- scene.cpp ----------------------------------------------------------------------------------
struct Tex { int w = 0, h = 0; const uint8_t *data = nullptr; };

// scene.cpp:9-16
static V3 load_texel(int ix, int iy, const Tex &tex, bool srgb) {
    size_t off = 3 * (ix + tex.w * iy);
    // The reference reads out of bounds when a wrapped coordinate rounds up to exactly 1.0
    // (ix == width on the last row); that is UB there, defined here as texel value 0.
    if (off + 2 >= (size_t)tex.w * tex.h * 3) return V3{0, 0, 0};
    V3 res = (float)(1. / 255) * V3{1.f * tex.data[off], 1.f * tex.data[off + 1], 1.f * tex.data[off + 2]};
    if (srgb) return V3{std::pow(res.x, 2.2f), std::pow(res.y, 2.2f), std::pow(res.z, 2.2f)};
    return res;
}
// scene.cpp:94-95.  Vec3's members are float: std::atan2 / std::asin resolve to atan2f / asinf, and only their results are
// widened to double for the rest of each expression.
static void env_uv(V3 d, float &tx, float &ty) {
    tx = 0.5 + 0.5 * std::atan2(d.z, d.x) / M_PI;
    ty = 0.5 - std::asin(d.y) / M_PI;
}
// scene.cpp:18-35
static V3 sample_texture(float tx, float ty, const Tex &tex, bool srgb) {
    tx -= std::floor(tx);
    ty -= std::floor(ty);
    tx *= tex.w;
    ty *= tex.h;
    int ix1 = std::floor(tx), ix2 = (ix1 + 1) % tex.w;
    int iy1 = std::floor(ty), iy2 = (iy1 + 1) % tex.h;
    float dx = tx - ix1;
    float dy = ty - iy1;
    V3 p11 = load_texel(ix1, iy1, tex, srgb);
    V3 p12 = load_texel(ix1, iy2, tex, srgb);
    V3 p21 = load_texel(ix2, iy1, tex, srgb);
    V3 p22 = load_texel(ix2, iy2, tex, srgb);
    return (1 - dx) * ((1 - dy) * p11 + dy * p12) + dx * ((1 - dy) * p21 + dy * p22);
}
// scene.cpp:37-53
static V3 apply_normal_map(V3 sn, V3 tan, float tanw, V3 sample) {
    V3 lx = tan, lz = sn;
    V3 ly = tanw * crossr(lx, lz);
    V3 ln = 2.f * sample - V3{1., 1., 1.};
    V3 n = ln.x * lx + ln.y * ly + ln.z * lz;
    return normalize(n);
}

struct Scene {
    std::vector<Fig> figs;                 // BVH order after init (scene.cpp:76-78)
    std::vector<rt_material> mats;
    std::vector<MaterialModel> models;     // sceneio.cpp:239-244
    std::vector<uint32_t> tex_source;
    std::vector<Tex> images;
    std::vector<std::vector<uint8_t>> image_store;
    bool has_env = false; Tex env;
    V3 camPos, camRight, camUp, camFwd; float fovY = 0;
    V3 bg;
    Bvh8 bvh;
    FiguresMix lightmix;
    int n_components = 2;
    bool hw7 = false; // replay hw7/src/scene.cpp:29-61 instead of hw8/src/scene.cpp:84-165

    bool emissive(const Fig &f) const {     // distributions.h:104-109 (factor, not texture)
        const rt_material &m = mats[f.mat];
        return !(m.emission[0] == 0 && m.emission[1] == 0 && m.emission[2] == 0);
    }
    void init() {
        bvh.init(figs, (uint32_t)figs.size());                       // scene.cpp:76-78
        std::vector<Fig> copy = figs;                                // distributions.h:103 (by value)
        size_t n = std::partition(copy.begin(), copy.end(), [this](const Fig &f) { return emissive(f); }) - copy.begin();
        lightmix.bvh.init(copy, (uint32_t)n);                        // :111
        lightmix.lights.clear();
        for (size_t i = 0; i < n; i++) lightmix.lights.push_back(TriLight(copy[i])); // :112-114
        n_components = lightmix.lights.empty() ? 2 : 3;              // scene.cpp:65-74
    }
    const Tex &tex(int32_t t) const { return images[tex_source[t]]; }

    // distributions.h:256-265
    V3 mix_sample(U01 &u01, N01 &n01, rng_t &rng, V3 x, V3 n, V3 v, float alpha) const {
        int k = u01(rng) * (size_t)n_components;
        if (k == 0) return cosine_sample(n01, rng, n);
        if (k == 2) return lightmix.sample(u01, rng, x);
        return Vndf::sample(u01, rng, n, v, alpha);
    }
    // distributions.h:267-279
    float mix_pdf(V3 x, V3 n, V3 d, V3 v, float alpha) const {
        float ans = 0;
        ans += cosine_pdf(n, d);
        ans += Vndf::pdf(n, d, v, alpha);
        if (n_components == 3) ans += lightmix.pdf(x, d);
        return ans / (size_t)n_components;
    }
    // scene.cpp:179-186
    void camera_ray(const Frame &fr, float x, float y, V3 &o, V3 &d) const {
        float tanFovY = std::tan((double)(fovY / 2));
        float tanFovX = tanFovY * fr.width / fr.height;
        float nx = tanFovX * (2 * x / fr.width - 1);
        float ny = tanFovY * (2 * y / fr.height - 1);
        o = camPos;
        d = normalize(nx * camRight - ny * camUp + camFwd);
    }
    // scene.cpp:84-165
    V3 get_color(U01 &u01, N01 &n01, rng_t &rng, V3 ro, V3 rd, int recLimit) const {
        if (recLimit == 0) return V3{0., 0., 0.};
        Hit h; int idx = -1;
        tl_cnt.closest++;
        const bool found = bvh.intersect(figs, bvh.root, ro, rd, false, 0.f, h, idx);
        if (tl_trace) { // diagnostic (rto_hw8_trace_pixel): every closest-hit query of the traced pixel
            const float rec[12] = {ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, found ? h.t : -1.f, found ? (float)idx : -1.f, found && h.inside ? 1.f : 0.f, found ? h.tu : 0.f, found ? h.tv : 0.f, (float)recLimit};
            tl_trace->insert(tl_trace->end(), rec, rec + 12);
        }
        if (!found) {
            if (!has_env) return bg;
            float tx, ty;
            env_uv(rd, tx, ty);
            return sample_texture(tx, ty, env, true);
        }
        const Fig &f = figs[idx];
        const rt_material &m = mats[f.mat];
        V3 sn = h.ns;
        V3 x = ro + h.t * rd;
        const MaterialModel &model = models[f.mat];
        V3 color{1, 1, 1};
        if (m.base_color_texture >= 0) color = sample_texture(h.tu, h.tv, tex(m.base_color_texture), true);
        V3 emission{m.emission[0], m.emission[1], m.emission[2]};
        if (m.emissive_texture >= 0) emission = emission * sample_texture(h.tu, h.tv, tex(m.emissive_texture), true);
        V3 mr{1, 1, 1};
        if (m.metallic_roughness_texture >= 0) mr = sample_texture(h.tu, h.tv, tex(m.metallic_roughness_texture), false);
        V3 nsample{0.5, 0.5, 1};
        if (m.normal_texture >= 0) nsample = sample_texture(h.tu, h.tv, tex(m.normal_texture), false);
        if (!hw7) sn = apply_normal_map(sn, h.tan, h.tanw, nsample);
        float alpha = hw7 ? (float)std::pow((double)m.roughness_factor, 2.0)   // hw7/src/scene.cpp:44
                          : (float)std::pow((double)smax(0.08f, m.roughness_factor * mr.y), 2.0);
        float metallic = mr.z;
        V3 xo = x + (float)eps_ld * h.ng;
        V3 d = mix_sample(u01, n01, rng, xo, sn, rd, alpha);
        float r2 = m.roughness_factor * m.roughness_factor; // hw7/src/sceneio.cpp:187, material.h:42
        V3 brdf = hw7 ? model.brdf_hw7(d, neg1(rd), sn, r2 * r2) : model.brdf(d, neg1(rd), sn, color, metallic, alpha);
        if (brdf.x < eps_ld && brdf.y < eps_ld && brdf.z < eps_ld) return emission;
        float pdf = mix_pdf(xo, sn, d, rd, alpha);
        float k = 1. / pdf * std::fabs((double)dot(d, sn));
        V3 mult = k * brdf;
        if (mult.x > CLAMP_HACK || mult.y > CLAMP_HACK || mult.z > CLAMP_HACK || std::isnan(mult.x) || std::isnan(mult.y) || std::isnan(mult.z))
            return emission;
        return emission + mult * get_color(u01, n01, rng, xo, d, recLimit - 1);
    }
    // scene.cpp:167-177
    V3 get_pixel(const Frame &fr, rng_t &rng, int x, int y) const {
        U01 u01(0.0, 1.0);
        N01 n01(0.0, 1.0);
        V3 color{0, 0, 0};
        for (int s = 0; s < fr.samples; s++) {
            float nx = x + u01(rng);
            float ny = y + u01(rng);
            V3 o, d;
            camera_ray(fr, nx, ny, o, d);
            color = color + get_color(u01, n01, rng, o, d, fr.ray_depth);
        }
        return (float)(1.0 / fr.samples) * color;
    }
};

} // namespace rto

using namespace rto;

extern "C" {

static void *create_common(const rt_scene_desc *d, bool hw7) {
    Scene *s = new Scene();
    s->hw7 = hw7; s->lightmix.hw7_geom_normal = hw7;
    s->figs.resize(d->n_triangles);
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        Fig &f = s->figs[i];
        Vertex *vs[3] = {&f.d, &f.d2, &f.d3};
        for (int k = 0; k < 3; k++) {
            vs[k]->coords = v3(d->positions + 9 * i + 3 * k);
            if (d->texcoords) { vs[k]->tu = d->texcoords[6 * i + 2 * k]; vs[k]->tv = d->texcoords[6 * i + 2 * k + 1]; }
            if (d->normals) vs[k]->normals = v3(d->normals + 9 * i + 3 * k);
            if (d->tangents) { vs[k]->tan = v3(d->tangents + 12 * i + 4 * k); vs[k]->tanw = d->tangents[12 * i + 4 * k + 3]; }
        }
        f.mat = d->material_index[i];
        f.orig = i;
    }
    s->mats.assign(d->materials, d->materials + d->n_materials);
    for (auto &m : s->mats) s->models.push_back(MaterialModel{m.metallic_factor, v3(m.base_color)});
    s->tex_source.assign(d->texture_source, d->texture_source + d->n_textures);
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rt_image &im = d->images[i];
        s->image_store.emplace_back(im.rgb, im.rgb + (size_t)im.width * im.height * 3);
    }
    for (uint32_t i = 0; i < d->n_images; i++) s->images.push_back(Tex{d->images[i].width, d->images[i].height, s->image_store[i].data()});
    if (d->environment_map) {
        const rt_image &im = *d->environment_map;
        s->image_store.emplace_back(im.rgb, im.rgb + (size_t)im.width * im.height * 3);
        s->env = Tex{im.width, im.height, s->image_store.back().data()};
        s->has_env = true;
    }
    s->camPos = v3(d->camera.position); s->camRight = v3(d->camera.right);
    s->camUp = v3(d->camera.up); s->camFwd = v3(d->camera.forward);
    s->fovY = d->camera.fov_y;
    s->bg = v3(d->bg_color);
    s->init();
    return s;
}
void *rto_hw8_create(const rt_scene_desc *d) { return create_common(d, false); }
// hw7 replay mode of the same code (pins the integrator structure)
void *rto_hw7_create(const rt_scene_desc *d) { return create_common(d, true); }
void rto_debug_bruteforce_lights(int on) { g_debug_bruteforce = on != 0; }
void rto_hw8_destroy(void *p) { delete (Scene *)p; }

uint32_t rto_hw8_num_lights(void *p) { return (uint32_t)((Scene *)p)->lightmix.lights.size(); }
// LOAD-order index of every light in light order / of every triangle in BVH order.
void rto_hw8_light_order(void *p, uint32_t *out) {
    Scene *s = (Scene *)p;
    for (size_t i = 0; i < s->lightmix.lights.size(); i++) out[i] = s->lightmix.lights[i].fig.orig;
}
void rto_hw8_figure_order(void *p, uint32_t *out) {
    Scene *s = (Scene *)p;
    for (size_t i = 0; i < s->figs.size(); i++) out[i] = s->figs[i].orig;
}
void rto_hw8_bvh_stats(void *p, uint32_t *out4) {
    Scene *s = (Scene *)p;
    out4[0] = (uint32_t)s->bvh.nodes.size(); out4[1] = s->bvh.depth;
    out4[2] = (uint32_t)s->lightmix.bvh.nodes.size(); out4[3] = s->lightmix.bvh.depth;
}

// Test hook for the product's throughput mode (include/rtamd.h: sample_streams): stream k of a pixel is an ordinary replay of
// the reference loop with the engine seeded y*width + x + k*width*height.  0 = the reference's seeding.
static uint32_t g_seed_offset = 0;
void rto_hw8_set_seed_offset(uint32_t off) { g_seed_offset = off; }

// Diagnostic: the closest-hit queries of one pixel's replay, 12 floats each (origin, direction, t or -1, figure index or -1, inside,
// texture u, v, remaining depth); returns the number of floats written (at most cap).
int rto_hw8_trace_pixel(void *p, int width, int height, int samples, int ray_depth, int x, int y, float *out, int cap) {
    const Scene *s = (const Scene *)p;
    const Frame fr{width, height, samples, ray_depth > 0 ? ray_depth : 6};
    std::vector<float> log;
    tl_trace = &log;
    rng_t rng((uint32_t)(y * width + x) + g_seed_offset);
    (void)s->get_pixel(fr, rng, x, y);
    tl_trace = nullptr;
    int n = (int)log.size() < cap ? (int)log.size() : cap;
    memcpy(out, log.data(), (size_t)n * sizeof(float));
    return n;
}

// Render the pixel rectangle [x0,x0+w) x [y0,y0+h) of a width x height image.
// out_rgb: w*h*3 linear float radiance (nullable); out8: w*h*3 tonemapped bytes (nullable).
// Mirrors the loop body of sceneio.cpp:387-396 (seed = y*width + x of the FULL image).
int rto_hw8_render(void *p, int width, int height, int samples, int ray_depth, int x0, int y0, int w, int h,
                   float *out_rgb, uint8_t *out8, int nthreads, Counters *cnt) {
    const Scene *s = (const Scene *)p;
    const Frame fr{width, height, samples, ray_depth > 0 ? ray_depth : 6};
    Counters total = render_rect(false, nthreads, x0, y0, w, h, out_rgb, out8,
                                 [&](int x, int y) { return rng_t((uint32_t)(y * width + x) + g_seed_offset); },
                                 [&](rng_t &rng, int x, int y) { return s->get_pixel(fr, rng, x, y); }, [] { return &tl_cnt; });
    if (cnt) *cnt = total;
    return 0;
}

// ---- per-function entry points for the reference pins (tests/test_oracle_ref.py) ---------------
// Closest hit of ray (o,d): returns BVH-order index or -1; out = t, ng(3), uv(2), ns(3), tan(3), tanw, inside
int rto_hw8_closest_hit(void *p, const float *o, const float *d, float *out14) {
    Scene *s = (Scene *)p;
    Hit h; int idx = -1;
    if (!s->bvh.intersect(s->figs, s->bvh.root, v3(o), v3(d), false, 0.f, h, idx)) return -1;
    float r[14] = {h.t, h.ng.x, h.ng.y, h.ng.z, h.tu, h.tv, h.ns.x, h.ns.y, h.ns.z, h.tan.x, h.tan.y, h.tan.z, h.tanw, h.inside ? 1.f : 0.f};
    memcpy(out14, r, sizeof r);
    return idx;
}
float rto_hw8_light_pdf(void *p, const float *x, const float *d) { return ((Scene *)p)->lightmix.pdf(v3(x), v3(d)); }
// ---- the intersection layer's two tests on their own (tests/intersection_cases.py), n rows each.
// rows12: mn, mx, o, d -> aabb_ray (oracle_bvh.h).  flags: 1 accepted | 2 inside; t: 0 for a rejected box.
void rto_box_test(const float *rows12, size_t n, uint32_t *flags, float *t) {
    for (size_t i = 0; i < n; i++) {
        const float *p = rows12 + 12 * i;
        float tt = 0; bool inside = false;
        const bool ok = aabb_ray(Box{v3(p), v3(p + 3)}, v3(p + 6), v3(p + 9), tt, inside);
        flags[i] = ok ? (1u | (inside ? 2u : 0u)) : 0u;
        t[i] = ok ? tt : 0.f;
    }
}
// rows15: the positions of data, data2, data3, then o, d -> tri_ray on a figure with texcoords (1,0), (0,1), (0,0), so that the hit's
// texcoords are 0 + u * 1 + v * 0 and 0 + u * 0 + v * 1.  flags: 1 hit | 2 inside; out3: t and the two texcoords (0 for a miss).
void rto_tri_test(const float *rows15, size_t n, uint32_t *flags, float *out3) {
    for (size_t i = 0; i < n; i++) {
        const float *p = rows15 + 15 * i;
        Fig f;
        f.d.coords = v3(p); f.d2.coords = v3(p + 3); f.d3.coords = v3(p + 6);
        f.d.tu = 1; f.d2.tv = 1;
        Hit h;
        const bool hit = tri_ray(f, v3(p + 9), v3(p + 12), h);
        flags[i] = hit ? (1u | (h.inside ? 2u : 0u)) : 0u;
        out3[3 * i] = hit ? h.t : 0.f; out3[3 * i + 1] = hit ? h.tu : 0.f; out3[3 * i + 2] = hit ? h.tv : 0.f;
    }
}
// Mix::sample then Mix::pdf with a fresh engine seeded `seed` after `burn` discarded uniform draws.
void rto_hw8_mix_sample_pdf(void *p, uint32_t seed, const float *x, const float *n, const float *v, float alpha, float *out_d3_pdf) {
    Scene *s = (Scene *)p;
    rng_t rng(seed); U01 u01(0.0, 1.0); N01 n01(0.0, 1.0);
    V3 d = s->mix_sample(u01, n01, rng, v3(x), v3(n), v3(v), alpha);
    float pdf = s->mix_pdf(v3(x), v3(n), d, v3(v), alpha);
    out_d3_pdf[0] = d.x; out_d3_pdf[1] = d.y; out_d3_pdf[2] = d.z; out_d3_pdf[3] = pdf;
    out_d3_pdf[4] = u01(rng); // stream position check
}
void rto_hw8_brdf(float base_metallic, const float *base_color, const float *l, const float *v, const float *n, const float *color,
                  float metallic, float alpha, float *out3) {
    MaterialModel m{base_metallic, v3(base_color)};
    V3 r = m.brdf(v3(l), v3(v), v3(n), v3(color), metallic, alpha);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
// ---- the shading layer's functions on their own (tests/shading_cases.py).  The samplers return the sample, the pdf of that sample
// and the next uniform draw of the engine (the stream position), as rto_hw8_mix_sample_pdf does.
void rto_hw8_vndf_sample_pdf(uint32_t seed, const float *n, const float *v, float alpha, float *out5) {
    rng_t rng(seed); U01 u01(0.0, 1.0);
    V3 d = Vndf::sample(u01, rng, v3(n), v3(v), alpha);
    float pdf = Vndf::pdf(v3(n), d, v3(v), alpha);
    out5[0] = d.x; out5[1] = d.y; out5[2] = d.z; out5[3] = pdf; out5[4] = u01(rng);
}
float rto_hw8_vndf_pdf(const float *n, const float *d, const float *v, float alpha) { return Vndf::pdf(v3(n), v3(d), v3(v), alpha); }
// Vndf::sample_ behind its two draws: (t1, t2) is the point on the disk, vT the view direction in the local frame
void rto_hw8_vndf_sample_local(float t1, float t2, const float *vT, float alpha, float *out3) {
    V3 r = Vndf::sample_local(t1, t2, v3(vT), alpha);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
void rto_hw8_cosine_sample_pdf(uint32_t seed, const float *n, float *out5) {
    rng_t rng(seed); U01 u01(0.0, 1.0); N01 n01(0.0, 1.0);
    V3 d = cosine_sample(n01, rng, v3(n));
    float pdf = cosine_pdf(v3(n), d);
    out5[0] = d.x; out5[1] = d.y; out5[2] = d.z; out5[3] = pdf; out5[4] = u01(rng);
}
float rto_hw8_cosine_pdf(const float *n, const float *d) { return cosine_pdf(v3(n), v3(d)); }
// hw7's MaterialModel(alpha, metallic, baseColor): the constructor squares alpha (hw7/src/include/material.h:42)
void rto_hw7_brdf(float alpha, float metallic, const float *base_color, const float *l, const float *v, const float *n, float *out3) {
    MaterialModel m{metallic, v3(base_color)};
    V3 r = m.brdf_hw7(v3(l), v3(v), v3(n), alpha * alpha);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
// dot(h, l) and dot(h, v) of specularBrdf (material.h:24-25) for n pairs (l, v: n x 3; out: n x 2): what its 1e-4 gate compares, so
// that the cases can be put on the gate's threshold to the bit
void rto_hw8_half_dots(const float *l, const float *v, float *out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        V3 h = normalize(v3(l + 3 * i) + v3(v + 3 * i));
        out[2 * i] = dot(h, v3(l + 3 * i)); out[2 * i + 1] = dot(h, v3(v + 3 * i));
    }
}
void rto_tonemap(const float *rgb, uint8_t *out3) { to_extern(gamma_corrected(aces_tonemap(v3(rgb))), out3); }
// Host libm cos / sin on doubles (what the reference's Vndf::sample_ calls, distributions.h:183-184).  numpy's own may be a SIMD
// implementation that is not glibc's.
void rto_cos_array(const double *in, double *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = std::cos(in[i]); }
void rto_sin_array(const double *in, double *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = std::sin(in[i]); }
void rto_sample_texture(int w, int h, const uint8_t *data, float tx, float ty, int srgb, float *out3) {
    V3 r = sample_texture(tx, ty, Tex{w, h, data}, srgb != 0);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
void rto_apply_normal_map(const float *sn3, const float *tan4, const float *sample3, float *out3) {
    V3 r = apply_normal_map(v3(sn3), v3(tan4), tan4[3], v3(sample3));
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
// RNG known-answer helper: seed, then n_u uniforms followed by n_n normals.
void rto_rng_kat(uint32_t seed, int n_u, int n_n, float *out) {
    rng_t rng(seed); U01 u01(0.0, 1.0); N01 n01(0.0, 1.0);
    for (int i = 0; i < n_u; i++) out[i] = u01(rng);
    for (int i = 0; i < n_n; i++) out[n_u + i] = n01(rng);
}
// Host libm logf (what the reference's normal_distribution calls) on an array.
void rto_logf_array(const float *in, float *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = std::log(in[i]); }
// Host libm atan2f / asinf (what the reference's environment lookup calls on floats) on arrays.
void rto_atan2f_array(const float *y, const float *x, float *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = std::atan2(y[i], x[i]); }
void rto_asinf_array(const float *in, float *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = std::asin(in[i]); }
// The oracle's environment-map uv for n directions (d: n x 3, uv: n x 2).
void rto_hw8_env_uv(const float *d, float *uv, size_t n) {
    for (size_t i = 0; i < n; i++) env_uv(V3{d[3 * i], d[3 * i + 1], d[3 * i + 2]}, uv[2 * i], uv[2 * i + 1]);
}
// Same engine, normals drawn first, then uniforms.
void rto_rng_kat_normals_first(uint32_t seed, int n_n, int n_u, float *out) {
    rng_t rng(seed); U01 u01(0.0, 1.0); N01 n01(0.0, 1.0);
    for (int i = 0; i < n_n; i++) out[i] = n01(rng);
    for (int i = 0; i < n_u; i++) out[n_n + i] = u01(rng);
}

} // extern "C"

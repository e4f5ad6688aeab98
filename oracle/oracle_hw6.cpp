// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the hw6 render path (BASELINE.json configs[2]: glTF triangles, DIFFUSE / METALLIC /
// DIELECTRIC materials, Mix{Cosine, FiguresMix}, branching dielectric recursion) in exact-replay semantics.
// glTF scenes contain triangles only (hw6/src/sceneio.cpp:214), so the ELLIPSOID / BOX / PLANE figure types and
// their lights (hw6/src/include/distributions.h:61-105,142-172) are not restated; every figure has
// position (0,0,0) and the identity rotation, whose quaternion arithmetic is nevertheless carried out literally.
// Pinned bit-exact against the compiled hw6 reference (oracle/ref/ref_hw6_scene.cpp, tests/test_oracle_pins.py).
#include "oracle_bvh.h"

namespace rto6 {
using namespace rto;

static const float T_MAX = 1e4;               // hw6/src/primitives.cpp:11
static const long double eps_ld = 1e-4;       // hw6/src/include/primitives.h:9

struct Fig {                                   // hw6/src/include/primitives.h:33-55 (TRIANGLE only)
    V3 position;                               // (0,0,0)
    Quat rotation;                             // identity
    V3 data, data2, data3;
    uint32_t mat = 0, orig = 0;
};
struct Hit { float t; V3 norma; bool inside; };
static thread_local Counters tl_cnt;

static inline V3 rotate(Quat q, V3 p) { return qtransform(q, p); }

// primitives.cpp:77-86
static inline bool plane_ray(V3 n, V3 o, V3 d, Hit &h) {
    float t = -dot(o, n) / dot(d, n);
    if (t > 0 && t < T_MAX) {
        if (dot(d, n) > 0) { h = Hit{t, neg1(n), true}; return true; }
        h = Hit{t, n, false};
        return true;
    }
    return false;
}
// primitives.cpp:143-164
static inline bool tri_ray_local(const Fig &f, V3 o, V3 d, Hit &h) {
    V3 a = f.data3, b = f.data - a, c = f.data2 - a;
    V3 n = crossr(b, c);
    if (!plane_ray(n, o - a, d, h)) return false;
    V3 p = o - a + h.t * d;
    if (dot(crossr(b, p), n) < 0) return false;
    if (dot(crossr(p, c), n) < 0) return false;
    if (dot(crossr(c - b, p - b), n) < 0) return false;
    return true;
}
// primitives.cpp:13-33
static bool fig_ray(const Fig &f, V3 o, V3 d, Hit &h) {
    tl_cnt.tris++;
    V3 to = rotate(f.rotation, o - f.position), td = rotate(f.rotation, d);
    if (!tri_ray_local(f, to, td, h)) return false;
    h.norma = normalize(rotate(qconj(f.rotation), h.norma));
    return true;
}
// hw6/src/include/bvh.h — the shared builder.  The sort key is Figure::position (:61-63), which is (0,0,0) for every glTF
// triangle: the comparator is always false and std::sort leaves whatever permutation introsort produces on all-equal keys.
struct Tree6 {
    typedef rto6::Hit Hit;
    // primitives.cpp:169-199 (TRIANGLE branch + the rotate-8-corners step, carried out literally)
    static Box box_of(const Fig &f) {
        Box u;
        u.mn = {smin(f.data3.x, smin(f.data.x, f.data2.x)), smin(f.data3.y, smin(f.data.y, f.data2.y)), smin(f.data3.z, smin(f.data.z, f.data2.z))};
        u.mx = {smax(f.data3.x, smax(f.data.x, f.data2.x)), smax(f.data3.y, smax(f.data.y, f.data2.y)), smax(f.data3.z, smax(f.data.z, f.data2.z))};
        Quat r = qconj(f.rotation);
        Box b;
        b.mn = b.mx = rotate(r, u.mn);
        extend(b, rotate(r, V3{u.mn.x, u.mn.y, u.mx.z}));
        extend(b, rotate(r, V3{u.mn.x, u.mx.y, u.mn.z}));
        extend(b, rotate(r, V3{u.mn.x, u.mx.y, u.mx.z}));
        extend(b, rotate(r, V3{u.mx.x, u.mn.y, u.mn.z}));
        extend(b, rotate(r, V3{u.mx.x, u.mn.y, u.mx.z}));
        extend(b, rotate(r, V3{u.mx.x, u.mx.y, u.mn.z}));
        extend(b, rotate(r, V3{u.mx.x, u.mx.y, u.mx.z}));
        b.mn = b.mn + f.position;
        b.mx = b.mx + f.position;
        return b;
    }
    static V3 key(const Fig &f) { return f.position; }
    static bool hit(const Fig &f, V3 o, V3 d, Hit &h) { return fig_ray(f, o, d, h); }
    static void count_box() { tl_cnt.boxes++; }
};
typedef rto::Bvh<Fig, Tree6> Bvh;

struct TriLight {                              // distributions.h:107-143
    float pointProb;
    Fig fig;
    explicit TriLight(const Fig &f) : fig(f) {
        V3 a = fig.data3, b = fig.data - a, c = fig.data2 - a;
        pointProb = 1.0 / (0.5 * len(crossr(b, c)));
    }
    float pdfOne(V3 x, V3 d, V3 y, V3 yn) const { return pointProb * len2(x - y) / std::fabs((double)dot(d, yn)); }
    V3 sample(U01 &u01, rng_t &rng, V3 x) const {
        V3 a = fig.data3, b = fig.data - a, c = fig.data2 - a;
        float u = u01(rng);
        float v = u01(rng);
        if (u + v > 1.) { u = 1 - u; v = 1 - v; }
        V3 point = fig.position + rotate(qconj(fig.rotation), a + u * b + v * c);
        return normalize(point - x);
    }
};

struct Scene {
    std::vector<Fig> figs;
    std::vector<rt_material> mats;
    std::vector<TriLight> lights;
    Bvh bvh, lbvh;
    V3 camPos, camRight, camUp, camFwd, bg;
    float fovY = 0;
    int n_components = 1;

    void init() {
        // scene.cpp:18-23: partition non-planes first (all figures are triangles -> every predicate is true)
        std::partition(figs.begin(), figs.end(), [](const Fig &) { return true; });
        bvh.init(figs, (uint32_t)figs.size());
        std::vector<Fig> copy = figs;                                              // distributions.h:180 (by value)
        size_t n = std::partition(copy.begin(), copy.end(), [this](const Fig &f) {
            const rt_material &m = mats[f.mat];
            return !(m.emission[0] == 0 && m.emission[1] == 0 && m.emission[2] == 0);
        }) - copy.begin();
        lbvh.init(copy, (uint32_t)n);
        for (size_t i = 0; i < n; i++) lights.push_back(TriLight(copy[i]));
        n_components = lights.empty() ? 1 : 2;                                     // scene.cpp:8-16
    }
    float pdf_one(const TriLight &tl, V3 x, V3 d) const {                          // distributions.h:212-237
        Hit h;
        if (!fig_ray(tl.fig, x, d, h)) return 0.;
        if (std::isnan(h.t)) return INFINITY;
        V3 y = x + h.t * d;
        return tl.pdfOne(x, d, y, h.norma);
    }
    V3 mix_sample(U01 &u01, N01 &n01, rng_t &rng, V3 x, V3 n) const {              // :283-290
        int k = u01(rng) * (size_t)n_components;
        if (k == 0) return cosine_sample(n01, rng, n);
        int li = u01(rng) * lights.size();                                         // :199-208
        return lights[li].sample(u01, rng, x);
    }
    float mix_pdf(V3 x, V3 n, V3 d) const {                                        // :292-302
        float ans = 0;
        ans += cosine_pdf(n, d);
        if (n_components == 2) {                                                   // getTotalPdf :239-256
            tl_cnt.lightq++;
            ans += lbvh.total_pdf(0, x, d, [&](uint32_t i) { return pdf_one(lights[i], x, d); }) / lights.size();
        }
        return ans / (size_t)n_components;
    }
    // scene.cpp:47-105
    V3 get_color(U01 &u01, N01 &n01, rng_t &rng, V3 ro, V3 rd, int recLimit) const {
        if (recLimit == 0) return V3{0., 0., 0.};
        Hit h; int idx = -1;
        tl_cnt.closest++;
        if (!bvh.intersect(figs, bvh.root, ro, rd, false, 0.f, h, idx)) return bg;
        const rt_material &m = mats[figs[idx].mat];
        V3 emission{m.emission[0], m.emission[1], m.emission[2]}, color{m.base_color[0], m.base_color[1], m.base_color[2]};
        V3 x = ro + h.t * rd;
        V3 norma = h.norma;
        if (m.kind == RT_MAT_DIFFUSE) {
            V3 xo = x + (float)eps_ld * norma;
            V3 d = mix_sample(u01, n01, rng, xo, norma);
            if (dot(d, norma) < 0) return emission;
            float pdf = mix_pdf(xo, norma, d);
            V3 no = x + (float)eps_ld * d;
            float k = 1. / (PI * pdf) * dot(d, norma);
            return emission + (k * color) * get_color(u01, n01, rng, no, d, recLimit - 1);
        }
        return specular_tail(h.t, norma, h.inside, ro, rd, color, emission, m.kind, m.ior, (float)eps_ld, [&] { return u01(rng); },
                             [&](V3 o, V3 d) { return get_color(u01, n01, rng, o, d, recLimit - 1); });
    }
    // scene.cpp:107-127 (camera direction is NOT normalised in hw6)
    V3 get_pixel(const Frame &fr, rng_t &rng, int x, int y) const {
        U01 u01(0.0, 1.0);
        N01 n01(0.0, 1.0);
        V3 color{0, 0, 0};
        for (int s = 0; s < fr.samples; s++) {
            float nx = x + u01(rng);
            float ny = y + u01(rng);
            float tanFovY = std::tan((double)(fovY / 2));
            float tanFovX = tanFovY * fr.width / fr.height;
            float cx = tanFovX * (2 * nx / fr.width - 1);
            float cy = tanFovY * (2 * ny / fr.height - 1);
            color = color + get_color(u01, n01, rng, camPos, cx * camRight - cy * camUp + camFwd, fr.ray_depth);
        }
        return (float)(1.0 / fr.samples) * color;
    }
};
} // namespace rto6

using namespace rto6;
extern "C" {
void *rto_hw6_create(const rt_scene_desc *d) {
    Scene *s = new Scene();
    s->figs.resize(d->n_triangles);
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        Fig &f = s->figs[i];
        f.data = v3(d->positions + 9 * i); f.data2 = v3(d->positions + 9 * i + 3); f.data3 = v3(d->positions + 9 * i + 6);
        f.mat = d->material_index[i]; f.orig = i;
    }
    s->mats.assign(d->materials, d->materials + d->n_materials);
    s->camPos = v3(d->camera.position); s->camRight = v3(d->camera.right); s->camUp = v3(d->camera.up); s->camFwd = v3(d->camera.forward);
    s->fovY = d->camera.fov_y; s->bg = v3(d->bg_color);
    s->init();
    return s;
}
void rto_hw6_destroy(void *p) { delete (Scene *)p; }
uint32_t rto_hw6_num_lights(void *p) { return (uint32_t)((Scene *)p)->lights.size(); }
void rto_hw6_light_order(void *p, uint32_t *out) { Scene *s = (Scene *)p; for (size_t i = 0; i < s->lights.size(); i++) out[i] = s->lights[i].fig.orig; }
void rto_hw6_figure_order(void *p, uint32_t *out) { Scene *s = (Scene *)p; for (size_t i = 0; i < s->figs.size(); i++) out[i] = s->figs[i].orig; }
void rto_hw6_bvh_stats(void *p, uint32_t *out4) {
    Scene *s = (Scene *)p;
    out4[0] = (uint32_t)s->bvh.nodes.size(); out4[1] = s->bvh.depth; out4[2] = (uint32_t)s->lbvh.nodes.size(); out4[3] = s->lbvh.depth;
}
// Test hook for throughput mode (rt_render_params.sample_streams): stream k of a pixel is the reference's per-pixel loop with the engine
// seeded y*W+x + k*W*H instead of y*W+x (hw6/src/sceneio.cpp:280-284 seeds with y*W+x).
static uint32_t g_seed_offset6 = 0;
void rto_hw6_set_seed_offset(uint32_t off) { g_seed_offset6 = off; }
int rto_hw6_render(void *p, int width, int height, int samples, int ray_depth, int x0, int y0, int w, int h, float *out_rgb, uint8_t *out8,
                   int nthreads, Counters *cnt) {
    const Scene *s = (const Scene *)p;
    const Frame fr{width, height, samples, ray_depth > 0 ? ray_depth : 6};
    Counters total = render_rect(false, nthreads, x0, y0, w, h, out_rgb, out8,
                                 [&](int x, int y) { return rng_t((uint32_t)(y * width + x) + g_seed_offset6); },  // hw6/src/sceneio.cpp:280-284
                                 [&](rng_t &rng, int x, int y) { return s->get_pixel(fr, rng, x, y); }, [] { return &tl_cnt; });
    if (cnt) *cnt = total;
    return 0;
}
}

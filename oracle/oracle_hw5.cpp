// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the hw5 snapshot: analytic primitives + TRIANGLE figures (each with its own position/rotation),
// a SAH BVH over the non-plane figures sorted by Figure::position, Mix{Cosine, FiguresMix{Box|Ellipsoid|Triangle lights
// behind their own BVH}} and — from this snapshot on — one engine per pixel, rng_type rng(y*W+x)
// (hw5/src/scene.cpp:8-126, hw5/src/primitives.cpp:12-222, hw5/src/include/bvh.h:18-141,
//  hw5/src/include/distributions.h:15-302, hw5/src/sceneio.cpp:103-123).
// `eps` is a LONG DOUBLE constant in this snapshot (primitives.h:9): (t + eps) is an x87 80-bit sum narrowed to float.
#include "oracle_txt_prims.h"
#include "oracle_bvh.h"

namespace rto5 {
using namespace rtot;

static const long double eps = 1e-4;     // primitives.h:9
static const float T_MAX = 1e4;          // primitives.cpp:11

struct Fig {
    int type; V3 data, data2, data3, position; Quat rotation; V3 color, emission; int kind; float ior;
    uint32_t load_index;
};

// intersectPlaneAndRay, primitives.cpp:76-85
static bool plane_ray(V3 n, V3 o, V3 d, Hit &h) {
    float t = -dot(o, n) / dot(d, n);
    if (t > 0 && t < T_MAX) {
        h = dot(d, n) > 0 ? Hit{t, neg1(n), true} : Hit{t, n, false};
        return true;
    }
    return false;
}
// Figure::intersect, primitives.cpp:13-35 and the four intersectAs* (:57-166)
static bool fig_ray(const Fig &f, V3 o, V3 d, Hit &h) {
    V3 to = qtransform(f.rotation, o - f.position), td = qtransform(f.rotation, d);
    bool ok;
    if (f.type == RT_PRIM_ELLIPSOID) {
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
    } else if (f.type == RT_PRIM_PLANE) ok = plane_ray(f.data, to, td, h);
    else if (f.type == RT_PRIM_BOX) ok = box_local(f.data, to, td, h);        // intersectBoxAndRay, :91-137
    else {                                                                 // :143-166
        V3 a = f.data3, b = f.data - a, c = f.data2 - a;
        V3 n = crossr(b, c);
        ok = plane_ray(n, to - a, td, h);
        if (ok) {
            V3 p = to - a + h.t * td;
            if (dot(crossr(b, p), n) < 0) ok = false;
            else if (dot(crossr(p, c), n) < 0) ok = false;
            else if (dot(crossr(c - b, p - b), n) < 0) ok = false;
        }
    }
    if (!ok) return false;
    h.norma = normalize(qtransform(qconj(f.rotation), h.norma));
    return true;
}

// bvh.h:18-141: the shared builder, sorted on Figure::position
struct Tree5 {
    typedef rtot::Hit Hit;
    // AABB::AABB(const Figure&), primitives.cpp:171-201: local extent, its 8 corners rotated back, then translated
    static Box box_of(const Fig &f) {
        Box u;
        if (f.type == RT_PRIM_BOX || f.type == RT_PRIM_ELLIPSOID) { u.mn = (float)(-1.) * f.data; u.mx = f.data; }
        else {
            u.mn = {smin(f.data3.x, smin(f.data.x, f.data2.x)), smin(f.data3.y, smin(f.data.y, f.data2.y)), smin(f.data3.z, smin(f.data.z, f.data2.z))};
            u.mx = {smax(f.data3.x, smax(f.data.x, f.data2.x)), smax(f.data3.y, smax(f.data.y, f.data2.y)), smax(f.data3.z, smax(f.data.z, f.data2.z))};
        }
        Quat r = qconj(f.rotation);
        Box b;
        b.mn = b.mx = qtransform(r, u.mn);
        extend(b, qtransform(r, V3{u.mn.x, u.mn.y, u.mx.z}));
        extend(b, qtransform(r, V3{u.mn.x, u.mx.y, u.mn.z}));
        extend(b, qtransform(r, V3{u.mn.x, u.mx.y, u.mx.z}));
        extend(b, qtransform(r, V3{u.mx.x, u.mn.y, u.mn.z}));
        extend(b, qtransform(r, V3{u.mx.x, u.mn.y, u.mx.z}));
        extend(b, qtransform(r, V3{u.mx.x, u.mx.y, u.mn.z}));
        extend(b, qtransform(r, V3{u.mx.x, u.mx.y, u.mx.z}));
        b.mn = b.mn + f.position;
        b.mx = b.mx + f.position;
        return b;
    }
    static V3 key(const Fig &f) { return f.position; }
    static bool hit(const Fig &f, V3 o, V3 d, Hit &h) { return fig_ray(f, o, d, h); }
    static void count_box() {}
};
typedef rto::Bvh<Fig, Tree5> Bvh;

// ---- distributions.h -------------------------------------------------------------------------------------------
struct Light {
    Fig fig;
    float pointProb = 0;                                             // TriangleLight :121-127
    explicit Light(const Fig &f) : fig(f) {
        if (f.type == RT_PRIM_TRIANGLE) {
            V3 a = f.data3, b = f.data - a, c = f.data2 - a;
            V3 n = crossr(b, c);
            pointProb = 1.0 / (0.5 * (double)len(n));
        }
    }
    float pdf_one(V3 x, V3 d, V3 y, V3 yn) const {
        if (fig.type == RT_PRIM_BOX) return box_emitter_pdf_one(fig, x, d, y, yn);
        if (fig.type == RT_PRIM_TRIANGLE) return (double)(pointProb * len2(x - y)) / std::fabs((double)dot(d, yn)); // :117-119
        return ellipsoid_emitter_pdf_one(fig, x, d, y, yn);
    }
    typedef bool (*RayFn)(const Fig &, V3, V3, Hit &);
    template <class R = RayFn> V3 sample(U01 &u01, N01 &n01, rng_t &rng, V3 x, R &&ray = Tree5::hit) const {
        if (fig.type == RT_PRIM_TRIANGLE) {                                // :129-142
            V3 a = fig.data3, b = fig.data - a, c = fig.data2 - a;
            float u = u01(rng);
            float v = u01(rng);
            if ((double)(u + v) > 1.) { u = 1 - u; v = 1 - v; }
            V3 point = fig.position + qtransform(qconj(fig.rotation), a + u * b + v * c);
            return normalize(point - x);
        }
        if (fig.type == RT_PRIM_BOX) return box_emitter_sample(fig, u01, rng, x, ray);
        return ellipsoid_emitter_sample(fig, n01, rng, x, ray);
    }
};

struct Scene5 {
    std::vector<Fig> figs;      // after initBVH: [0, nonPlanes) in BVH order, planes after
    uint32_t nonPlanes = 0;
    Bvh bvh;
    std::vector<Light> lights;  // FiguresMix::figures_
    Bvh light_bvh;
    V3 camPos, camRight, camUp, camFwd, bg;
    float fovX = 0;

    void init() {
        // Scene::initBVH, scene.cpp:18-23
        nonPlanes = (uint32_t)(std::partition(figs.begin(), figs.end(), [](const Fig &e) { return e.type != RT_PRIM_PLANE; }) - figs.begin());
        bvh.init(figs, nonPlanes);
        // FiguresMix::FiguresMix on a COPY of the reordered figures, distributions.h:180-198
        std::vector<Fig> copy = figs;
        size_t n = std::partition(copy.begin(), copy.end(), [](const Fig &f) {
            if (f.emission.x == 0 && f.emission.y == 0 && f.emission.z == 0) return false;
            return f.type == RT_PRIM_BOX || f.type == RT_PRIM_ELLIPSOID || f.type == RT_PRIM_TRIANGLE;
        }) - copy.begin();
        light_bvh.init(copy, (uint32_t)n);
        for (size_t i = 0; i < n; i++) lights.push_back(Light(copy[i]));
    }
    // Scene::intersect, scene.cpp:25-45
    bool intersect(V3 o, V3 d, Hit &best, int &pos) const {
        bool have = false;
        for (int i = (int)nonPlanes; i < (int)figs.size(); i++) {
            Hit h;
            if (fig_ray(figs[i], o, d, h) && (!have || h.t < best.t)) { best = h; pos = i; have = true; }
        }
        Hit bh; int bi = -1;
        if (bvh.intersect(figs, 0, o, d, have, have ? best.t : 0.f, bh, bi) && (!have || bh.t < best.t)) { best = bh; pos = bi; have = true; }
        return have;
    }
    // FiguresMix::pdfOneFigureLight, distributions.h:219-254
    float light_pdf_one(const Light &L, V3 x, V3 d) const {
        Hit h1;
        if (!fig_ray(L.fig, x, d, h1)) return 0.;
        if (std::isnan(h1.t)) return INFINITY;
        V3 y = x + h1.t * d;
        float ans = L.pdf_one(x, d, y, h1.norma);
        if (L.fig.type == RT_PRIM_TRIANGLE) return ans;
        Hit h2;
        if (!fig_ray(L.fig, x + (float)((long double)h1.t + eps) * d, d, h2)) return ans;
        V3 y2 = x + (float)((long double)h1.t + eps + (long double)h2.t) * d;
        return ans + L.pdf_one(x, d, y2, h2.norma);
    }
    V3 mix_sample(U01 &u01, N01 &n01, rng_t &rng, V3 x, V3 n) const { // Mix::sample :283-290, FiguresMix::sample :200-209
        size_t comps = lights.empty() ? 1 : 2;
        int distNum = u01(rng) * comps;
        if (distNum == 0) return cosine_sample(n01, rng, n);
        int li = u01(rng) * lights.size();
        return lights[li].sample(u01, n01, rng, x);
    }
    float mix_pdf(V3 x, V3 n, V3 d) const { // Mix::pdf :292-302, FiguresMix::pdf :211-213
        float ans = 0;
        ans += cosine_pdf(n, d);
        if (lights.empty()) return ans / (size_t)1;
        ans += light_bvh.total_pdf(0, x, d, [&](uint32_t i) { return light_pdf_one(lights[i], x, d); }) / lights.size(); // getTotalPdf :256-274
        return ans / (size_t)2;
    }
    // Scene::getColor, scene.cpp:47-103
    V3 get_color(U01 &u01, N01 &n01, rng_t &rng, V3 ro, V3 rd, int recLimit) const {
        if (recLimit == 0) return V3{0., 0., 0.};
        Hit h; int pos = -1;
        if (!intersect(ro, rd, h, pos)) return bg;
        const Fig &f = figs[pos];
        float t = h.t; V3 norma = h.norma;
        V3 x = ro + t * rd;
        const float epsf = (float)eps;
        if (f.kind == RT_MAT_DIFFUSE) {
            V3 d = mix_sample(u01, n01, rng, x + epsf * norma, norma);
            if (dot(d, norma) < 0) return f.emission;
            float pdf = mix_pdf(x + epsf * norma, norma, d);
            V3 inner = get_color(u01, n01, rng, x + epsf * d, d, recLimit - 1);
            return f.emission + (float)(1. / (double)(PI * pdf) * (double)dot(d, norma)) * f.color * inner;
        }
        return specular_tail(t, norma, h.inside, ro, rd, f.color, f.emission, f.kind, f.ior, epsf, [&] { return u01(rng); },
                             [&](V3 o, V3 d) { return get_color(u01, n01, rng, o, d, recLimit - 1); });
    }
    // scene.cpp:105-126
    V3 get_pixel(const Frame &fr, rng_t &rng, int x, int y) const {
        U01 u01(0.0, 1.0); N01 n01(0.0, 1.0);
        V3 color{0, 0, 0};
        float tanFovX = std::tan((double)(fovX / 2));
        float tanFovY = tanFovX * fr.height / fr.width;
        for (int s = 0; s < fr.samples; s++) {
            float fx = x + u01(rng);
            float fy = y + u01(rng);
            float nx = tanFovX * (2 * fx / fr.width - 1);
            float ny = tanFovY * (2 * fy / fr.height - 1);
            color = color + get_color(u01, n01, rng, camPos, nx * camRight - ny * camUp + camFwd, fr.ray_depth);
        }
        return (float)(1.0 / fr.samples) * color;
    }
};
} // namespace rto5

using namespace rto5;
extern "C" {
void *rto_hw5_create(const rt_scene_desc *d) {
    Scene5 *s = new Scene5();
    for (uint32_t i = 0; i < d->n_primitives; i++) {
        const rt_primitive &p = d->primitives[i];
        Fig f;
        f.type = p.type; f.data = v3(p.data); f.data2 = v3(p.data2); f.data3 = v3(p.data3); f.position = v3(p.position);
        f.rotation = Quat{v3(p.rotation), p.rotation[3]};
        f.color = v3(p.color); f.emission = v3(p.emission); f.kind = p.kind; f.ior = p.ior; f.load_index = i;
        s->figs.push_back(f);
    }
    s->camPos = v3(d->camera.position); s->camRight = v3(d->camera.right); s->camUp = v3(d->camera.up); s->camFwd = v3(d->camera.forward);
    s->fovX = d->camera.fov_x; s->bg = v3(d->bg_color);
    s->init();
    return s;
}
void rto_hw5_destroy(void *p) { delete (Scene5 *)p; }
uint32_t rto_hw5_num_lights(void *p) { return (uint32_t)((Scene5 *)p)->lights.size(); }
// figure order after initBVH and light order (indices into the LOAD-order primitive array)
void rto_hw5_orders(void *p, uint32_t *figure_order, uint32_t *light_order) {
    Scene5 *s = (Scene5 *)p;
    for (size_t i = 0; i < s->figs.size(); i++) figure_order[i] = s->figs[i].load_index;
    for (size_t i = 0; i < s->lights.size(); i++) light_order[i] = s->lights[i].fig.load_index;
}
// Function-level entry points (rows and answers as oracle_txt_prims.h describes them; tests/analytic_cases.py).
static Fig fig_of_row(const float *r) {
    Fig f;
    f.type = (int)r[R_TYPE]; f.data = v3(r + R_DATA); f.data2 = v3(r + R_DATA2); f.data3 = v3(r + R_DATA3); f.position = v3(r + R_POS);
    f.rotation = Quat{v3(r + R_ROT), r[R_ROT + 3]};
    f.color = V3{1, 1, 1}; f.emission = V3{1, 1, 1}; f.kind = RT_MAT_DIFFUSE; f.ior = 1; f.load_index = 0;
    return f;
}
void rto_hw5_fig(const float *rows, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        Hit h;
        put_hit(fig_ray(fig_of_row(r), v3(r + R_O), v3(r + R_D), h), h, out + 5 * i);
    }
}
// FiguresMix::pdfOneFigureLight of the row's figure as a light, x = o.  out: 1 word
void rto_hw5_lpdf(const float *rows, size_t n, uint32_t *out) {
    Scene5 s;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        out[i] = word(s.light_pdf_one(Light(fig_of_row(r)), v3(r + R_O), v3(r + R_D)));
    }
}
// pdfOne(x, d, y, yn) of the row's figure as a light on a y and yn of the row's own (30 floats: the figure row, y 3, yn 3).  out: 1 word
void rto_hw5_pdf_one(const float *rows30, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows30 + 30 * i;
        out[i] = word(Light(fig_of_row(r)).pdf_one(v3(r + R_O), v3(r + R_D), v3(r + 24), v3(r + 27)));
    }
}
// The light's sample(x), engine seeded aux[0], the caller's normal_distribution primed by aux[1].  out: 8 words (put_sample).  A row that
// asks the figure more than max_attempts times gets zeros; returns the number of such rows.  attempts (may be null): the figure tests per row.
int rto_hw5_lsample(const float *rows, const uint32_t *aux, size_t n, uint32_t max_attempts, uint32_t *out, uint32_t *attempts) {
    int over = 0;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        const Light L(fig_of_row(r));
        rng_t rng(aux[2 * i]);
        U01 u01(0.0, 1.0);
        const N01 before = primed(aux[2 * i + 1]);
        N01 n01 = before;
        CountedRay<Light::RayFn> ray{Tree5::hit, max_attempts};
        try {
            const V3 d = L.sample(u01, n01, rng, v3(r + R_O), ray);
            put_sample(d, rng, n01, before, out + 8 * i);
        } catch (const TooManyAttempts &) { memset(out + 8 * i, 0, 32); over++; }
        if (attempts) attempts[i] = max_attempts - ray.left;
    }
    return over;
}
// Cosine::sample(n), engine seeded aux[0], the pixel's normal_distribution primed by aux[1].  out: 8 words (put_sample)
void rto_hw5_cosine(const float *normals, const uint32_t *aux, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        rng_t rng(aux[2 * i]);
        const N01 before = primed(aux[2 * i + 1]);
        N01 n01 = before;
        const V3 d = cosine_sample(n01, rng, v3(normals + 3 * i));
        put_sample(d, rng, n01, before, out + 8 * i);
    }
}
int rto_hw5_render(void *p, int width, int height, int samples, int ray_depth, int x0, int y0, int w, int h, float *out_rgb, uint8_t *out8, int nthreads) {
    const Scene5 *s = (const Scene5 *)p;
    const Frame fr{width, height, samples, ray_depth};
    render_rect(false, nthreads, x0, y0, w, h, out_rgb, out8, [&](int x, int y) { return rng_t(y * width + x); },  // hw5/src/sceneio.cpp:110
                [&](rng_t &rng, int x, int y) { return s->get_pixel(fr, rng, x, y); });
    return 0;
}
}

// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the hw4 snapshot: hw3's path tracer over analytic primitives with importance sampling —
// Mix{Cosine, Mix{BoxLight | EllipsoidLight ...}} (hw4/src/scene.cpp:10-122, hw4/src/include/distributions.h:13-204).
//
// hw4 still draws every random number of the frame from ONE file-static minstd_rand (hw4/src/scene.cpp:5-6), and each
// distribution object owns its own std::normal_distribution (whose cached second value survives between calls:
// Cosine's at distributions.h:48, every EllipsoidLight's at :156).  seed_mode 0 replays exactly that, sequentially
// (pinned bit for bit against the compiled hw4 sources); seed_mode 1 gives every pixel a fresh engine(y*W+x) and fresh
// distribution objects — the form a parallel machine can run, used to check the GPU.
#include "oracle_txt_prims.h"

namespace rto4 {
using namespace rtot;

struct Sampler { // all mutable sampling state of one replay stream
    rng_t rng;
    U01 u01{0.0, 1.0};            // scene.cpp:6 and the (stateless) copies inside Mix / BoxLight
    N01 cosine_n01{0.f, 1.f};     // Cosine::n01
    std::vector<N01> light_n01;   // EllipsoidLight::n01, one per light (unused for boxes)
};

struct Scene4 {
    std::vector<Prim> figs;
    std::vector<int> lights; // indices of emissive BOX / ELLIPSOID figures in figure order (scene.cpp:12-21)
    V3 camPos, camRight, camUp, camFwd, bg;
    float fovX = 0;

    bool intersect(V3 o, V3 d, Hit &best, int &pos) const { // scene.cpp:31-49
        pos = -1;
        for (int i = 0; i < (int)figs.size(); i++) {
            Hit h;
            if (prim_ray3(figs[i], o, d, h, true) && h.t <= INFINITY && (pos == -1 || h.t < best.t)) { best = h; pos = i; }
        }
        return pos != -1;
    }

    // ---- distributions.h ---------------------------------------------------------------------------------------
    struct Ray { bool operator()(const Prim &f, V3 o, V3 d, Hit &h) const { return prim_ray3(f, o, d, h, true); } };
    float pdf_one(const Prim &f, V3 x, V3 d, V3 y, V3 yn) const {
        return f.type == RT_PRIM_BOX ? box_emitter_pdf_one(f, x, d, y, yn) : ellipsoid_emitter_pdf_one(f, x, d, y, yn);
    }
    float light_pdf(const Prim &f, V3 x, V3 d) const { // FigureLight::pdf :85-107
        Hit h1;
        if (!prim_ray3(f, x, d, h1, true)) return 0.;
        if (std::isnan(h1.t)) return INFINITY;
        V3 y = x + h1.t * d;
        float ans = pdf_one(f, x, d, y, h1.norma);
        Hit h2;
        if (!prim_ray3(f, x + (float)((double)h1.t + 0.0001) * d, d, h2, true)) return ans;
        V3 y2 = x + (float)((double)h1.t + 0.0001 + (double)h2.t) * d;
        return ans + pdf_one(f, x, d, y2, h2.norma);
    }
    template <class R = Ray> V3 light_sample(Sampler &S, int li, V3 x, R &&ray = R()) const { // each EllipsoidLight draws from its own normal_distribution
        const Prim &f = figs[lights[li]];
        if (f.type == RT_PRIM_BOX) return box_emitter_sample(f, S.u01, S.rng, x, ray);
        return ellipsoid_emitter_sample(f, S.light_n01[li], S.rng, x, ray);
    }
    V3 mix_sample(Sampler &S, V3 x, V3 n) const { // Mix::sample :194-197, outer then inner
        size_t comps = lights.empty() ? 1 : 2;
        int distNum = S.u01(S.rng) * comps;
        if (distNum == 0) return cosine_sample(S.cosine_n01, S.rng, n);
        int li = S.u01(S.rng) * lights.size();
        return light_sample(S, li, x);
    }
    float mix_pdf(V3 x, V3 n, V3 d) const { // Mix::pdf :199-205
        float ans = 0;
        ans += cosine_pdf(n, d);
        if (lights.empty()) return ans / (size_t)1;
        float inner = 0;
        for (int idx : lights) inner += light_pdf(figs[idx], x, d);
        ans += inner / lights.size();
        return ans / (size_t)2;
    }

    // ---- scene.cpp:51-112 --------------------------------------------------------------------------------------
    V3 get_color(Sampler &S, V3 ro, V3 rd, int recLimit) const {
        if (recLimit == 0) return V3{0., 0., 0.};
        Hit h; int pos;
        if (!intersect(ro, rd, h, pos)) return bg;
        const Prim &f = figs[pos];
        float t = h.t; V3 norma = h.norma;
        V3 x = ro + t * rd;
        if (f.kind == RT_MAT_DIFFUSE) {
            V3 d = mix_sample(S, x + (float)0.0001 * norma, norma);
            if (dot(d, norma) < 0) return f.emission;
            float pdf = mix_pdf(x + (float)0.0001 * norma, norma, d);
            V3 inner = get_color(S, x + (float)0.0001 * d, d, recLimit - 1);
            return f.emission + (float)(1. / (double)(PI * pdf) * (double)dot(d, norma)) * f.color * inner;
        }
        return specular_tail(t, norma, h.inside, ro, rd, f.color, f.emission, f.kind, f.ior, (float)0.0001, [&] { return S.u01(S.rng); },
                             [&](V3 o, V3 d) { return get_color(S, o, d, recLimit - 1); });
    }
    void camera_ray(const Frame &fr, float x, float y, V3 &o, V3 &d) const { // scene.cpp:124-132: all float, no half-pixel offset
        float tanFovX = std::tan((double)(fovX / 2));
        float tanFovY = tanFovX * fr.height / fr.width;
        float nx = tanFovX * (2 * x / fr.width - 1);
        float ny = tanFovY * (2 * y / fr.height - 1);
        o = camPos;
        d = nx * camRight - ny * camUp + camFwd;
    }
    V3 get_pixel(const Frame &fr, Sampler &S, int x, int y) const { // scene.cpp:114-122
        V3 color{0, 0, 0};
        for (int s = 0; s < fr.samples; s++) {
            float nx = x + S.u01(S.rng);
            float ny = y + S.u01(S.rng);
            V3 o, d;
            camera_ray(fr, nx, ny, o, d);
            color = color + get_color(S, o, d, fr.ray_depth);
        }
        return (float)(1.0 / fr.samples) * color;
    }
};
} // namespace rto4

using namespace rto4;
extern "C" {
void *rto_hw4_create(const rt_scene_desc *d) {
    Scene4 *s = new Scene4();
    for (uint32_t i = 0; i < d->n_primitives; i++) {
        s->figs.push_back(prim_from_abi(d->primitives[i]));
        const Prim &f = s->figs.back();
        if ((f.emission.x > 0 || f.emission.y > 0 || f.emission.z > 0) && (f.type == RT_PRIM_BOX || f.type == RT_PRIM_ELLIPSOID)) s->lights.push_back((int)i);
    }
    s->camPos = v3(d->camera.position); s->camRight = v3(d->camera.right); s->camUp = v3(d->camera.up); s->camFwd = v3(d->camera.forward);
    s->fovX = d->camera.fov_x; s->bg = v3(d->bg_color);
    return s;
}
void rto_hw4_destroy(void *p) { delete (Scene4 *)p; }
int rto_hw4_num_lights(void *p) { return (int)((Scene4 *)p)->lights.size(); }

// Function-level entry points (rows and answers as oracle_txt_prims.h describes them; tests/analytic_cases.py).
void rto_hw4_fig(const float *rows, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        Hit h;
        put_hit(prim_ray3(prim_of_row(r), v3(r + R_O), v3(r + R_D), h, true), h, out + 5 * i);
    }
}
// FigureLight::pdf of the row's figure as a light, x = o.  out: 1 word
void rto_hw4_lpdf(const float *rows, size_t n, uint32_t *out) {
    Scene4 s;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        out[i] = word(s.light_pdf(prim_of_row(r), v3(r + R_O), v3(r + R_D)));
    }
}
// pdfOne(x, d, y, yn) of the row's figure as a light on a y and yn of the row's own (30 floats: the figure row, y 3, yn 3).  out: 1 word
void rto_hw4_pdf_one(const float *rows30, size_t n, uint32_t *out) {
    Scene4 s;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows30 + 30 * i;
        out[i] = word(s.pdf_one(prim_of_row(r), v3(r + R_O), v3(r + R_D), v3(r + 24), v3(r + 27)));
    }
}
// One round's point of BoxLight::sample (box_emitter_point, the same lines in hw4 and hw5) for half-sizes s3 and an engine seeded seeds[i].
// out: 4 words (the point in the box's frame, engine state after)
void rto_box_face_point(const float *s3, const uint32_t *seeds, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        rng_t rng(seeds[i]);
        U01 u01(0.0, 1.0);
        const V3 p = box_emitter_point(v3(s3 + 3 * i), u01, rng);
        out[4 * i] = word(p.x); out[4 * i + 1] = word(p.y); out[4 * i + 2] = word(p.z); out[4 * i + 3] = state_of(rng);
    }
}
// The light's sample(x), engine seeded aux[0], the light's own normal_distribution primed by aux[1].  out: 8 words (put_sample).  A row
// that asks the figure more than max_attempts times gets zeros; returns the number of such rows.  attempts (may be null): the figure tests per row.
int rto_hw4_lsample(const float *rows, const uint32_t *aux, size_t n, uint32_t max_attempts, uint32_t *out, uint32_t *attempts) {
    int over = 0;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        Scene4 s;
        s.figs.push_back(prim_of_row(r));
        s.lights.push_back(0);
        Sampler S;
        S.rng.seed(aux[2 * i]);
        const N01 before = primed(aux[2 * i + 1]);
        S.light_n01.assign(1, before);
        CountedRay<Scene4::Ray> ray{Scene4::Ray(), max_attempts};
        try {
            const V3 d = s.light_sample(S, 0, v3(r + R_O), ray);
            put_sample(d, S.rng, S.light_n01[0], before, out + 8 * i);
        } catch (const TooManyAttempts &) { memset(out + 8 * i, 0, 32); over++; }
        if (attempts) attempts[i] = max_attempts - ray.left;
    }
    return over;
}
// Cosine::sample(n), engine seeded aux[0], the Cosine object's normal_distribution primed by aux[1].  out: 8 words (put_sample)
void rto_hw4_cosine(const float *normals, const uint32_t *aux, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        rng_t rng(aux[2 * i]);
        const N01 before = primed(aux[2 * i + 1]);
        N01 n01 = before;
        const V3 d = cosine_sample(n01, rng, v3(normals + 3 * i));
        put_sample(d, rng, n01, before, out + 8 * i);
    }
}

// seed_mode 0: one engine + one set of distribution objects for the whole call, pixels in row-major order (the reference);
// seed_mode 1: fresh engine(y*W+x) and fresh distribution objects per pixel (parallel).
int rto_hw4_render(void *p, int width, int height, int samples, int ray_depth, int seed_mode, int x0, int y0, int w, int h,
                   float *out_rgb, uint8_t *out8, int nthreads) {
    const Scene4 *s = (const Scene4 *)p;
    const Frame fr{width, height, samples, ray_depth};
    auto pixel = [&](Sampler &S, int x, int y) { return s->get_pixel(fr, S, x, y); };
    auto fresh = [&](int seed) { Sampler S; S.rng.seed(seed); S.light_n01.assign(s->lights.size(), N01(0.f, 1.f)); return S; };
    Sampler whole = fresh(rng_t::default_seed);             // scene.cpp:5: a default-constructed engine
    if (seed_mode == 0) render_rect(true, 1, x0, y0, w, h, out_rgb, out8, [&](int, int) -> Sampler & { return whole; }, pixel);
    else render_rect(false, nthreads, x0, y0, w, h, out_rgb, out8, [&](int x, int y) { return fresh(y * width + x); }, pixel);
    return 0;
}
}

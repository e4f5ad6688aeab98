// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the two .txt-scene snapshots named by BASELINE.json:
//   hw1  ray caster            (hw1/src/scene.cpp:7-30, hw1/src/primitives.cpp:24-91)          — configs[0]
//   hw3  first path tracer     (hw3/src/scene.cpp:11-107, hw3/src/primitives.cpp:8-123)        — configs[1]
// hw3 draws every random number of the whole frame from ONE file-static minstd_rand in pixel order
// (hw3/src/scene.cpp:5-7), so the reference image can only be replayed sequentially; `seed_mode` 0 does
// exactly that (pinned byte-for-byte against the compiled hw3 program), `seed_mode` 1 seeds one engine per
// pixel with y*W+x like hw5+ do — the only form a parallel machine can run, used to check the GPU.
#include "oracle_txt_prims.h"

namespace rtot {

struct Scene3 {
    std::vector<Prim> figs;
    V3 camPos, camRight, camUp, camFwd, bg;
    float fovX = 0;

    // hw3/src/scene.cpp:11-29 (tmax = +inf)
    bool intersect(V3 o, V3 d, Hit &best, int &pos) const {
        pos = -1;
        for (int i = 0; i < (int)figs.size(); i++) {
            Hit h;
            if (prim_ray3(figs[i], o, d, h) && h.t <= INFINITY && (pos == -1 || h.t < best.t)) { best = h; pos = i; }
        }
        return pos != -1;
    }
    // hw3/src/scene.cpp:31-87
    V3 get_color(rng_t &rnd, U01 &u01, N01 &n01, V3 ro, V3 rd, int recLimit) const {
        if (recLimit == 0) return V3{0., 0., 0.};
        Hit h; int pos;
        if (!intersect(ro, rd, h, pos)) return bg;
        const Prim &f = figs[pos];
        float t = h.t; V3 norma = h.norma;
        if (f.kind == RT_MAT_DIFFUSE) {
            float a = n01(rnd), b = n01(rnd), c = n01(rnd);
            V3 w = normalize(V3{a, b, c});
            if (dot(w, norma) < 0) w = neg1(w);
            V3 o = ro + t * rd + (float)0.0001 * w;
            return f.emission + (2 * dot(w, norma)) * f.color * get_color(rnd, u01, n01, o, w, recLimit - 1);
        }
        return specular_tail(t, norma, h.inside, ro, rd, f.color, f.emission, f.kind, f.ior, (float)0.0001, [&] { return u01(rnd); },
                             [&](V3 o, V3 d) { return get_color(rnd, u01, n01, o, d, recLimit - 1); });
    }
    // hw3/src/scene.cpp:99-107
    void camera_ray(const Frame &fr, float x, float y, V3 &o, V3 &d, bool float_tan = false) const {
        float tanFovX = float_tan ? tanf(fovX / 2) : (float)std::tan((double)(fovX / 2)); // hw1: <math.h> => tanf
        float tanFovY = tanFovX * fr.height / fr.width;
        float nx = tanFovX * (2 * (x + 0.5) / fr.width - 1);
        float ny = tanFovY * (2 * (y + 0.5) / fr.height - 1);
        o = camPos;
        d = nx * camRight - ny * camUp + camFwd;
    }
    // hw3/src/scene.cpp:89-97
    V3 get_pixel(const Frame &fr, rng_t &rnd, U01 &u01, N01 &n01, int x, int y) const {
        V3 color{0, 0, 0};
        for (int s = 0; s < fr.samples; s++) {
            float nx = x + u01(rnd);
            float ny = y + u01(rnd);
            V3 o, d;
            camera_ray(fr, nx, ny, o, d);
            color = color + get_color(rnd, u01, n01, o, d, fr.ray_depth);
        }
        return (float)(1.0 / fr.samples) * color;
    }
};

// ---- hw1 -------------------------------------------------------------------------------------------------
// hw1/src/primitives.cpp:24-91: nearest primitive, flat colour, no normals.
static bool prim_ray1(const Prim &f, V3 o, V3 d, float &t) {
    V3 to = qtransform(f.rotation, o - f.position), td = qtransform(f.rotation, d);
    if (f.type == RT_PRIM_ELLIPSOID) {                                     // :54-59: b = (2*(o/r)) . (d/r)
        V3 r = f.data;
        float c = len2(to / r) - 1;
        float b = dot(2 * (to / r), td / r);
        float a = len2(td / r);
        float dd = b * b - 4 * a * c;
        if (dd <= 0) return false;
        float x1 = (-b - sqrtf(dd)) / (2 * a);   // hw1 includes <math.h>: sqrt(float) is the float overload (see oracle_hw2.cpp)
        float x2 = (-b + sqrtf(dd)) / (2 * a);
        if (x1 > x2) std::swap(x1, x2);
        if (x2 < 0) return false;
        t = x1 < 0 ? x2 : x1;
        return true;
    }
    if (f.type == RT_PRIM_PLANE) {                                          // :64-70
        t = -dot(to, f.data) / dot(td, f.data);
        return t > 0;
    }
    V3 s = f.data;                                                          // :76-91
    V3 ts1 = (neg1(s) - to) / td, ts2 = (s - to) / td;
    float t1x = smin(ts1.x, ts2.x), t2x = smax(ts1.x, ts2.x);
    float t1y = smin(ts1.y, ts2.y), t2y = smax(ts1.y, ts2.y);
    float t1z = smin(ts1.z, ts2.z), t2z = smax(ts1.z, ts2.z);
    float t1 = smax(smax(t1x, t1y), t1z), t2 = smin(smin(t2x, t2y), t2z);
    if (t1 > t2 || t2 < 0) return false;
    t = t1 < 0 ? t2 : t1;
    return true;
}

static Scene3 *make_scene(const rt_scene_desc *d) {
    Scene3 *s = new Scene3();
    for (uint32_t i = 0; i < d->n_primitives; i++) {
        s->figs.push_back(prim_from_abi(d->primitives[i]));
    }
    s->camPos = v3(d->camera.position); s->camRight = v3(d->camera.right); s->camUp = v3(d->camera.up); s->camFwd = v3(d->camera.forward);
    s->fovX = d->camera.fov_x; s->bg = v3(d->bg_color);
    return s;
}
} // namespace rtot

using namespace rtot;
extern "C" {
void *rto_txt_create(const rt_scene_desc *d) { return make_scene(d); }
void rto_txt_destroy(void *p) { delete (Scene3 *)p; }

// hw1: out8 = round(255*colour) bytes (hw1/src/color.cpp:13-19), out_rgb = the colour itself.
int rto_hw1_render(void *p, int width, int height, float *out_rgb, uint8_t *out8) {
    const Scene3 *s = (const Scene3 *)p;
    const Frame fr{width, height, 1, 1};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            V3 o, d;
            s->camera_ray(fr, (float)x, (float)y, o, d, true); // hw1/src/scene.cpp:22-30 takes ints; (x + 0.5) is the same double either way
            V3 ans = s->bg;
            float best = -1;
            for (const Prim &f : s->figs) {
                float t;
                if (prim_ray1(f, o, d, t) && (best == -1 || t < best)) { best = t; ans = f.color; }
            }
            size_t j = (size_t)y * width + x;
            if (out_rgb) { out_rgb[3 * j] = ans.x; out_rgb[3 * j + 1] = ans.y; out_rgb[3 * j + 2] = ans.z; }
            if (out8) { out8[3 * j] = (uint8_t)std::round((double)(255 * ans.x)); out8[3 * j + 1] = (uint8_t)std::round((double)(255 * ans.y)); out8[3 * j + 2] = (uint8_t)std::round((double)(255 * ans.z)); }
        }
    return 0;
}

// Function-level entry points (rows and answers as oracle_txt_prims.h describes them; tests/analytic_cases.py).
void rto_hw1_fig(const float *rows, size_t n, uint32_t *out) { // hw1 has no side and no normal: flags 1, t, zeros
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        float t = 0;
        Hit h{0, V3{0, 0, 0}, false};
        const bool ok = prim_ray1(prim_of_row(r), v3(r + R_O), v3(r + R_D), t);
        h.t = t;
        put_hit(ok, h, out + 5 * i);
    }
}
void rto_hw3_quad(const float *abc, size_t n, uint32_t *out) { quad_rows(abc, n, out, smallest_root); }
void rto_hw3_slabs(const float *rows9, size_t n, uint32_t *out) { // box_local's slab test: s, o, d -> flags, t
    for (size_t i = 0; i < n; i++) {
        const float *p = rows9 + 9 * i;
        Hit h;
        const bool ok = box_local(v3(p), v3(p + 3), v3(p + 6), h);
        out[2 * i] = ok ? (1u | (h.inside ? 2u : 0u)) : 0u; out[2 * i + 1] = ok ? word(h.t) : 0u;
    }
}
void rto_hw3_fig(const float *rows, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        const float *r = rows + ROW * i;
        Hit h;
        put_hit(prim_ray3(prim_of_row(r), v3(r + R_O), v3(r + R_D), h), h, out + 5 * i);
    }
}

// hw3.  seed_mode 0: one engine for the whole frame, pixels in row-major order (the reference, single thread);
//       seed_mode 1: engine(y*W+x) per pixel (parallel).
struct Stream3 { rng_t rnd; U01 u01{0.0, 1.0}; N01 n01{0.0, 1.0}; }; // hw3/src/scene.cpp:5-7: default-seeded, shared by everything
int rto_hw3_render(void *p, int width, int height, int samples, int ray_depth, int seed_mode, int x0, int y0, int w, int h,
                   float *out_rgb, uint8_t *out8, int nthreads) {
    const Scene3 *s = (const Scene3 *)p;
    const Frame fr{width, height, samples, ray_depth};
    auto pixel = [&](Stream3 &S, int x, int y) { return s->get_pixel(fr, S.rnd, S.u01, S.n01, x, y); };
    Stream3 whole;
    if (seed_mode == 0) render_rect(true, 1, x0, y0, w, h, out_rgb, out8, [&](int, int) -> Stream3 & { return whole; }, pixel);
    else render_rect(false, nthreads, x0, y0, w, h, out_rgb, out8, [&](int x, int y) { Stream3 S; S.rnd.seed(y * width + x); return S; }, pixel);
    return 0;
}
}

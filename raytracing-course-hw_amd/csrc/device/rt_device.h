// Device-side building blocks of the replay path tracer (gfx950).
//
// Arithmetic contract: this translation unit is compiled with -ffp-contract=off and IEEE
// division/sqrt (hipcc default), so every float/double expression below rounds exactly like the
// reference's x86-64 -O3 build (no FMA, no fast-math).  Where the reference
// promotes to double across SEVERAL operations the doubles are kept; where it promotes around a
// single +,-,*,/ or sqrt the float operation is used (double rounding is innocuous there:
// 53 >= 2*24+2).  FMA is used only where it is spelled fmaf()/fma(): in my own BVH slab test
// (conservative by construction) and in rt_logf, which replays glibc 2.35's FMA build of logf.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_types.h"

#define RT_DEV __device__ __forceinline__

namespace rtamd {
namespace dev {

struct F3 { float x, y, z; };
RT_DEV F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
RT_DEV F3 f3(const float *p) { return f3(p[0], p[1], p[2]); }
RT_DEV F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
RT_DEV F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
RT_DEV F3 operator*(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
RT_DEV F3 operator*(float k, F3 p) { return f3(k * p.x, k * p.y, k * p.z); }
RT_DEV F3 neg(F3 a) { return f3(-a.x, -a.y, -a.z); }                       // "-1. * v"
RT_DEV float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; } // vec3.h:53-55
// vec3.h:57-59: the reference's cross() is the NEGATED conventional cross product.
RT_DEV F3 crossr(F3 a, F3 o) { return f3(a.z * o.y - a.y * o.z, a.x * o.z - a.z * o.x, a.y * o.x - a.x * o.y); }
RT_DEV float len2(F3 a) { return dot(a, a); }
RT_DEV float len(F3 a) { return sqrtf(len2(a)); }                          // vec3.h:65-67
RT_DEV F3 normalize(F3 a) { return (1.0f / len(a)) * a; }                  // vec3.h:78-80
RT_DEV float smin(float a, float b) { return (b < a) ? b : a; }            // std::min
RT_DEV float smax(float a, float b) { return (a < b) ? b : a; }            // std::max

// ---- RNG: std::minstd_rand + libstdc++ distributions -------------------------
struct Rng {
    uint32_t x;      // engine state
    float saved;     // normal_distribution::_M_saved
    bool has_saved;  // _M_saved_available
};
RT_DEV void rng_seed(Rng &r, uint32_t s) { // linear_congruential_engine::seed: s mod m, 0 -> 1
    uint32_t v = s % 2147483647u;
    r.x = v == 0 ? 1u : v;
    r.saved = 0.f;
    r.has_saved = false;
}
RT_DEV uint32_t rng_next(Rng &r) { // x <- 48271 x mod (2^31 - 1), via 2^31 == 1 (mod m)
    uint64_t p = (uint64_t)r.x * 48271ull;
    uint32_t s = (uint32_t)(p & 0x7fffffffu) + (uint32_t)(p >> 31);
    if (s >= 2147483647u) s -= 2147483647u;
    r.x = s;
    return s;
}
// uniform_real_distribution<float>(0,1): generate_canonical<float,24> with one engine call
// (bits/random.tcc:3348-3385): float(x - min) / 2147483648.0f, clamped below 1.
RT_DEV float rng_u01(Rng &r) {
    float s = __uint2float_rn(rng_next(r) - 1u);
    float v = s * 4.656612873077392578125e-10f; // exact: division by 2^31
    return v >= 1.0f ? 0.99999994f : v;
}

// glibc 2.35 logf, FMA build (sysdeps/ieee754/flt-32/e_logf.c selected by the x86_64 multiarch
// ifunc on CPUs with FMA+AVX2): table + degree-3 polynomial in double, contracted exactly as
// in that build.  Bit-identical to the host logf for every positive normal float
// (tests/test_device_math.py checks it exhaustively against libm on the CPU).
struct LogfTab { double invc, logc; };
__device__ const LogfTab rt_logf_tab[16] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
RT_DEV float rt_logf(float x) {
    uint32_t ix = __float_as_uint(x);
    if (ix == 0x3f800000u) return 0.f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2 == 0) return -__builtin_inff();
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return __builtin_nanf("");
        ix = __float_as_uint(x * 0x1p23f);
        ix -= 23u << 23;
    }
    uint32_t tmp = ix - 0x3f330000u;
    uint32_t i = (tmp >> 19) & 15u;
    int k = (int)tmp >> 23;
    uint32_t iz = ix - (tmp & 0xff800000u);
    double invc = rt_logf_tab[i].invc, logc = rt_logf_tab[i].logc;
    double z = (double)__uint_as_float(iz);
    double r = fma(z, invc, -1.0);
    double y0 = fma((double)k, 0x1.62e42fefa39efp-1, logc);
    double r2 = r * r;
    double y = fma(0x1.5575b0be00b6ap-2, r, -0x1.ffffef20a4123p-2);
    y = fma(-0x1.00ea348b88334p-2, r2, y);
    y = fma(y, r2, y0 + r);
    return (float)y;
}

// glibc 2.35 atanf, atan2f and asinf (sysdeps/ieee754/flt-32/s_atanf.c, e_atan2f.c, e_asinf.c): the float overloads
// that std::atan2(float, float) and std::asin(float) select in the reference's environment-map lookup (scene.cpp:94-95).
// fdlibm's float algorithms, restated in float arithmetic only: no FMA (x86-64 glibc builds these without the multiarch
// ifunc that logf has, so the host CPU does not matter), correctly rounded division and sqrtf, atanf's atanhi / atanlo
// picked by selects instead of a runtime-indexed table.  Bit-identical to the host libm of an x86-64 glibc 2.35 host: asinf on
// every float in [-1, 1], atanf on every float, atan2f on 6e7 pairs and the special values; tests/test_gpu_device_math.py
// checks the device against the host libm.
RT_DEV float rt_atanf(float x) {
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    if (ix >= 0x4c000000u) {                                   // |x| >= 2^25 (or NaN)
        if (ix > 0x7f800000u) return x + x;
        const float r = 1.5707962513e+00f + 7.5497894159e-08f; // atanhi[3] + atanlo[3]
        return (hx >> 31) ? -r : r;
    }
    int id = -1;
    if (ix < 0x3ee00000u) {                                    // |x| < 7/16
        if (ix < 0x31000000u) return x;                        // |x| < 2^-29
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000u) {                                // |x| < 19/16
            if (ix < 0x3f300000u) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }   // 7/16 <= |x| < 11/16
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }                        // 11/16 <= |x| < 19/16
        } else {
            if (ix < 0x401c0000u) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); } // 19/16 <= |x| < 39/16
            else { id = 3; x = -1.0f / x; }                                        // 39/16 <= |x| < 2^26
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (3.3333334327e-01f + w * (1.4285714924e-01f + w * (9.0908870101e-02f + w * (6.6610731184e-02f + w * (4.9768779427e-02f + w * 1.6285819933e-02f)))));
    const float s2 = w * (-2.0000000298e-01f + w * (-1.1111110449e-01f + w * (-7.6918758452e-02f + w * (-5.8335702866e-02f + w * -3.6531571299e-02f))));
    if (id < 0) return x - x * (s1 + s2);
    // atanhi[id], atanlo[id] by selects: a table indexed by a runtime id would live in scratch
    const float hi = id == 0 ? 4.6364760399e-01f : id == 1 ? 7.8539812565e-01f : id == 2 ? 9.8279368877e-01f : 1.5707962513e+00f;
    const float lo = id == 0 ? 5.0121582440e-09f : id == 1 ? 3.7748947079e-08f : id == 2 ? 3.4473217170e-08f : 7.5497894159e-08f;
    const float r = hi - ((x * (s1 + s2) - lo) - x);
    return (hx >> 31) ? -r : r;
}

RT_DEV float rt_atan2f(float y, float x) {
    const float pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const uint32_t hx = __float_as_uint(x), hy = __float_as_uint(y);
    const uint32_t ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix > 0x7f800000u || iy > 0x7f800000u) return x + y;   // NaN
    if (hx == 0x3f800000u) return rt_atanf(y);                 // x = 1
    const uint32_t m = ((hy >> 31) & 1u) | ((hx >> 30) & 2u);  // 2 sign(x) + sign(y)
    if (iy == 0) return m < 2 ? y : m == 2 ? pi : -pi;        // atan(+-0, +x) = +-0, atan(+-0, -x) = +-pi
    if (ix == 0) return (hy >> 31) ? -pi_o_2 : pi_o_2;
    if (ix == 0x7f800000u) {
        if (iy == 0x7f800000u) return m == 0 ? pi_o_4 : m == 1 ? -pi_o_4 : m == 2 ? 3.0f * pi_o_4 : -3.0f * pi_o_4;
        return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? pi : -pi;
    }
    if (iy == 0x7f800000u) return (hy >> 31) ? -pi_o_2 : pi_o_2;
    const int k = ((int)iy - (int)ix) >> 23;
    float z;
    if (k > 26) z = pi_o_2 + 0.5f * pi_lo;                     // |y/x| > 2^26
    else if ((hx >> 31) && k < -26) z = 0.0f;                  // |y|/x < -2^26
    else z = rt_atanf(fabsf(y / x));
    switch (m) {
    case 0: return z;
    case 1: return -z;
    case 2: return pi - (z - pi_lo);
    default: return (z - pi_lo) - pi;
    }
}

RT_DEV float rt_asinf(float x) {
    const float pio2_hi = 1.57079637050628662109375f, pio2_lo = -4.37113900018624283e-8f, pio4_hi = 0.785398185253143310546875f;
    const float p0 = 1.666675248e-1f, p1 = 7.495297643e-2f, p2 = 4.547037598e-2f, p3 = 2.417951451e-2f, p4 = 4.216630880e-2f;
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    if (ix == 0x3f800000u) return x * pio2_hi + x * pio2_lo;  // asin(+-1) = +-pi/2
    if (ix > 0x3f800000u) return (x - x) / (x - x);            // |x| > 1 (and NaN): NaN
    if (ix < 0x3f000000u) {                                    // |x| < 0.5
        if (ix < 0x32000000u) return x;                        // |x| < 2^-27
        const float t = x * x;
        const float w = t * (p0 + t * (p1 + t * (p2 + t * (p3 + t * p4))));
        return x + x * w;
    }
    const float w = 1.0f - fabsf(x);                           // 0.5 <= |x| < 1
    float t = w * 0.5f;
    float p = t * (p0 + t * (p1 + t * (p2 + t * (p3 + t * p4))));
    const float s = sqrtf(t);
    if (ix >= 0x3f79999au) {                                   // |x| > 0.975
        t = pio2_hi - (2.0f * (s + s * p) - pio2_lo);
    } else {
        const float wh = __uint_as_float(__float_as_uint(s) & 0xfffff000u);
        const float c = (t - wh * wh) / (s + wh);
        const float r = p;
        p = 2.0f * s * r - (pio2_lo - 2.0f * c);
        const float q = pio4_hi - 2.0f * wh;
        t = pio4_hi - (p - q);
    }
    return (hx >> 31) ? -t : t;
}

// normal_distribution<float>(0,1): Marsaglia polar with the saved second value
// (bits/random.tcc:1802-1838).
RT_DEV float rng_n01(Rng &r) {
    if (r.has_saved) {
        r.has_saved = false;
        return r.saved;
    }
    float x, y, r2;
    do {
        x = 2.0f * rng_u01(r) - 1.0f;
        y = 2.0f * rng_u01(r) - 1.0f;
        r2 = x * x + y * y;
    } while (r2 > 1.0f || r2 == 0.0f);
    float mult = sqrtf(-2 * rt_logf(r2) / r2);
    r.saved = x * mult;
    r.has_saved = true;
    return y * mult;
}
// One polar round of rng_n01: the value it returns (y * mult) and the one it saves (x * mult).
RT_DEV void rng_polar(Rng &r, float &ret, float &keep) {
    float x, y, r2;
    do {
        x = 2.0f * rng_u01(r) - 1.0f;
        y = 2.0f * rng_u01(r) - 1.0f;
        r2 = x * x + y * y;
    } while (r2 > 1.0f || r2 == 0.0f);
    float mult = sqrtf(-2 * rt_logf(r2) / r2);
    keep = x * mult;
    ret = y * mult;
}
// a = rng_n01(r), b = rng_n01(r), c = rng_n01(r): the same engine calls, values and state afterwards.  A lane that enters with a saved value
// needs one polar round (saved, ret, keep), one without needs two (ret, keep, ret2; keep2 saved).  Three inlined rng_n01 make a wave that
// holds both kinds run three rejection loops with the logarithm, root and division after each; here it runs one round for every lane and
// a second for the lanes that entered without a saved value.
RT_DEV void rng_n01x3(Rng &r, float &a, float &b, float &c) {
    float p, q;
    rng_polar(r, p, q);
    if (r.has_saved) { a = r.saved; b = p; c = q; r.saved = q; r.has_saved = false; }
    else { a = p; b = q; rng_polar(r, c, r.saved); r.has_saved = true; }
}

// ---- quaternion (quaternion.h:36-46) ------------------------------------------------------------
struct Quat { F3 v; float w; };
RT_DEV Quat qmul(Quat a, Quat b) {
    Quat r;
    r.v = a.w * b.v + b.w * a.v + crossr(a.v, b.v);
    r.w = a.w * b.w - dot(a.v, b.v);
    return r;
}
RT_DEV Quat qconj(Quat q) { Quat r; r.v = neg(q.v); r.w = q.w; return r; }
RT_DEV F3 qtransform(Quat q, F3 p) {
    Quat pq; pq.v = p; pq.w = 0.f;
    return qmul(qmul(q, pq), qconj(q)).v;
}

// ---- ray / triangle (primitives.cpp:18-27,76-125) -----------------------------------------------
#define RT_T_MAX 1e4f
#define RT_MAGIC1_0 0.239f
#define RT_MAGIC1_1 0.419f
#define RT_MAGIC1_2 0.533f
#define RT_MAGIC2_0 0.35743f
#define RT_MAGIC2_1 0.66682f
#define RT_MAGIC2_2 0.69695f

// Bit-exact Figure::intersectAsTriangle up to the barycentric rejection; attribute interpolation
// is deferred to the hit that survives (shade_fetch).
RT_DEV bool tri_test(const TriIsect &T, F3 o, F3 d, float &t, float &u, float &v, bool &inside) {
    F3 a = f3(T.ax, T.ay, T.az), n = f3(T.nx, T.ny, T.nz);
    F3 ro = o - a;
    float dn = dot(d, n);
    t = -dot(ro, n) / dn;
    if (!(t > 0 && t < RT_T_MAX)) return false;
    inside = dn > 0;
    F3 p = ro + t * d;
    float c1 = RT_MAGIC1_0 * p.x + RT_MAGIC1_1 * p.y + RT_MAGIC1_2 * p.z;
    float c2 = RT_MAGIC2_0 * p.x + RT_MAGIC2_1 * p.y + RT_MAGIC2_2 * p.z;
    float yy = (c1 * T.a2 - c2 * T.a1) / T.den;
    float xx = T.a2 == 0 ? (c1 - T.b1 * yy) / T.a1 : (c2 - T.b2 * yy) / T.a2;
    u = xx; v = yy;
    if (u < 0 || v < 0 || u + v > 1) return false;
    return true;
}

// tri_test for a closest-hit walk that already holds a hit: a triangle whose plane lies beyond keep_t (the best t plus the walkers'
// look-behind, rt_exact.h) can neither become the closest hit nor matter as its runner-up whatever its barycentrics are, so their
// two divisions are skipped.  Exactly the same accept / reject decisions as tri_test for every triangle that could still matter.
RT_DEV bool tri_test_closer(const TriIsect &T, F3 o, F3 d, float keep_t, float &t, float &u, float &v, bool &inside) {
    F3 a = f3(T.ax, T.ay, T.az), n = f3(T.nx, T.ny, T.nz);
    F3 ro = o - a;
    float dn = dot(d, n);
    t = -dot(ro, n) / dn;
    if (!(t > 0 && t < RT_T_MAX)) return false;
    if (t > keep_t) return false;
    inside = dn > 0;
    F3 p = ro + t * d;
    float c1 = RT_MAGIC1_0 * p.x + RT_MAGIC1_1 * p.y + RT_MAGIC1_2 * p.z;
    float c2 = RT_MAGIC2_0 * p.x + RT_MAGIC2_1 * p.y + RT_MAGIC2_2 * p.z;
    float yy = (c1 * T.a2 - c2 * T.a1) / T.den;
    float xx = T.a2 == 0 ? (c1 - T.b1 * yy) / T.a1 : (c2 - T.b2 * yy) / T.a2;
    u = xx; v = yy;
    if (u < 0 || v < 0 || u + v > 1) return false;
    return true;
}

RT_DEV TriIsect isect_of(float4 a, float4 b, float4 c) { // a record from its three 16-byte words
    TriIsect T;
    T.ax = a.x; T.ay = a.y; T.az = a.z; T.nx = a.w;
    T.ny = b.x; T.nz = b.y; T.a1 = b.z; T.b1 = b.w;
    T.a2 = c.x; T.b2 = c.y; T.den = c.z; T.pad = __float_as_uint(c.w);
    return T;
}
RT_DEV TriIsect load_isect(const TriIsect *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    return isect_of(a, b, c);
}

// A wave-uniform array that a walker reads in its innermost loops, as the loads want it: the base in a scalar register pair of its own, known to
// the compiler to point into global memory, and every record at a 32-bit byte offset from it.  That is the `global_load v, v_off, s[base]` form:
// no 64-bit address arithmetic per fetch, and no flat access, which would count on the LDS counter as well and make a fetch wait for the lane's
// stack traffic.  The arrays read this way hold at most RT_WALK_MAX_RECORDS records and stay below 4 GiB (rt_types.h; checked at scene creation).
// Why a pair of its own: taken straight from the kernel arguments the pointer sits in a group of four registers that the allocator keeps or spills
// as a whole.  Without the copy (profiles/r09_scheduler_refactor.txt) the hw8 node loops reload the pointer with 4 v_readlane per step and the light
// leaf loop reloads 30 SGPRs per iteration instead of 15.
#define RT_GLOBAL __attribute__((address_space(1)))
struct GlobalBytes {
    const RT_GLOBAL char *base;
    // A plain vector: HIP's uint4 is a class, which no address space but the generic one can copy.  Loaded this way a record's three words come as
    // three 16-byte loads ahead of the test; through a uint4 pointer the compiler cut them up and sank 20 bytes of a triangle behind its plane test,
    // a second round trip for every lane that passed it (profiles/r32_walker_loads.txt).
    typedef uint32_t Word4 __attribute__((ext_vector_type(4)));
    // 16-byte word k of the record at byte `ofs`: base + ofs is the load's scalar base and 32-bit offset, 16 k its immediate
    RT_DEV uint4 u4(uint32_t ofs, uint32_t k = 0u) const { const Word4 w = reinterpret_cast<const RT_GLOBAL Word4 *>(base + ofs)[k]; return make_uint4(w.x, w.y, w.z, w.w); }
    RT_DEV float4 f4(uint32_t ofs, uint32_t k = 0u) const { const uint4 w = u4(ofs, k); return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w)); }
};
RT_DEV GlobalBytes global_bytes(const void *p) { return GlobalBytes{(const RT_GLOBAL char *)p}; }                    // the address space alone
RT_DEV GlobalBytes global_bytes_own(const void *p) { asm volatile("" : "+s"(p)); return global_bytes(p); }           // ... and the register pair
// byte offset of record i < 2^24 of `stride` bytes each: one full-rate 24-bit multiply
RT_DEV uint32_t record_ofs(uint32_t i, uint32_t stride) { return __umul24(i, stride); }
// the TriIsect at the head of the record at byte `ofs`
RT_DEV TriIsect load_isect(const GlobalBytes &g, uint32_t ofs) {
    const float4 a = g.f4(ofs, 0u), b = g.f4(ofs, 1u), c = g.f4(ofs, 2u);
    return isect_of(a, b, c);
}

// ---- my BVH: conservative two-box slab test -------------------------------------------------------
struct RayInv { F3 o, inv; };
RT_DEV RayInv make_ray_inv(F3 o, F3 d) {
    RayInv r;
    r.o = o;
    // A zero (or denormal) direction component would give inf*0 = NaN in the slab products.
    float dx = fabsf(d.x) > 1e-30f ? d.x : copysignf(1e-30f, d.x);
    float dy = fabsf(d.y) > 1e-30f ? d.y : copysignf(1e-30f, d.y);
    float dz = fabsf(d.z) > 1e-30f ? d.z : copysignf(1e-30f, d.z);
    r.inv = f3(1.0f / dx, 1.0f / dy, 1.0f / dz);
    return r;
}
// Returns whether [tmin,tmax] (widened by 4 ulp-ish) overlaps [0, tbest]; boxes are host-padded.
RT_DEV bool slab_test(float4 lo, float4 hi, const RayInv &r, float tbest, float &tnear) {
    float t0x = (lo.x - r.o.x) * r.inv.x, t1x = (hi.x - r.o.x) * r.inv.x;
    float t0y = (lo.y - r.o.y) * r.inv.y, t1y = (hi.y - r.o.y) * r.inv.y;
    float t0z = (lo.z - r.o.z) * r.inv.z, t1z = (hi.z - r.o.z) * r.inv.z;
    float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    tmin = fmaf(-fabsf(tmin), 4.8e-7f, tmin);
    tmax = fmaf(fabsf(tmax), 4.8e-7f, tmax);
    tnear = tmin;
    return (tmin <= tmax) & (tmax >= 0.f) & (tmin <= tbest);
}

typedef float rt_f2 __attribute__((ext_vector_type(2)));
// The walk nodes on the 16-bit grid (rt_types.h GpuNode4Q).  The ray moves into grid coordinates once per walk,
//     o' = (o - grid.lo) / step,   1/d' = step / d      (t keeps its meaning: x = o + t d  <=>  x' = o' + t d'),
// and a child's slabs are t = cell * (1/d') + c with c = -o' * (1/d') formed once per walk: one FMA per slab.  Cells are small integers,
// exact in a float.  The error budget, as a displacement of a slab along its axis, in cells (an error dt of t is dt / |1/d'| cells):
//   o'    three roundings (the difference, grid.lo itself, the product with 1/step), each 2^-24 of a coordinate of at most 65,536 cells
//         for an origin inside the grid (the grid covers the scene's boxes and the camera, so every ray origin):  3 * 2^-8  = 0.012
//   1/d'  a 1-ulp reciprocal and a rounded product, 2.5 * 2^-24 relative; c is formed from the same rounded 1/d', so what is left is a
//         scaling of the axis' t about the origin, of a distance |cell - o'| <= 65,536 cells:                    2.5 * 2^-8 = 0.010
//   c     one rounding, 2^-24 |c| = 2^-24 |o'| |1/d'|:                                                             2^-8  = 0.004
//   t     the FMA's single rounding, 2^-24 |t| = 2^-24 |cell - o'| |1/d'|:                                          2^-8  = 0.004
// together 0.03 cells, whatever the direction: every term is relative to a product with 1/d', so a component clamped to 1e-30 scales the
// error and the cell alike.  (On float boxes the same form was dropped: there |o / d| has no bound.  Here |o'| <= 65,536 by construction.)
// A point of the float box lies at least one whole cell inside the grid box on every axis (rt_node_grid.h grid_axis_word), so every t at
// which the real ray is in the float box stays inside all three computed intervals, and the interval needs no widening of its own.
// Overflow: |cell * (1/d')| and |c| stay finite while step < 2^127 / (65,536 * 1e30), a scene under 1e8 across; beyond that a NaN slab is
// ignored by v_max / v_min, which only lets more boxes in.
// cx, cy, cz: c.  sx, sy, sz: byte selectors (v_perm_b32) that put the slab the ray meets first into the low half of
// a record's axis word — lo | hi << 16 as stored for a direction component >= 0, the halves swapped for a negative one — so that the test
// needs no min / max per axis.
struct RayGrid { float cx, cy, cz, ix, iy, iz; uint32_t sx, sy, sz; };
RT_DEV RayGrid ray_grid_idle() { // what an idle lane holds (never used); field by field: an aggregate constant would be copied from memory
    RayGrid g;
    g.cx = 0.f; g.cy = 0.f; g.cz = 0.f; g.ix = 1.f; g.iy = 1.f; g.iz = 1.f; g.sx = 0x03020100u; g.sy = 0x03020100u; g.sz = 0x03020100u;
    return g;
}
#define RT_GRID_RAY_IDLE ray_grid_idle()
RT_DEV RayGrid make_ray_grid(const NodeGrid &G, F3 o, F3 d) {
    // reciprocals by v_rcp_f32 (1 ulp): part of the relative error the boxes' extra cell covers (above); a zero (or denormal) component is
    // replaced as in make_ray_inv
    const float dx = fabsf(d.x) > 1e-30f ? d.x : copysignf(1e-30f, d.x), dy = fabsf(d.y) > 1e-30f ? d.y : copysignf(1e-30f, d.y), dz = fabsf(d.z) > 1e-30f ? d.z : copysignf(1e-30f, d.z);
    RayGrid g;
    g.cx = (o.x - G.lo[0]) * G.istep[0]; g.cy = (o.y - G.lo[1]) * G.istep[1]; g.cz = (o.z - G.lo[2]) * G.istep[2];
    g.ix = G.step[0] * __builtin_amdgcn_rcpf(dx); g.iy = G.step[1] * __builtin_amdgcn_rcpf(dy); g.iz = G.step[2] * __builtin_amdgcn_rcpf(dz);
    g.cx = -g.cx * g.ix; g.cy = -g.cy * g.iy; g.cz = -g.cz * g.iz;
    g.sx = g.ix < 0.f ? 0x01000302u : 0x03020100u; g.sy = g.iy < 0.f ? 0x01000302u : 0x03020100u; g.sz = g.iz < 0.f ? 0x01000302u : 0x03020100u;
    return g;
}
// b = one child record of a GpuNode4Q: x, y, z words (lo | hi << 16) and the child word.  [tmin, tmax]: where the ray is between all three
// pairs of slabs (tmin unclamped: negative for an origin inside).
RT_DEV void slab_span_q(uint4 b, const RayGrid &r, float &tmin, float &tmax) {
    const uint32_t wx = __builtin_amdgcn_perm(b.x, b.x, r.sx), wy = __builtin_amdgcn_perm(b.y, b.y, r.sy), wz = __builtin_amdgcn_perm(b.z, b.z, r.sz);
    const rt_f2 x = {__builtin_fmaf((float)(wx & 0xFFFFu), r.ix, r.cx), __builtin_fmaf((float)(wx >> 16), r.ix, r.cx)}; // (entry, exit) along x
    const rt_f2 y = {__builtin_fmaf((float)(wy & 0xFFFFu), r.iy, r.cy), __builtin_fmaf((float)(wy >> 16), r.iy, r.cy)};
    const rt_f2 z = {__builtin_fmaf((float)(wz & 0xFFFFu), r.iz, r.cz), __builtin_fmaf((float)(wz >> 16), r.iz, r.cz)};
    tmin = fmaxf(fmaxf(x.x, y.x), z.x);
    tmax = fminf(fminf(x.y, y.y), z.y);
}
// Whether [tmin, tmax] overlaps [0, tbest] (tbest >= 0): max(tmin, 0) <= min(tmax, tbest), one compare.  `key`: the bits of max(tmin, 0), the
// sort key of the child's entry distance (a float >= 0 orders like its bits; never 0xFFFFFFFF, the key of a child that is not entered).
RT_DEV bool slab_enter_q(uint4 b, const RayGrid &r, float tbest, uint32_t &key) {
    float tmin, tmax;
    slab_span_q(b, r, tmin, tmax);
    const float t0 = fmaxf(tmin, 0.f);
    key = __float_as_uint(t0);
    return t0 <= fminf(tmax, tbest);
}
// The same decision; tnear = tmin as it is, unclamped.
RT_DEV bool slab_test_q(uint4 b, const RayGrid &r, float tbest, float &tnear) {
    float tmax;
    slab_span_q(b, r, tnear, tmax);
    return fmaxf(tnear, 0.f) <= fminf(tmax, tbest);
}
// With no bound on t (the light sums enter every box on the ray): slab_test_q at tbest = inf.
RT_DEV bool slab_test_q(uint4 b, const RayGrid &r) {
    float tmin, tmax;
    slab_span_q(b, r, tmin, tmax);
    return fmaxf(tmin, 0.f) <= tmax;
}

#define RT_LEAF_BIT 0x80000000u
#define RT_EMPTY_LEAF 0xFFFFFFFFu

struct HitRec {
    int idx;       // BVH-order triangle index or -1
    float t, u, v;
    bool inside;
};

struct Counters { unsigned long long closest, lightq, nodes, tris; };

// Closest hit with the reference's tie rule: smallest t, equal t -> lowest figure index
// (bvh.h:111-142 visits figures in increasing index order and replaces only on strict '<').
// STRIDE: distance in words between consecutive stack entries (1 = a private array; the persistent kernel's exact role interleaves its lanes' stacks in LDS)
template <bool COUNT, int STRIDE = 1>
RT_DEV HitRec closest_hit(const SceneView &S, F3 o, F3 d, uint32_t *stack, Counters &cnt) {
    HitRec best;
    best.idx = -1; best.t = RT_T_MAX; best.u = 0.f; best.v = 0.f; best.inside = false;
    if (COUNT) cnt.closest++;
    RayInv ray = make_ray_inv(o, d);
    int sp = 0;
    uint32_t cur = 0; // root is always an inner node
    for (;;) {
        if (!(cur & RT_LEAF_BIT)) {
            const float4 *q = reinterpret_cast<const float4 *>(S.nodes + cur);
            float4 lo0 = q[0], hi0 = q[1], lo1 = q[2], hi1 = q[3];
            if (COUNT) cnt.nodes++;
            float n0, n1;
            bool h0 = slab_test(lo0, hi0, ray, best.t, n0);
            bool h1 = slab_test(lo1, hi1, ray, best.t, n1);
            uint32_t c0 = __float_as_uint(lo0.w), c1 = __float_as_uint(lo1.w);
            if (h0 & h1) {
                bool swap = n1 < n0;
                stack[STRIDE * sp++] = swap ? c0 : c1;
                cur = swap ? c1 : c0;
                continue;
            }
            if (h0) { cur = c0; continue; }
            if (h1) { cur = c1; continue; }
        } else if (cur != RT_EMPTY_LEAF) {
            uint32_t i = cur & ~RT_LEAF_BIT;
            for (;;) {
                TriIsect T = load_isect(S.tri_walk + i);
                if (COUNT) cnt.tris++;
                float t, u, v; bool inside;
                const int fi = (int)(T.pad >> 1); // index in the figure order
                if (tri_test(T, o, d, t, u, v, inside) && (t < best.t || (t == best.t && fi < best.idx))) {
                    best.t = t; best.u = u; best.v = v; best.inside = inside; best.idx = fi;
                }
                if (T.pad & 1u) break; // last triangle of this leaf
                i++;
            }
        }
        if (sp == 0) break;
        cur = stack[STRIDE * --sp];
    }
    return best;
}

// ---- light pdf: one light's term of the all-hits sum (FiguresMix::getTotalPdf; the sum itself: light_pdf_sum, rt_kernels_hw8.h) ----
RT_DEV float light_pdf_one(const LightRec *L, F3 x, F3 d, bool &last, bool geometric_normal = false) {
    TriIsect T = load_isect(&L->isect);
    last = T.pad != 0;
    float t, u, v; bool inside;
    if (!tri_test(T, x, d, t, u, v, inside)) return 0.f;
    // (t cannot be NaN here: tri_test requires t > 0; distributions.h:141-143 is dead code)
    const float4 *q = reinterpret_cast<const float4 *>(L) + 3;
    float4 q1 = q[1], q2 = q[2], q3 = q[3];
    // (q[0] = b.xyz c.x, used by the sampler only) | q1 = c.yz point_prob n3.x | q2 = n3.yz dn1.xy | q3 = dn1.z dn2.xyz
    float point_prob = q1.z;
    F3 n3 = f3(q1.w, q2.x, q2.y), dn1 = f3(q2.z, q2.w, q3.x), dn2 = f3(q3.y, q3.z, q3.w);
    F3 sn = n3 + u * dn1 + v * dn2;           // primitives.cpp:110
    sn = normalize(sn);                        // :117
    if (inside) sn = neg(sn);                  // :118-119
    if (geometric_normal) { F3 n = f3(T.nx, T.ny, T.nz); sn = normalize(inside ? neg(n) : n); } // hw7: yn of the intersection
    F3 y = x + t * d;                          // distributions.h:144
    return point_prob * len2(x - y) / fabsf(dot(d, sn)); // :68-70 (pdfOne, shading normal in hw8)
}

// ---- textures (scene.cpp:9-53) --------------------------------------------------------------------
// Texels are RGB8; one (unaligned) 4-byte load fetches all three channels — the texel array ends with four spare bytes (scene_prep.cpp).
// 32-bit offsets: an image has fewer than 2^32 / 3 texels (checked at scene preparation).
RT_DEV F3 load_texel(const SceneView &S, const GpuImage &im, int ix, int iy, bool srgb) {
    const uint32_t off = 3u * ((uint32_t)ix + (uint32_t)im.width * (uint32_t)iy);
    if (off + 2u >= (uint32_t)im.width * (uint32_t)im.height * 3u) return f3(0.f, 0.f, 0.f); // reference reads OOB here (UB)
    uint32_t w;
    __builtin_memcpy(&w, S.texels + im.offset + off, 4);
    const uint32_t r = w & 255u, g = (w >> 8) & 255u, b = (w >> 16) & 255u;
    if (srgb) return f3(S.srgb_lut[r], S.srgb_lut[g], S.srgb_lut[b]);
    const float k = (float)(1. / 255);
    return f3(k * (1.f * (float)r), k * (1.f * (float)g), k * (1.f * (float)b));
}
RT_DEV F3 sample_texture(const SceneView &S, GpuImage im, float tx, float ty, bool srgb); // with the image's descriptor already loaded
RT_DEV F3 sample_texture(const SceneView &S, int slot, float tx, float ty, bool srgb) { return sample_texture(S, S.images[slot], tx, ty, srgb); }
RT_DEV F3 sample_texture(const SceneView &S, GpuImage im, float tx, float ty, bool srgb) {
    tx -= floorf(tx);
    ty -= floorf(ty);
    tx *= im.width;
    ty *= im.height;
    // (i + 1) % size without the integer division: i lies in [0, size] (size itself when the product rounds up), so one subtraction wraps it
    int ix1 = (int)floorf(tx), ix2 = ix1 + 1; if (ix2 >= im.width) ix2 -= im.width;
    int iy1 = (int)floorf(ty), iy2 = iy1 + 1; if (iy2 >= im.height) iy2 -= im.height;
    float dx = tx - ix1;
    float dy = ty - iy1;
    F3 p11 = load_texel(S, im, ix1, iy1, srgb);
    F3 p12 = load_texel(S, im, ix1, iy2, srgb);
    F3 p21 = load_texel(S, im, ix2, iy1, srgb);
    F3 p22 = load_texel(S, im, ix2, iy2, srgb);
    return (1 - dx) * ((1 - dy) * p11 + dy * p12) + dx * ((1 - dy) * p21 + dy * p22);
}
RT_DEV F3 apply_normal_map(F3 sn, F3 tan, float tanw, F3 sample) {
    F3 lx = tan, lz = sn;
    F3 ly = tanw * crossr(lx, lz);
    F3 ln = 2.f * sample - f3(1.f, 1.f, 1.f);
    F3 n = ln.x * lx + ln.y * ly + ln.z * lz;
    return normalize(n);
}

// ---- BRDF (material.h:11-65) -----------------------------------------------------------------------
#define RT_PI 3.14159265358979323846
RT_DEV float distribution_term(F3 h, F3 n, float alpha2) {
    float dotHN = dot(h, n);
    if (dotHN <= 0) return 0.f;
    double q = (double)smax(0.f, (alpha2 - 1) * dotHN * dotHN + 1);
    return (float)((double)alpha2 / (RT_PI * (q * q)));
}
RT_DEV float v1_term(F3 n, F3 x, float alpha2) {
    float nx = dot(n, x);
    return (float)(1. / (fabs((double)nx) + sqrt((double)smax(0.f, alpha2 + (1 - alpha2) * nx * nx))));
}
RT_DEV float specular_brdf(F3 l, F3 v, F3 n, float alpha2) {
    F3 h = normalize(l + v);
    if ((double)dot(h, l) < 1e-4 || (double)dot(h, v) < 1e-4) return 0.f;
    return distribution_term(h, n, alpha2) * v1_term(n, l, alpha2) * v1_term(n, v, alpha2);
}
RT_DEV float pow5_d2f(float b) { // (float)pow((double)b, 5.0): three double products, <= 1.5 ulp(double)
    double x = (double)b, x2 = x * x;
    return (float)(x2 * x2 * x);
}
RT_DEV F3 fresnel_term(F3 f0, F3 f90, F3 v, F3 h) {
    float k = pow5_d2f(smax(0.f, 1.f - fabsf(dot(v, h))));
    return f0 + k * (f90 - f0);
}
RT_DEV F3 material_brdf(F3 base_color, float base_metallic, F3 l, F3 v, F3 n, F3 color, float metallic, float alpha) {
    F3 h = normalize(l + v);
    float specular = specular_brdf(l, v, n, alpha * alpha);
    F3 metal = f3(0.f, 0.f, 0.f), dielectric = f3(0.f, 0.f, 0.f);
    metallic *= base_metallic;
    if (metallic > 0 && dot(v, n) >= 0 && dot(l, n) >= 0) {
        F3 ft = fresnel_term(base_color * color, f3(1.f, 1.f, 1.f), v, h);
        metal = specular * ft;
    }
    if (metallic < 1) {
        F3 diffuse = f3(0.f, 0.f, 0.f);
        if (dot(l, n) >= 0) diffuse = (float)(1. / RT_PI) * (base_color * color);
        F3 ft = fresnel_term(f3(0.04f, 0.04f, 0.04f), f3(1.f, 1.f, 1.f), v, h);
        dielectric = diffuse * (f3(1.f, 1.f, 1.f) - ft) + specular * ft;
    }
    return (1.0f - metallic) * dielectric + metallic * metal;
}

// material_brdf with its two products formed by the caller (bc = base_color * color, metallic = texture metallic * baseMetallic —
// the same single multiplications, so the same values): the shader computes them before it samples a direction and so carries
// four values instead of eight through the sampling code.
RT_DEV F3 material_brdf_pre(F3 bc, float metallic, F3 l, F3 v, F3 n, float alpha) {
    F3 h = normalize(l + v);
    float specular = specular_brdf(l, v, n, alpha * alpha);
    F3 metal = f3(0.f, 0.f, 0.f), dielectric = f3(0.f, 0.f, 0.f);
    if (metallic > 0 && dot(v, n) >= 0 && dot(l, n) >= 0) {
        F3 ft = fresnel_term(bc, f3(1.f, 1.f, 1.f), v, h);
        metal = specular * ft;
    }
    if (metallic < 1) {
        F3 diffuse = f3(0.f, 0.f, 0.f);
        if (dot(l, n) >= 0) diffuse = (float)(1. / RT_PI) * bc;
        F3 ft = fresnel_term(f3(0.04f, 0.04f, 0.04f), f3(1.f, 1.f, 1.f), v, h);
        dielectric = diffuse * (f3(1.f, 1.f, 1.f) - ft) + specular * ft;
    }
    return (1.0f - metallic) * dielectric + metallic * metal;
}

// hw7/src/include/material.h:44-61: per-material colour and metallic only, and none of hw8's v.n / l.n gates
RT_DEV F3 material_brdf_hw7(F3 base_color, float base_metallic, F3 l, F3 v, F3 n, float alpha2) {
    F3 h = normalize(l + v);
    float specular = specular_brdf(l, v, n, alpha2);
    F3 metal = f3(0.f, 0.f, 0.f), dielectric = f3(0.f, 0.f, 0.f);
    float metallic = base_metallic;
    if (metallic > 0) metal = specular * fresnel_term(base_color, f3(1.f, 1.f, 1.f), v, h);
    if (metallic < 1) {
        F3 diffuse = (float)(1. / RT_PI) * base_color;
        F3 ft = fresnel_term(f3(0.04f, 0.04f, 0.04f), f3(1.f, 1.f, 1.f), v, h);
        dielectric = diffuse * (f3(1.f, 1.f, 1.f) - ft) + specular * ft;
    }
    return (1.0f - metallic) * dielectric + metallic * metal;
}

// ---- samplers (distributions.h) --------------------------------------------------------------------
RT_DEV F3 cosine_sample(Rng &rng, F3 n) { // :42-52
    float a, b, c;
    rng_n01x3(rng, a, b, c);
    F3 d = normalize(f3(a, b, c));
    d = d + n;
    float l = len(d);
    const float ceps = 1e-9f;
    if (l <= ceps || dot(d, n) <= ceps || l != l) return n;
    return (1.0f / l) * d;
}
RT_DEV float cosine_pdf(F3 n, F3 d) { return smax(0.f, dot(d, n) / (float)RT_PI); } // :54-57

RT_DEV Quat vndf_getq(F3 n) { // :212-224
    Quat q;
    float nz = dot(n, f3(0.f, 0.f, 1.f));
    if ((double)nz > 0.9999) { q.v = f3(0.f, 0.f, 0.f); q.w = 1.f; return q; }
    if ((double)nz < -0.9999) { q.v = f3(0.f, 0.f, 0.f); q.w = -1.f; return q; }
    F3 a = crossr(n, f3(0.f, 0.f, 1.f));
    float w = (float)(sqrt((double)len2(n)) + (double)nz);
    float l = sqrtf(len2(a) + w * w);
    q.v = (1.0f / l) * a;
    q.w = w / l;
    return q;
}
// The two uniform draws of the sampler and the point they give on the unit disk (:178-182).  Split from the rest so that a caller can
// take the draws — and the double-precision sin / cos, the register-hungriest part — before it builds the frame around v: the random
// stream and every value are the same in either order.
RT_DEV void vndf_disk_point(Rng &rng, float &t1, float &t2) {
    float u1 = rng_u01(rng), u2 = rng_u01(rng);
    float r = sqrtf(u1);
    float phi = (float)(2.0 * RT_PI * (double)u2);
    t1 = (float)((double)r * cos((double)phi));
    t2 = (float)((double)r * sin((double)phi));
}
RT_DEV F3 vndf_sample_local(float t1, float t2, F3 v, float alpha) { // :170-194 (Heitz 2018)
    F3 vh = normalize(f3(alpha * v.x, alpha * v.y, v.z));
    float lensq = vh.x * vh.x + vh.y * vh.y;
    F3 T1 = lensq > 0 ? (float)(1. / sqrt((double)lensq)) * f3(-vh.y, vh.x, 0.f) : f3(1.f, 0.f, 0.f);
    F3 T2 = crossr(T1, vh);
    float s = 0.5f * (1.0f + vh.z);
    t2 = (float)((1.0 - (double)s) * sqrt((double)(1.f - t1 * t1)) + (double)(s * t2));
    float rem = (float)(1.0 - (double)(t1 * t1) - (double)(t2 * t2));
    F3 nh = t1 * T1 + t2 * T2 + sqrtf(smax(0.f, rem)) * vh;
    F3 ne = normalize(f3(alpha * nh.x, alpha * nh.y, smax(0.0f, nh.z)));
    return (2 * dot(ne, v)) * ne - v;
}
RT_DEV float vndf_D(F3 n, float a) { // :196-198
    double q = (double)(n.x * n.x / (a * a) + n.y * n.y / (a * a) + n.z * n.z);
    return (float)(1. / (RT_PI * (double)a * (double)a * (q * q)));
}
RT_DEV float vndf_G1(F3 v, float a) { // :200-203
    float q = 1 + (a * a * v.x * v.x + a * a * v.y * v.y) / (v.z * v.z);
    float lambda = (float)(0.5 * (-1 + sqrt((double)q)));
    return 1.0f / (1 + lambda);
}
RT_DEV float vndf_pdf_local(F3 d, F3 v, float a) { // :205-210
    F3 ni = normalize(v + d);
    float dv = vndf_G1(v, a) * smax(0.f, dot(v, ni)) * vndf_D(ni, a) / fabsf(v.z);
    return dv / (4 * dot(v, ni));
}
RT_DEV F3 vndf_sample(Rng &rng, F3 n, F3 v, float alpha) { // :229-237
    float t1, t2;
    vndf_disk_point(rng, t1, t2);
    v = neg(v);
    Quat q = vndf_getq(n);
    F3 vT = qtransform(q, v);
    F3 dT = vndf_sample_local(t1, t2, vT, alpha);
    return qtransform(qconj(q), dT);
}
RT_DEV float vndf_pdf(F3 n, F3 d, F3 v, float alpha) { // :239-245
    v = neg(v);
    Quat q = vndf_getq(n);
    return vndf_pdf_local(qtransform(q, d), qtransform(q, v), alpha);
}
// The same two with the frame given: q = vndf_getq(n) and vT = qtransform(q, -v), which both build from the same normal and direction.
// A caller that needs the sample and the pdf forms the frame once.
RT_DEV F3 vndf_sample(Rng &rng, Quat q, F3 vT, float alpha) {
    float t1, t2;
    vndf_disk_point(rng, t1, t2);
    F3 dT = vndf_sample_local(t1, t2, vT, alpha);
    return qtransform(qconj(q), dT);
}
RT_DEV float vndf_pdf(Quat q, F3 vT, F3 d, float alpha) {
    return vndf_pdf_local(qtransform(q, d), vT, alpha);
}
RT_DEV F3 light_sample(const SceneView &S, Rng &rng, F3 x) { // :117-120, :81-94
    int k = (int)(rng_u01(rng) * S.n_lights_f);
    const LightRec *L = S.lights + k;
    const float4 *q = reinterpret_cast<const float4 *>(L);
    float4 a4 = q[0], q0 = q[3], q1 = q[4];
    F3 a = f3(a4.x, a4.y, a4.z), b = f3(q0.x, q0.y, q0.z), c = f3(q0.w, q1.x, q1.y);
    float u = rng_u01(rng);
    float v = rng_u01(rng);
    if ((double)(u + v) > 1.) { u = 1 - u; v = 1 - v; }
    F3 point = a + u * b + v * c;
    return normalize(point - x);
}

// ---- epilogue (color.cpp:4-31) -----------------------------------------------------------------------
RT_DEV float aces1(float x) {
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    float q = (x * (a * x + b)) / (x * (c * x + d) + e);
    return smin(1.f, smax(0.f, q));
}
RT_DEV uint8_t tonemap1(float x) {
    const float gamma = (float)(1. / 2.2);
    float g = (float)pow((double)aces1(x), (double)gamma);
    return (uint8_t)round((double)(255 * g));
}

// Pixel slot -> pixel: slots run through the 8x8 sub-tiles of this shard's tiles (slot >> 6 = sub-tile, slot & 63 = pixel in it).
// n / d and n % d for n < 2^24 (exact as a float) and a wave-uniform d: a multiplication by the reciprocal and one correction step instead of
// the ~30 instructions of a 32-bit integer division.
RT_DEV uint32_t udiv24(uint32_t n, uint32_t d, float rcp_d, uint32_t &rem) {
    uint32_t q = (uint32_t)((float)n * rcp_d);
    int r = (int)(n - q * d);
    if (r < 0) { q--; r += (int)d; } else if (r >= (int)d) { q++; r -= (int)d; }
    rem = (uint32_t)r;
    return q;
}
// The end of the mapping, shared with for_each_pixel: shard-local tile st at (gtx, gty) of the tile grid, 8x8 sub-tile (sx, sy) in it, pixel `lane` of that.
RT_DEV void subtile_to_pixel(const RenderView &R, uint32_t st, uint32_t gtx, uint32_t gty, uint32_t sx, uint32_t sy, uint32_t lane, int &x, int &y, bool &inside, size_t &out_index) {
    int tx0 = (int)gtx * R.tile_w, ty0 = (int)gty * R.tile_h;
    int lx = (int)sx * 8 + (int)(lane & 7), ly = (int)sy * 8 + (int)(lane >> 3);
    x = tx0 + lx; y = ty0 + ly;
    inside = x < R.width && y < R.height;
    out_index = R.shard_count > 1 ? ((size_t)st * R.tile_h + ly) * R.tile_w + lx : (size_t)y * R.width + x;
}
RT_DEV void slot_to_pixel(const RenderView &R, uint32_t slot, int &x, int &y, bool &inside, size_t &out_index) {
    const int sub_x = R.tile_w >> 3, sub_per_tile = sub_x * (R.tile_h >> 3);
    uint32_t w = slot >> 6, lane = slot & 63u; // w < 2^24: a launch holds fewer than 2^30 slots
    uint32_t sub, st = udiv24(w, (uint32_t)sub_per_tile, __builtin_amdgcn_rcpf((float)sub_per_tile), sub);
    uint32_t gt = R.shard_count > 1 ? (uint32_t)R.shard_index + st * (uint32_t)R.shard_count : st;
    uint32_t gtx, gty, sx, sy;
    if (gt < (1u << 24)) gty = udiv24(gt, (uint32_t)R.tiles_x, __builtin_amdgcn_rcpf((float)R.tiles_x), gtx);
    else { gty = gt / (uint32_t)R.tiles_x; gtx = gt % (uint32_t)R.tiles_x; }
    sy = udiv24(sub, (uint32_t)sub_x, __builtin_amdgcn_rcpf((float)sub_x), sx);
    subtile_to_pixel(R, st, gtx, gty, sx, sy, lane, x, y, inside, out_index);
}

// One finished pixel: the float radiance and its tonemapped bytes (sceneio.cpp:393-395), whichever buffers the caller asked for; and the black
// pixel that pads a border tile in the compact shard layout.  `lit` = false is the black pixel: the bytes are then 0 and the caller passes px = 0 too,
// since the floats are always written from px.  The shell stores both kinds through this one block (a branch per kind cost hw2-hw4 up to 21 more SGPR spills).
RT_DEV void store_pixel(const RenderView &R, size_t out_index, F3 px, bool lit = true) {
    if (R.out_rgb) { R.out_rgb[3 * out_index] = px.x; R.out_rgb[3 * out_index + 1] = px.y; R.out_rgb[3 * out_index + 2] = px.z; }
    if (R.out_rgb8) {
        R.out_rgb8[3 * out_index] = lit ? tonemap1(px.x) : 0;
        R.out_rgb8[3 * out_index + 1] = lit ? tonemap1(px.y) : 0;
        R.out_rgb8[3 * out_index + 2] = lit ? tonemap1(px.z) : 0;
    }
}
RT_DEV void store_pixel_zero(const RenderView &R, size_t out_index) { store_pixel(R, out_index, f3(0.f, 0.f, 0.f), false); }

// The shell of the per-pixel kernels hw2-hw5 (the hw8 megakernel spells the same loop out, rt_kernels_hw8.h), one wave per block: waves are persistent and pull work items from a
// global queue (the GPU form of `#pragma omp parallel for schedule(dynamic,8)`, hw8/src/sceneio.cpp:387).  A work item is one 8x8 sub-tile of
// a shard tile (tile_w x tile_h, multiples of 8), one lane per pixel.  body(x, y) -> F3 runs for the pixels inside the image; the padding of a
// border tile is written black in the compact shard layout and not at all in a whole frame.
template <class BODY>
RT_DEV void for_each_pixel(const RenderView &R, uint32_t n_work, const BODY &body) {
    const uint32_t lane = threadIdx.x & 63u;
    const int sub_x = R.tile_w >> 3, sub_per_tile = sub_x * (R.tile_h >> 3);
    for (;;) {
        uint32_t w = 0;
        if (lane == 0) w = atomicAdd(R.work_counter, 1u);
        w = __shfl(w, 0);
        if (w >= n_work) break;
        uint32_t st = w / sub_per_tile, sub = w % sub_per_tile; // shard-local tile, 8x8 block inside it: plain divisions, w is wave-uniform
        uint32_t gt = R.shard_count > 1 ? (uint32_t)R.shard_index + st * (uint32_t)R.shard_count : st;
        int x, y; bool inside; size_t out_index;
        subtile_to_pixel(R, st, gt % (uint32_t)R.tiles_x, gt / (uint32_t)R.tiles_x, sub % sub_x, sub / sub_x, lane, x, y, inside, out_index);
        F3 px = f3(0.f, 0.f, 0.f);
        if (inside) px = body(x, y);
        if (inside || R.shard_count > 1) store_pixel(R, out_index, px, inside);
    }
}
// The pixel's mean over R.samples camera samples: its own minstd_rand(y*W+x) (sceneio.cpp:389-391), two jitter draws per sample, then
// sample(rng, fx, fy) -> F3 with the jittered pixel coordinates; scaled by the float 1/spp (scene.cpp:171-176).
template <class SAMPLE>
RT_DEV F3 average_samples(const RenderView &R, int x, int y, const SAMPLE &sample) {
    Rng rng;
    rng_seed(rng, (uint32_t)(y * R.width + x));
    F3 color = f3(0.f, 0.f, 0.f);
    for (int s = 0; s < R.samples; s++) {
        float fx = (float)x + rng_u01(rng);
        float fy = (float)y + rng_u01(rng);
        color = color + sample(rng, fx, fy);
    }
    return R.inv_samples * color;
}

// Pixel slot of a shard -> pixel slot of the unsharded frame (its "frame order": the 8x8 sub-tiles of the image row-major, 64 slots each),
// the order a portable checkpoint keeps the state in (rt_multi_accum_save).  `tile` = side of the shard's square tiles, tiles_x = tiles per
// row, sub_w x sub_h = ceil(W/8) x ceil(H/8).  false: the slot lies in a sub-tile wholly outside the image (padding of a border tile),
// which the frame order does not have.  Same divisions as slot_to_pixel on the device; the host (tests, no GPU) divides plainly.
__host__ __device__ inline bool shard_slot_to_frame_slot(int tile, int tiles_x, int sub_w, int sub_h, uint32_t shard_index, uint32_t shard_count, uint32_t slot, uint32_t &frame_slot) {
    const uint32_t sub_x = (uint32_t)tile >> 3, sub_per_tile = sub_x * sub_x;
    const uint32_t w = slot >> 6, lane = slot & 63u; // w < 2^24, as in slot_to_pixel
    uint32_t sub, st, gtx, gty, sx, sy;
#if defined(__HIP_DEVICE_COMPILE__)
    st = udiv24(w, sub_per_tile, __builtin_amdgcn_rcpf((float)sub_per_tile), sub);
    const uint32_t gt = shard_index + st * shard_count;
    if (gt < (1u << 24)) gty = udiv24(gt, (uint32_t)tiles_x, __builtin_amdgcn_rcpf((float)tiles_x), gtx);
    else { gty = gt / (uint32_t)tiles_x; gtx = gt % (uint32_t)tiles_x; }
    sy = udiv24(sub, sub_x, __builtin_amdgcn_rcpf((float)sub_x), sx);
#else
    st = w / sub_per_tile; sub = w % sub_per_tile;
    const uint32_t gt = shard_index + st * shard_count;
    gty = gt / (uint32_t)tiles_x; gtx = gt % (uint32_t)tiles_x;
    sy = sub / sub_x; sx = sub % sub_x;
#endif
    const uint32_t gx = gtx * sub_x + sx, gy = gty * sub_x + sy;
    frame_slot = ((gy * (uint32_t)sub_w + gx) << 6) | lane;
    return gx < (uint32_t)sub_w && gy < (uint32_t)sub_h;
}

} // namespace dev
} // namespace rtamd

// Preview filter of a noisy frame (include/rtamd.h: rt_denoise, rt_accum_denoise): an edge-avoiding a-trous wavelet filter over the
// first-hit guide images, its luminance stop steered by the noise monitor's error map.  Two kernels:
//   denoise_pack_kernel   one lane per pixel: the planes -> two 16-byte records per pixel and the depth gradient; counts the fixed pixels
//   denoise_level_kernel  one lane per pixel, 64x4 blocks: the 25 taps of one level at stride 2^i; the last level remodulates and tonemaps
// A pixel is summed by one lane over its taps in a fixed order (dy outer, dx inner), so the bits depend on nothing but the planes: not on
// the block shape, the launch geometry or a second run.  No float atomics.  All arithmetic is float32 with one rounding per operation
// (the build's -ffp-contract=off) and no transcendental function, written so that tests/denoise_model.py restates it in numpy bit for bit.
#pragma once
#include "rt_device.h"

namespace rtamd {

struct DenoiseView {
    int32_t width, height;
    uint32_t n;                         // width * height <= 2^26
    // the planes as given, row-major, row 0 first
    const float *rgb, *normal, *depth;  // n*3, n*3, n
    const float *albedo, *emission;     // n*3 each, nullable
    const float *se;                    // n, nullable
    // the working set
    float4 *geo;                        // {n.x, n.y, n.z, z}; z < 0 marks a fixed pixel
    float4 *irr_in, *irr_out;           // {irr r, g, b, v}: read / written by a level (a fixed pixel keeps its rgb as given here)
    float2 *grad;                       // depth gradient {gx, gy}
    unsigned long long *fixed_pixels;
    // one level
    int32_t step;                       // 1 << i
    uint32_t last;                      // this level writes the picture instead of irr_out
    float sigma_depth, sigma_luminance;
    float *out_rgb;                     // n*3, nullable
    uint8_t *out_rgb8;                  // n*3, nullable
};

namespace dev {

#define DN_ALBEDO_FLOOR 0.015625f   // 1 / 64
#define DN_EPS_DEPTH_REL 1e-3f
#define DN_EPS_DEPTH_ABS 1e-12f
#define DN_EPS_LUMINANCE 1e-6f

RT_DEV float dn_luminance(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }
RT_DEV bool dn_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
RT_DEV bool dn_finite3(const float *p) { return dn_finite(p[0]) && dn_finite(p[1]) && dn_finite(p[2]); }
// about exp(-x): max(0, 1 - x / 16) squared four times; zero from x = 16, and for a NaN
RT_DEV float dn_e16(float x) {
    float t = smax(0.f, 1.f - x * 0.0625f);
    t = t * t; t = t * t; t = t * t; t = t * t;
    return t;
}
// the albedo the irradiance is divided by and multiplied with again: floored per channel, 1 without an albedo plane
RT_DEV void dn_albedo(const DenoiseView &V, size_t p, float a[3]) {
    for (int k = 0; k < 3; k++) a[k] = V.albedo ? smax(DN_ALBEDO_FLOOR, V.albedo[3 * p + k]) : 1.f;
}

// Planes -> records.  A pixel is fixed when it is a miss (depth not > 0), when it emits, or when one of its inputs is not finite: it
// comes out as it went in and is nobody's neighbour.  Everything of `rgb` is read here, so the last level may write over it.
__global__ __launch_bounds__(256) void denoise_pack_kernel(DenoiseView V) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool fixed = false;
    if (p < V.n) {
        const int W = V.width, H = V.height;
        const int y = (int)(p / (uint32_t)W), x = (int)(p - (uint32_t)y * (uint32_t)W);
        const float *rgb = V.rgb + 3 * (size_t)p, *nrm = V.normal + 3 * (size_t)p;
        const float z = V.depth[p];
        fixed = !(z > 0.f) || !dn_finite(z) || !dn_finite3(rgb) || !dn_finite3(nrm);
        if (V.emission) { const float *e = V.emission + 3 * (size_t)p; fixed = fixed || e[0] != 0.f || e[1] != 0.f || e[2] != 0.f; }
        if (V.albedo) fixed = fixed || !dn_finite3(V.albedo + 3 * (size_t)p);
        if (V.se) fixed = fixed || !dn_finite(V.se[p]);
        float a[3];
        dn_albedo(V, p, a);
        float4 c = make_float4(rgb[0], rgb[1], rgb[2], 0.f);
        if (!fixed) {
            c.x = c.x / a[0]; c.y = c.y / a[1]; c.z = c.z / a[2];
            if (V.se) { const float s = V.se[p] / dn_luminance(a[0], a[1], a[2]); c.w = s * s; }
        }
        const int xr = x + 1 < W ? x + 1 : W - 1, xl = x > 0 ? x - 1 : 0;
        const int yr = y + 1 < H ? y + 1 : H - 1, yl = y > 0 ? y - 1 : 0;
        float2 g = make_float2(0.f, 0.f);
        if (xr != xl) g.x = (V.depth[(size_t)y * W + xr] - V.depth[(size_t)y * W + xl]) / (float)(xr - xl);
        if (yr != yl) g.y = (V.depth[(size_t)yr * W + x] - V.depth[(size_t)yl * W + x]) / (float)(yr - yl);
        V.geo[p] = make_float4(nrm[0], nrm[1], nrm[2], fixed ? -1.f : z);
        V.irr_out[p] = c;
        V.grad[p] = g;
    }
    const uint32_t n_fixed = (uint32_t)__popcll(__ballot(fixed));
    if ((threadIdx.x & 63u) == 0u && n_fixed) atomicAdd(V.fixed_pixels, (unsigned long long)n_fixed);
}

// One level.  HAS_SE: the error map steers a luminance stop; its variance is carried along and smoothed over 3x3 before it is used.
template <bool HAS_SE>
__global__ __launch_bounds__(256) void denoise_level_kernel(DenoiseView V) {
    const int W = V.width, H = V.height;
    const uint32_t blocks_x = ((uint32_t)W + 63u) >> 6;
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const int x = (int)(bx * 64u + threadIdx.x), y = (int)(by * 4u + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 gp = V.geo[p];
    float4 c = V.irr_in[p];
    const bool fixed = gp.w < 0.f;
    if (!fixed) {
        float sd = 0.f, yp = 0.f;
        if (HAS_SE) {
            float num = 0.f, den = 0.f;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    if (V.geo[q].w < 0.f) continue;
                    const float g = (dy ? 0.25f : 0.5f) * (dx ? 0.25f : 0.5f);
                    num = num + g * V.irr_in[q].w;
                    den = den + g;
                }
            sd = sqrtf(smax(0.f, num / den));
            yp = dn_luminance(c.x, c.y, c.z);
        }
        const float2 grad = V.grad[p];
        const float k5[3] = {0.375f, 0.25f, 0.0625f};
        float ar = 0.f, ag = 0.f, ab = 0.f, accw = 0.f, accv = 0.f;
        for (int dy = -2; dy <= 2; dy++) {
            const int oy = dy * V.step, qy = y + oy;
            if (qy < 0 || qy >= H) continue;
            for (int dx = -2; dx <= 2; dx++) {
                const int ox = dx * V.step, qx = x + ox;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                const float4 gq = V.geo[q];
                if (gq.w < 0.f) continue;
                const float4 cq = V.irr_in[q];
                const float h = k5[dy < 0 ? -dy : dy] * k5[dx < 0 ? -dx : dx];
                float wn = smax(0.f, ((gp.x * gq.x) + (gp.y * gq.y)) + (gp.z * gq.z));
                wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn;
                float xs = fabsf(gp.w - gq.w) / (((V.sigma_depth * fabsf((grad.x * (float)ox) + (grad.y * (float)oy))) + (DN_EPS_DEPTH_REL * gp.w)) + DN_EPS_DEPTH_ABS);
                if (HAS_SE) xs = xs + fabsf(yp - dn_luminance(cq.x, cq.y, cq.z)) / ((V.sigma_luminance * sd) + DN_EPS_LUMINANCE);
                const float w = (h * dn_e16(xs)) * wn;
                ar = ar + w * cq.x; ag = ag + w * cq.y; ab = ab + w * cq.z;
                accw = accw + w;
                accv = accv + (w * w) * cq.w;
            }
        }
        if (accw > 0.f) { c.x = ar / accw; c.y = ag / accw; c.z = ab / accw; c.w = accv / (accw * accw); }
    }
    if (!V.last) { V.irr_out[p] = c; return; }
    if (!fixed) {
        float a[3];
        dn_albedo(V, p, a);
        c.x = c.x * a[0]; c.y = c.y * a[1]; c.z = c.z * a[2];
    }
    if (V.out_rgb) { V.out_rgb[3 * p] = c.x; V.out_rgb[3 * p + 1] = c.y; V.out_rgb[3 * p + 2] = c.z; }
    if (V.out_rgb8) { V.out_rgb8[3 * p] = tonemap1(c.x); V.out_rgb8[3 * p + 1] = tonemap1(c.y); V.out_rgb8[3 * p + 2] = tonemap1(c.z); }
}

} // namespace dev
} // namespace rtamd

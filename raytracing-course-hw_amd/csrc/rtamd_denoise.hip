// Denoised previews (include/rtamd.h: rt_denoise, rt_accum_denoise): the argument checks, the working set and the launches of the filter in
// device/rt_denoise.h.  rt_denoise is an image filter: the scene names the GPU, owns the working set and serialises the call.
// rt_accum_denoise composes the public calls on the device -- rt_accum_resolve, rt_render_guides (once per rt_accum), rt_noise_estimate --
// and filters what they wrote; it only reads the accumulator and the monitor.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/rtamd.h"
#include "host/rt_accum_state.h"
#include "device/rt_denoise.h"

using namespace rtamd;

namespace {

const int DENOISE_DEFAULT_ITERATIONS = 5, DENOISE_MAX_ITERATIONS = 8;
const float DENOISE_DEFAULT_SIGMA_DEPTH = 1.f, DENOISE_DEFAULT_SIGMA_LUMINANCE = 4.f;
const int64_t DENOISE_MAX_PIXELS = (int64_t)1 << 26;

// What both calls refuse in their params; `allowed` are the flags the call takes.
int check_params(const rt_denoise_params *p, const rt_denoise_stats *stats, uint32_t allowed, const char *allowed_names, const std::string &who) {
    if (!p) return fail(RT_ERR_INVALID_ARG, who + "null argument (params)");
    if (p->struct_size != sizeof(rt_denoise_params)) return fail(RT_ERR_INVALID_ARG, who + "params: struct_size mismatch (ABI skew)");
    if (stats && stats->struct_size != sizeof(rt_denoise_stats)) return fail(RT_ERR_INVALID_ARG, who + "stats: struct_size mismatch (ABI skew)");
    if (p->reserved != 0) return fail(RT_ERR_INVALID_ARG, who + "reserved must be 0");
    if (p->flags & ~allowed) return fail(RT_ERR_INVALID_ARG, who + "flags other than " + allowed_names);
    if (p->iterations < 0 || p->iterations > DENOISE_MAX_ITERATIONS) return fail(RT_ERR_INVALID_ARG, who + "iterations must be 0 (the default, 5) or 1 .. 8");
    if (!std::isfinite(p->sigma_depth) || p->sigma_depth < 0.f) return fail(RT_ERR_INVALID_ARG, who + "sigma_depth must be finite and not negative (0 = the default, 1)");
    if (!std::isfinite(p->sigma_luminance) || p->sigma_luminance < 0.f) return fail(RT_ERR_INVALID_ARG, who + "sigma_luminance must be finite and not negative (0 = the default, 4)");
    return RT_OK;
}

int check_size(int32_t width, int32_t height, const std::string &who) {
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, who + "width and height must be positive");
    if ((int64_t)width * height > DENOISE_MAX_PIXELS) return fail(RT_ERR_LIMIT, who + "width * height above 2^26");
    return RT_OK;
}

// The planes of one call: where they are, and whether that is device memory of the scene's GPU.
struct DenoisePlanes {
    const float *rgb, *normal, *depth, *albedo, *emission, *se;
    bool in_on_device;
    float *out_rgb; uint8_t *out_rgb8;
    bool out_on_device;
};

// The scene's working set for a frame of n pixels, carved out of one allocation in 256-byte steps: the counter, the records
// (56 bytes per pixel), then room for `floats_per_pixel` floats and `bytes_per_pixel` bytes per pixel of staged planes.
struct DenoiseStage {
    unsigned long long *fixed_pixels;
    float4 *geo, *irr[2];
    float2 *grad;
    float *planes;
    uint8_t *bytes;
};
DenoiseStage denoise_stage(rt_scene *scene, size_t n, size_t floats_per_pixel, size_t bytes_per_pixel) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255u) & ~(size_t)255u; return here; };
    const size_t o_fixed = take(8), o_geo = take(n * 16), o_a = take(n * 16), o_b = take(n * 16), o_grad = take(n * 8),
                 o_planes = take(n * floats_per_pixel * 4), o_bytes = take(n * bytes_per_pixel);
    grow(scene->denoise_stage, scene->denoise_stage_bytes, at);
    uint8_t *b = scene->denoise_stage;
    DenoiseStage s;
    s.fixed_pixels = (unsigned long long *)(b + o_fixed);
    s.geo = (float4 *)(b + o_geo); s.irr[0] = (float4 *)(b + o_a); s.irr[1] = (float4 *)(b + o_b); s.grad = (float2 *)(b + o_grad);
    s.planes = (float *)(b + o_planes); s.bytes = b + o_bytes;
    return s;
}

// Next `floats` floats of the staged planes.
float *take_plane(float *&at, size_t floats) { float *here = at; at += floats; return here; }

// The filter itself, on the null stream of the scene's device (which is current): pack, the levels, the copies; returns when all of it has finished.
// `free_planes`: where in S.planes the staging of host planes may begin (rt_accum_denoise keeps its resolve and its error map in front).
int denoise_run(rt_scene *scene, const rt_denoise_params *p, int32_t width, int32_t height, const DenoisePlanes &io, const DenoiseStage &S, float *free_planes,
                rt_denoise_stats *stats, double t0) {
    hipStream_t stream = nullptr;
    const size_t n = (size_t)width * height;
    const int iterations = p->iterations ? p->iterations : DENOISE_DEFAULT_ITERATIONS;
    DenoiseView V{};
    V.width = width; V.height = height; V.n = (uint32_t)n;
    const struct { const float *from; const float **to; size_t k; } in[6] = {{io.rgb, &V.rgb, 3}, {io.normal, &V.normal, 3}, {io.depth, &V.depth, 1},
                                                                            {io.albedo, &V.albedo, 3}, {io.emission, &V.emission, 3}, {io.se, &V.se, 1}};
    for (const auto &pl : in) {
        *pl.to = pl.from;
        if (!pl.from || io.in_on_device) continue;
        float *d = take_plane(free_planes, n * pl.k);
        HIP_CHECK(hipMemcpyAsync(d, pl.from, n * pl.k * sizeof(float), hipMemcpyHostToDevice, stream));
        *pl.to = d;
    }
    V.out_rgb = io.out_rgb; V.out_rgb8 = io.out_rgb8;
    if (!io.out_on_device) {
        if (io.out_rgb) V.out_rgb = take_plane(free_planes, n * 3);
        if (io.out_rgb8) V.out_rgb8 = S.bytes;
    }
    V.geo = S.geo; V.grad = S.grad; V.fixed_pixels = S.fixed_pixels;
    V.sigma_depth = p->sigma_depth != 0.f ? p->sigma_depth : DENOISE_DEFAULT_SIGMA_DEPTH;
    V.sigma_luminance = p->sigma_luminance != 0.f ? p->sigma_luminance : DENOISE_DEFAULT_SIGMA_LUMINANCE;
    HIP_CHECK(hipMemsetAsync(S.fixed_pixels, 0, 8, stream));
    HIP_CHECK(hipEventRecord(scene->ev_start, stream));
    V.irr_out = S.irr[0];
    hipLaunchKernelGGL(dev::denoise_pack_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, V);
    HIP_CHECK(hipGetLastError());
    const unsigned blocks = (unsigned)((((size_t)width + 63u) / 64u) * (((size_t)height + 3u) / 4u));
    for (int i = 0; i < iterations; i++) {
        V.irr_in = S.irr[i & 1]; V.irr_out = S.irr[(i + 1) & 1];
        V.step = 1 << i; V.last = i == iterations - 1;
        if (V.se) hipLaunchKernelGGL(dev::denoise_level_kernel<true>, dim3(blocks), dim3(64, 4), 0, stream, V);
        else hipLaunchKernelGGL(dev::denoise_level_kernel<false>, dim3(blocks), dim3(64, 4), 0, stream, V);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(scene->ev_stop, stream));
    unsigned long long fixed = 0;
    HIP_CHECK(hipMemcpyAsync(&fixed, S.fixed_pixels, 8, hipMemcpyDeviceToHost, stream));
    if (!io.out_on_device) {
        if (io.out_rgb) HIP_CHECK(hipMemcpyAsync(io.out_rgb, V.out_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (io.out_rgb8) HIP_CHECK(hipMemcpyAsync(io.out_rgb8, V.out_rgb8, n * 3, hipMemcpyDeviceToHost, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    if (stats) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop));
        stats->struct_size = sizeof(rt_denoise_stats);
        stats->launches = 1u + (uint32_t)iterations;
        stats->fixed_pixels = fixed;
        stats->kernel_ms = ms;
        stats->total_ms = now_ms() - t0;
    }
    return RT_OK;
}

// floats per pixel of the planes that denoise_run stages for host memory
size_t host_plane_floats(const DenoisePlanes &io) {
    size_t f = 0;
    if (!io.in_on_device) f += 3 + 3 + 1 + (io.albedo ? 3 : 0) + (io.emission ? 3 : 0) + (io.se ? 1 : 0);
    if (!io.out_on_device && io.out_rgb) f += 3;
    return f;
}

} // namespace

extern "C" {

int rt_denoise(rt_scene *scene, const rt_denoise_params *p, const float *rgb, const float *normal, const float *depth, const float *albedo,
               const float *emission, const float *se, float *out_rgb, uint8_t *out_rgb8, rt_denoise_stats *stats) {
    const std::string who = "rt_denoise: ";
    if (!scene) return fail(RT_ERR_INVALID_ARG, who + "null argument (scene)");
    if (const int rc = check_params(p, stats, RT_DENOISE_DEVICE_POINTERS, "RT_DENOISE_DEVICE_POINTERS", who)) return rc;
    if (!rgb) return fail(RT_ERR_INVALID_ARG, who + "null argument (rgb)");
    if (!normal) return fail(RT_ERR_INVALID_ARG, who + "null argument (normal)");
    if (!depth) return fail(RT_ERR_INVALID_ARG, who + "null argument (depth)");
    if (!out_rgb && !out_rgb8) return fail(RT_ERR_INVALID_ARG, who + "out_rgb and out_rgb8 are both null: nothing to write");
    if (const int rc = check_size(p->width, p->height, who)) return rc;
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        HIP_CHECK(hipSetDevice(scene->device));
        const bool on_device = (p->flags & RT_DENOISE_DEVICE_POINTERS) != 0;
        const DenoisePlanes io{rgb, normal, depth, albedo, emission, se, on_device, out_rgb, out_rgb8, on_device};
        const size_t n = (size_t)p->width * p->height;
        const DenoiseStage S = denoise_stage(scene, n, host_plane_floats(io), !on_device && out_rgb8 ? 3 : 0);
        return denoise_run(scene, p, p->width, p->height, io, S, S.planes, stats, t0);
    });
}

int rt_accum_denoise(rt_accum *a, rt_noise *noise, const rt_denoise_params *p, float *out_rgb, uint8_t *out_rgb8, rt_denoise_stats *stats) {
    const std::string who = "rt_accum_denoise: ";
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument (accum)");
    if (const int rc = check_params(p, stats, RT_DENOISE_DEVICE_POINTERS | RT_DENOISE_ALBEDO, "RT_DENOISE_DEVICE_POINTERS | RT_DENOISE_ALBEDO", who)) return rc;
    if (!out_rgb && !out_rgb8) return fail(RT_ERR_INVALID_ARG, who + "out_rgb and out_rgb8 are both null: nothing to write");
    return guarded(who, [&]() -> int {
        const double t0 = now_ms();
        if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "an earlier slice failed and left the state half advanced (" + a->broken + ")");
        const int32_t width = a->view.width, height = a->view.height;
        if ((p->width != 0 && p->width != width) || (p->height != 0 && p->height != height))
            return fail(RT_ERR_INVALID_ARG, who + "width and height must be 0 or the accumulator's (" + std::to_string(width) + " x " + std::to_string(height) + ")");
        if (a->view.shard_count > 1) return fail(RT_ERR_UNSUPPORTED, who + "a sharded accumulator holds a part of the frame: guide images are made for unsharded frames on one GPU");
        if (a->scene->flavor != RT_INTEGRATOR_HW8)
            return fail(RT_ERR_UNSUPPORTED, who + "guide images serve scenes created for hw8 / hw7 (this one was prepared for integrator " + std::to_string(a->scene->flavor) + ")");
        if (a->samples <= 0) return fail(RT_ERR_INVALID_ARG, who + "no samples yet (a picture needs at least one)");
        if (noise) if (const int rc = noise_estimate_ready(noise, a, who)) return rc;
        if (const int rc = check_size(width, height, who)) return rc;
        rt_scene *scene = a->scene;
        HIP_CHECK(hipSetDevice(scene->device));
        const size_t n = (size_t)width * height;
        if (!a->d_guides) { // the guide planes of this frame: albedo, normal, depth, emission, made once
            OwnedDev planes;
            HIP_CHECK(hipMalloc(&planes.p, n * 10 * sizeof(float)));
            float *g = (float *)planes.p;
            if (const int rc = rt_render_guides(scene, width, height, RT_QUERY_DEVICE_POINTERS, g, g + 3 * n, g + 6 * n, g + 7 * n, nullptr)) return rc;
            a->d_guides = (float *)planes.release();
        }
        const float *g = a->d_guides;
        const bool out_on_device = (p->flags & RT_DENOISE_DEVICE_POINTERS) != 0;
        DenoisePlanes io{nullptr, g + 3 * n, g + 6 * n, (p->flags & RT_DENOISE_ALBEDO) ? g : nullptr, g + 7 * n, nullptr, true, out_rgb, out_rgb8, out_on_device};
        const DenoiseStage S = denoise_stage(scene, n, 3 + (noise ? 1 : 0) + host_plane_floats(io), !out_on_device && out_rgb8 ? 3 : 0);
        float *at = S.planes;
        float *d_rgb = take_plane(at, 3 * n);
        if (const int rc = rt_accum_resolve(a, RT_FLAG_OUT_DEVICE, d_rgb, nullptr)) return rc;
        io.rgb = d_rgb;
        if (noise) {
            float *d_se = take_plane(at, n);
            if (const int rc = rt_noise_estimate(noise, RT_FLAG_OUT_DEVICE, d_se, nullptr)) return rc;
            io.se = d_se;
        }
        return denoise_run(scene, p, width, height, io, S, at, stats, t0);
    });
}

} // extern "C"

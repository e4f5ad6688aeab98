// The argument checks of rt_bake_rays and rt_bake (csrc/rtamd_query.hip) under the host's address and undefined-behaviour sanitizers,
// stand-alone: every refusal that is decided before the scene is looked at, on a null scene, so that no launch is ever reached -- the
// launches are stubs here that abort.  From the repository root:
//   hipcc -x hip -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/sanitize/bake_sanitize.cpp raytracing-course-hw_amd/csrc/rtamd_query.hip \
//       -o /tmp/bake_asan && /tmp/bake_asan
// Prints one line per refusal and "bake_sanitize: N refusals, all as expected"; no GPU, no Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "../../raytracing-course-hw_amd/csrc/device/rt_types_query.h"

namespace {
std::string last_error;
[[noreturn]] uint32_t reached(const char *what) {
    std::fprintf(stderr, "bake_sanitize: %s was reached on a null scene\n", what);
    std::abort();
}
int refusals = 0;
void expect(const char *what, int code, int want_code, const char *want_text) {
    const bool ok = code == want_code && last_error.find(want_text) != std::string::npos;
    std::printf("%-44s %d  %s\n", what, code, last_error.c_str());
    if (!ok) {
        std::fprintf(stderr, "bake_sanitize: %s: wanted code %d and a message with \"%s\"\n", what, want_code, want_text);
        std::exit(1);
    }
    refusals++;
}
} // namespace

namespace rtamd {
void set_error(const std::string &msg) { last_error = msg; }
size_t query_ovf_words(const rt_scene *) { reached("query_ovf_words"); }
uint32_t query_launch_closest(const rt_scene *, const QueryView &, hipStream_t) { reached("query_launch_closest"); }
uint32_t query_launch_light_pdf(const rt_scene *, const QueryView &, hipStream_t) { reached("query_launch_light_pdf"); }
uint32_t query_launch_occluded(const rt_scene *, const QueryView &, hipStream_t) { reached("query_launch_occluded"); }
uint32_t query_launch_material_table(const rt_scene *, uint32_t *, hipStream_t) { reached("query_launch_material_table"); }
uint32_t query_launch_surface(const rt_scene *, const SurfaceView &, hipStream_t) { reached("query_launch_surface"); }
uint32_t query_launch_environment(const rt_scene *, const EnvironmentView &, hipStream_t) { reached("query_launch_environment"); }
uint32_t query_launch_camera_rays(const rt_scene *, const CameraView &, hipStream_t) { reached("query_launch_camera_rays"); }
uint32_t query_launch_guides(const rt_scene *, const GuidesView &, hipStream_t) { reached("query_launch_guides"); }
uint32_t query_launch_scatter_sample(const rt_scene *, const ScatterView &, hipStream_t) { reached("query_launch_scatter_sample"); }
uint32_t query_launch_scatter_finish(const rt_scene *, const ScatterView &, hipStream_t) { reached("query_launch_scatter_finish"); }
uint32_t query_launch_bsdf_rays(const rt_scene *, const ScatterView &, hipStream_t) { reached("query_launch_bsdf_rays"); }
uint32_t query_launch_bsdf_finish(const rt_scene *, const ScatterView &, hipStream_t) { reached("query_launch_bsdf_finish"); }
uint32_t query_launch_path_advance(const rt_scene *, const PathView &, hipStream_t) { reached("query_launch_path_advance"); }
uint32_t query_launch_bake_rays(const rt_scene *, const BakeView &, hipStream_t) { reached("query_launch_bake_rays"); }
uint32_t query_launch_bake_advance(const rt_scene *, const PathView &, const BakeView &, hipStream_t) { reached("query_launch_bake_advance"); }
uint32_t query_launch_bake_resolve(const rt_scene *, const BakeView &, hipStream_t) { reached("query_launch_bake_resolve"); }
} // namespace rtamd

int main() {
    const size_t n = 8, K = 4;
    // exactly as large as the calls may read: one byte more and the address sanitizer speaks
    std::vector<rt_bake_point> points(n);
    std::vector<rt_rng> rng(n * K);
    std::vector<rt_ray> rays(n);
    std::vector<float> out(n * 27);
    for (size_t i = 0; i < rng.size(); i++) rt_rng_seed(&rng[i], (uint32_t)(1 + 7919 * i));
    rt_query_stats qs{};
    qs.struct_size = sizeof qs;

    rt_query_stats short_stats{};
    short_stats.struct_size = 8;
    expect("rays: stats.struct_size", rt_bake_rays(nullptr, points.data(), rng.data(), n, RT_BAKE_IRRADIANCE, 0, rays.data(), &short_stats), RT_ERR_INVALID_ARG, "rt_bake_rays: struct_size mismatch");
    expect("rays: mode 2", rt_bake_rays(nullptr, points.data(), rng.data(), n, 2, 0, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: mode = 2");
    expect("rays: mode -1", rt_bake_rays(nullptr, points.data(), rng.data(), n, -1, 0, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: mode = -1");
    expect("rays: flags 2", rt_bake_rays(nullptr, points.data(), rng.data(), n, RT_BAKE_SH9, RT_QUERY_REFERENCE_WALK, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: flags other than RT_QUERY_DEVICE_POINTERS");
    expect("rays: null points", rt_bake_rays(nullptr, nullptr, rng.data(), n, RT_BAKE_SH9, 0, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: null argument");
    rng[n - 1].x = 0u;
    expect("rays: engine 0 in the last record", rt_bake_rays(nullptr, points.data(), rng.data(), n, RT_BAKE_SH9, 0, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: rng[7].x = 0 is no state of the engine");
    rng[n - 1].x = 5u;
    expect("rays: null scene, n records", rt_bake_rays(nullptr, points.data(), rng.data(), n, RT_BAKE_SH9, 0, rays.data(), &qs), RT_ERR_INVALID_ARG, "rt_bake_rays: null argument");
    expect("rays: null scene, no record", rt_bake_rays(nullptr, nullptr, nullptr, 0, RT_BAKE_SH9, 0, nullptr, nullptr), RT_ERR_INVALID_ARG, "rt_bake_rays: null argument");

    rt_bake_params good{};
    good.struct_size = sizeof good; good.mode = RT_BAKE_SH9; good.samples = 8; good.streams = (int32_t)K; good.ray_depth = 4;
    rt_bake_stats bs{};
    bs.struct_size = sizeof bs;
    auto bake = [&](const rt_bake_params &p, size_t count = n, rt_bake_stats *stats = nullptr) { return rt_bake(nullptr, points.data(), count, &p, rng.data(), out.data(), stats ? stats : &bs); };
    rt_bake_params p = good;
    expect("bake: null params", rt_bake(nullptr, points.data(), n, nullptr, rng.data(), out.data(), &bs), RT_ERR_INVALID_ARG, "rt_bake: null argument (params)");
    p = good; p.struct_size = sizeof p - 4;
    expect("bake: params.struct_size", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.struct_size");
    rt_bake_stats skew{};
    skew.struct_size = sizeof skew + 8;
    expect("bake: stats.struct_size", bake(good, n, &skew), RT_ERR_INVALID_ARG, "rt_bake: stats.struct_size");
    p = good; p.mode = 2;
    expect("bake: mode 2", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.mode = 2");
    p = good; p.flags = 8u;
    expect("bake: flags 8", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.flags other than");
    p = good; p.reserved[1] = 1u;
    expect("bake: reserved", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.reserved");
    p = good; p.samples = 0;
    expect("bake: samples 0", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.samples must be at least 1");
    p = good; p.streams = 65; p.samples = 65;
    expect("bake: streams 65", bake(p), RT_ERR_LIMIT, "rt_bake: params.streams above 64");
    p = good; p.streams = -1;
    expect("bake: streams -1", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.streams");
    p = good; p.samples = 6;
    expect("bake: samples 6, streams 4", bake(p), RT_ERR_INVALID_ARG, "rt_bake: params.samples = 6 is no multiple of params.streams = 4");
    p = good; p.ray_depth = 17;
    expect("bake: ray_depth 17", bake(p), RT_ERR_LIMIT, "rt_bake: params.ray_depth above 16");
    p = good; p.streams = 64; p.samples = 64;
    expect("bake: 2^25 points of 64 streams", bake(p, (size_t)1 << 25), RT_ERR_LIMIT, "rt_bake: n_points * params.streams must stay below 2^31");
    expect("bake: null rng", rt_bake(nullptr, points.data(), n, &good, nullptr, out.data(), &bs), RT_ERR_INVALID_ARG, "rt_bake: null argument");
    rng[n * K - 1].x = 2147483647u;
    expect("bake: engine 2^31-1 in the last slot", bake(good), RT_ERR_INVALID_ARG, "rt_bake: rng[31].x = 2147483647 is no state of the engine");
    rng[n * K - 1].x = 2147483646u;
    expect("bake: null scene", bake(good), RT_ERR_INVALID_ARG, "rt_bake: null argument (scene)");
    p = good; p.streams = 0; p.ray_depth = 0; p.mode = RT_BAKE_IRRADIANCE; p.flags = RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK | RT_BAKE_LOCKSTEP;
    expect("bake: null scene, defaults and every flag", bake(p), RT_ERR_INVALID_ARG, "rt_bake: null argument (scene)");
    std::printf("bake_sanitize: %d refusals, all as expected\n", refusals);
    return 0;
}

// The argument checks of the query layer (csrc/rtamd_query.hip) under the host's address and undefined-behaviour sanitizers,
// stand-alone: every refusal of its thirteen entry points that is decided before the scene is looked at (the ones the test_*_host.py
// files list), on a null scene and exactly-sized buffers, so that no launch is ever reached -- everything rtamd_query.hip asks of
// rtamd_api.hip is a stub here that aborts, and a function it asks for that has no stub does not link.  From the repository root:
//   hipcc -x hip -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/sanitize/query_sanitize.cpp raytracing-course-hw_amd/csrc/rtamd_query.hip \
//       -o /tmp/query_asan && /tmp/query_asan
// Prints one line per refusal and "query_sanitize: N refusals, all as expected"; no GPU, no Python, nothing preloaded.
// tests/test_query_sanitize.py builds and runs it with this line wherever hipcc is.
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
    std::fprintf(stderr, "query_sanitize: %s was reached on a null scene\n", what);
    std::abort();
}
int refusals = 0;
const char *fn = ""; // the entry point under test: the front of every message
void expect(const char *what, int code, int want_code, const std::string &want_text) {
    const std::string want = std::string(fn) + ": " + want_text;
    std::printf("%-20s %-44s %d  %s\n", fn, what, code, last_error.c_str());
    if (code != want_code || last_error != want) {
        std::fprintf(stderr, "query_sanitize: %s, %s: wanted code %d and \"%s\"\n", fn, what, want_code, want.c_str());
        std::exit(1);
    }
    refusals++;
}
std::string no_state(size_t i, uint32_t x) { return "rng[" + std::to_string(i) + "].x = " + std::to_string(x) + " is no state of the engine (1 .. 2147483646)"; }
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
uint32_t query_launch_source_pack(const rt_scene *, const SourceView &, hipStream_t) { reached("query_launch_source_pack"); }
uint32_t query_launch_source_unpack(const rt_scene *, const SourceView &, hipStream_t) { reached("query_launch_source_unpack"); }
int source_check(const rt_scene *, uint32_t, int32_t, int32_t, const std::string &) { reached("source_check"); }
int source_render(rt_scene *, const SourceChunk &, hipStream_t, SourceResult &, const std::string &) { reached("source_render"); }
} // namespace rtamd

int main() {
    const int BAD = RT_ERR_INVALID_ARG, LIMIT = RT_ERR_LIMIT;
    const size_t n = 4, P = 8, K = 4;
    const uint32_t DEV = RT_QUERY_DEVICE_POINTERS, REF = RT_QUERY_REFERENCE_WALK;
    const char *WALK_FLAGS = "flags other than RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK", *SKEW = "struct_size mismatch (ABI skew)";
    // exactly as large as the calls may read or write: one byte more and the address sanitizer speaks
    std::vector<rt_ray> rays(n);
    std::vector<rt_hit> hits(n);
    std::vector<rt_surface> surfaces(n);
    std::vector<rt_scatter> scat(n);
    std::vector<rt_rng> rng(n), slots(P * K);
    std::vector<float> dirs(3 * n), rgb(3 * n), pdf(n), tmax(n), xy(2 * n), out(P * 27);
    std::vector<uint8_t> occ(n);
    std::vector<rt_bake_point> points(P);
    for (size_t i = 0; i < rng.size(); i++) rt_rng_seed(&rng[i], (uint32_t)(1 + 7919 * i));
    for (size_t i = 0; i < slots.size(); i++) rt_rng_seed(&slots[i], (uint32_t)(1 + 7919 * i));
    rt_query_stats qs{}, q_short{}, q_long{};
    qs.struct_size = sizeof qs; q_short.struct_size = sizeof qs - 8; q_long.struct_size = sizeof qs + 8;
    rt_bake_stats bs{}, b_short{}, b_query{};
    bs.struct_size = sizeof bs; b_short.struct_size = sizeof bs - 8; b_query.struct_size = sizeof qs;

    // the calls that ask check_walk_call first: the stats, then the scene
    fn = "rt_query_closest";
    expect("stats.struct_size", rt_query_closest(nullptr, rays.data(), n, 0, hits.data(), &q_short), BAD, SKEW);
    expect("null scene", rt_query_closest(nullptr, rays.data(), n, 8, hits.data(), &qs), BAD, "null argument");
    fn = "rt_query_light_pdf";
    expect("stats.struct_size", rt_query_light_pdf(nullptr, rays.data(), n, 0, pdf.data(), &q_long), BAD, SKEW);
    expect("null scene", rt_query_light_pdf(nullptr, rays.data(), n, 0, pdf.data(), nullptr), BAD, "null argument");
    fn = "rt_query_surface";
    expect("stats.struct_size", rt_query_surface(nullptr, hits.data(), n, 0, surfaces.data(), &q_short), BAD, SKEW);
    expect("null scene", rt_query_surface(nullptr, hits.data(), n, 0, surfaces.data(), &qs), BAD, "null argument");
    fn = "rt_query_environment";
    expect("stats.struct_size", rt_query_environment(nullptr, rays.data(), n, 0, rgb.data(), &q_short), BAD, SKEW);
    expect("null scene", rt_query_environment(nullptr, rays.data(), n, 0, rgb.data(), &qs), BAD, "null argument");
    fn = "rt_camera_rays";
    expect("null scene", rt_camera_rays(nullptr, 0, 0, xy.data(), n, 8, rays.data()), BAD, "null argument");
    fn = "rt_render_guides";
    expect("stats.struct_size", rt_render_guides(nullptr, 2, 2, 0, nullptr, nullptr, pdf.data(), nullptr, &q_short), BAD, SKEW);
    expect("null scene", rt_render_guides(nullptr, 2, 2, 0, nullptr, nullptr, pdf.data(), nullptr, &qs), BAD, "null argument");

    fn = "rt_query_occluded";
    expect("stats.struct_size", rt_query_occluded(nullptr, rays.data(), tmax.data(), n, 4, occ.data(), &q_short), BAD, SKEW);
    for (uint32_t flags : {4u, 8u, 0x80000000u, 3u | 16u})
        expect("flags", rt_query_occluded(nullptr, nullptr, tmax.data(), n, flags, occ.data(), &qs), BAD, WALK_FLAGS);
    expect("null rays", rt_query_occluded(nullptr, nullptr, tmax.data(), n, 0, nullptr, &qs), BAD, "null argument (rays)");
    expect("null out", rt_query_occluded(nullptr, rays.data(), tmax.data(), n, 0, nullptr, &qs), BAD, "null argument (out)");
    expect("null scene", rt_query_occluded(nullptr, rays.data(), tmax.data(), n, DEV | REF, occ.data(), &qs), BAD, "null argument (scene)");
    expect("null scene, no record", rt_query_occluded(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr), BAD, "null argument (scene)");

    // the bounce step: null arrays, stats, flags, engines, then the scene
    auto scatter = [&](uint32_t flags, rt_query_stats *st, int drop = -1) {
        return rt_query_scatter(nullptr, drop == 0 ? nullptr : rays.data(), drop == 1 ? nullptr : hits.data(), drop == 2 ? nullptr : surfaces.data(),
                                drop == 3 ? nullptr : rng.data(), n, flags, drop == 4 ? nullptr : scat.data(), st);
    };
    auto bsdf = [&](uint32_t flags, rt_query_stats *st, int drop = -1) {
        return rt_query_bsdf(nullptr, drop == 0 ? nullptr : rays.data(), drop == 1 ? nullptr : hits.data(), drop == 2 ? nullptr : surfaces.data(),
                             drop == 3 ? nullptr : dirs.data(), n, flags, drop == 4 ? nullptr : rgb.data(), drop == 5 ? nullptr : pdf.data(), st);
    };
    auto trace = [&](uint32_t flags, rt_query_stats *st, int drop = -1) {
        return rt_trace_paths(nullptr, drop == 0 ? nullptr : rays.data(), drop == 1 ? nullptr : rng.data(), n, 17, flags, drop == 2 ? nullptr : rgb.data(), st);
    };
    auto bounce = [&](const char *name, int arrays, bool engines, auto call) {
        fn = name;
        for (int drop = 0; drop < arrays; drop++) expect("null array", call(0, &q_short, drop), BAD, "null argument");
        expect("stats.struct_size", call(4, &q_short, -1), BAD, SKEW);
        expect("stats.struct_size", call(0, &q_long, -1), BAD, SKEW);
        for (uint32_t flags : {4u, 8u, 0x80000000u, 3u | 16u}) expect("flags", call(flags, &qs, -1), BAD, WALK_FLAGS);
        if (engines)
            for (uint32_t x : {0u, 2147483647u, 2147483648u, 4294967295u})
                for (size_t at : {(size_t)0, n - 1}) {
                    const uint32_t keep = rng[at].x;
                    rng[at].x = x;
                    expect("engine state", call(REF, &qs, -1), BAD, no_state(at, x));
                    expect("engine state, device array", call(DEV, &qs, -1), BAD, "null argument");
                    rng[at].x = keep;
                }
        rng[0].x = 1u; rng[n - 1].x = 2147483646u;
        expect("null scene", call(DEV | REF, &qs, -1), BAD, "null argument");
        expect("null scene, no stats", call(0, nullptr, -1), BAD, "null argument");
    };
    bounce("rt_query_scatter", 5, true, scatter);
    bounce("rt_query_bsdf", 6, false, bsdf);
    bounce("rt_trace_paths", 3, true, trace);

    fn = "rt_bake_rays";
    auto bake_rays = [&](int32_t mode, uint32_t flags, rt_query_stats *st, int drop = -1) {
        return rt_bake_rays(nullptr, drop == 0 ? nullptr : points.data(), drop == 1 ? nullptr : rng.data(), n, mode, flags, drop == 2 ? nullptr : rays.data(), st);
    };
    expect("stats.struct_size", bake_rays(2, 0, &q_short), BAD, SKEW);
    for (int32_t mode : {2, -1, 27}) expect("mode", bake_rays(mode, 2, &qs), BAD, "mode = " + std::to_string(mode) + " is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9");
    for (uint32_t flags : {2u, 4u, 8u, 0x80000000u, 1u | 4u}) expect("flags", bake_rays(RT_BAKE_SH9, flags, &qs, 0), BAD, "flags other than RT_QUERY_DEVICE_POINTERS");
    for (int drop = 0; drop < 3; drop++) expect("null array", bake_rays(RT_BAKE_SH9, 0, &qs, drop), BAD, "null argument");
    for (uint32_t x : {0u, 2147483647u, 4294967295u})
        for (size_t at : {(size_t)0, n - 1}) {
            const uint32_t keep = rng[at].x;
            rng[at].x = x;
            expect("engine state", bake_rays(RT_BAKE_IRRADIANCE, 0, &qs), BAD, no_state(at, x));
            expect("engine state, device array", bake_rays(RT_BAKE_IRRADIANCE, DEV, &qs), BAD, "null argument");
            rng[at].x = keep;
        }
    expect("null scene", bake_rays(RT_BAKE_SH9, 0, &qs), BAD, "null argument");
    expect("null scene, no record", rt_bake_rays(nullptr, nullptr, nullptr, 0, RT_BAKE_SH9, 0, nullptr, nullptr), BAD, "null argument");

    // the two bakers share their params block; rt_render_bake adds two refusals before the null arrays
    rt_bake_params good{};
    good.struct_size = sizeof good; good.mode = RT_BAKE_IRRADIANCE; good.samples = 8; good.streams = (int32_t)K; good.ray_depth = 4;
    auto baker = [&](const char *name, auto entry, uint32_t bad_flags, const char *flag_names, bool render) {
        fn = name;
        auto call = [&](const rt_bake_params &p, size_t count = 8, rt_bake_stats *st = nullptr, int drop = -1) {
            return entry(nullptr, drop == 0 ? nullptr : points.data(), count, &p, drop == 1 ? nullptr : slots.data(), drop == 2 ? nullptr : out.data(), st ? st : &bs);
        };
        rt_bake_params p = good;
        expect("null params", entry(nullptr, points.data(), P, nullptr, slots.data(), out.data(), &bs), BAD, "null argument (params)");
        for (uint32_t size : {0u, 28u, 36u}) { p = good; p.struct_size = size; expect("params.struct_size", call(p, P, &b_short), BAD, std::string("params.") + SKEW); }
        p = good; p.mode = 2;
        expect("stats.struct_size", call(p, P, &b_short), BAD, std::string("stats.") + SKEW);
        expect("stats.struct_size", call(good, P, &b_query), BAD, std::string("stats.") + SKEW);
        for (int32_t mode : {2, -1}) { p = good; p.mode = mode; p.flags = 0x80u; expect("mode", call(p), BAD, "params.mode = " + std::to_string(mode) + " is neither RT_BAKE_IRRADIANCE nor RT_BAKE_SH9"); }
        for (uint32_t flags : {bad_flags, 0x80000000u, bad_flags | 1u}) { p = good; p.flags = flags; p.reserved[0] = 1u; expect("flags", call(p), BAD, std::string("params.flags other than ") + flag_names); }
        for (int word : {0, 1}) { p = good; p.reserved[word] = 1u; p.streams = -1; expect("reserved", call(p), BAD, "params.reserved must be zero"); }
        p = good; p.streams = -1; p.samples = 0;
        expect("streams -1", call(p), BAD, "params.streams must not be negative");
        p = good; p.streams = 65; p.samples = 65;
        expect("streams 65", call(p), LIMIT, "params.streams above 64");
        for (int32_t samples : {0, -8}) { p = good; p.samples = samples; expect("samples", call(p), BAD, "params.samples must be at least 1"); }
        for (auto sk : {std::pair<int32_t, int32_t>{6, 4}, {63, 64}, {1, 2}}) {
            p = good; p.samples = sk.first; p.streams = sk.second; p.ray_depth = 17;
            expect("samples no multiple", call(p), BAD, "params.samples = " + std::to_string(sk.first) + " is no multiple of params.streams = " + std::to_string(sk.second));
        }
        for (int32_t depth : {17, 1000}) { p = good; p.ray_depth = depth; expect("ray_depth", call(p, (size_t)1 << 31), LIMIT, "params.ray_depth above 16"); }
        p = good; p.streams = 64; p.samples = 64;
        expect("2^25 points of 64 streams", call(p, (size_t)1 << 25), LIMIT, "n_points * params.streams must stay below 2^31");
        p = good; p.streams = 1;
        expect("2^31 points", call(p, (size_t)1 << 31, nullptr, 0), LIMIT, "n_points * params.streams must stay below 2^31");
        if (render) {
            p = good; p.streams = 1; p.samples = 1 << 25; p.mode = RT_BAKE_SH9;
            expect("2^25 samples per stream", call(p), LIMIT, "params.samples / params.streams must stay below 2^25 (the path record's sample index)");
            p = good; p.mode = RT_BAKE_SH9;
            expect("SH9", call(p, P, nullptr, 0), RT_ERR_UNSUPPORTED, "RT_BAKE_SH9 does not fit the persistent kernel's path record (27 accumulators and the first direction): rt_bake serves it");
        }
        for (int drop = 0; drop < 3; drop++) expect("null array", call(good, P, nullptr, drop), BAD, "null argument");
        for (uint32_t x : {0u, 2147483647u})
            for (size_t at : {(size_t)0, P * K - 1}) {
                const uint32_t keep = slots[at].x;
                slots[at].x = x;
                expect("engine state", call(good), BAD, no_state(at, x));
                p = good; p.flags = DEV;
                expect("engine state, device array", call(p), BAD, "null argument (scene)");
                slots[at].x = keep;
            }
        slots[P * K - 1].x = 2147483646u;
        expect("null scene", call(good), BAD, "null argument (scene)");
        p = good; p.streams = 0; p.ray_depth = 0; p.flags = render ? DEV : DEV | REF | RT_BAKE_LOCKSTEP;
        expect("null scene, defaults and every flag", call(p), BAD, "null argument (scene)");
        p = good; p.ray_depth = 16; p.streams = 1; p.samples = 1;
        expect("null scene, depth 16", call(p), BAD, "null argument (scene)");
    };
    baker("rt_bake", rt_bake, 8u, "RT_QUERY_DEVICE_POINTERS | RT_QUERY_REFERENCE_WALK | RT_BAKE_LOCKSTEP", false);
    baker("rt_render_bake", rt_render_bake, 2u, "RT_QUERY_DEVICE_POINTERS", true);
    good.mode = RT_BAKE_SH9;
    fn = "rt_bake";
    expect("null scene, SH9", rt_bake(nullptr, points.data(), P, &good, slots.data(), out.data(), &bs), BAD, "null argument (scene)");

    fn = "rt_render_paths";
    auto paths = [&](int32_t depth, uint32_t flags, rt_query_stats *st, int drop = -1) {
        return rt_render_paths(nullptr, drop == 0 ? nullptr : rays.data(), drop == 1 ? nullptr : rng.data(), n, depth, flags, drop == 2 ? nullptr : rgb.data(), st);
    };
    for (int drop = 0; drop < 3; drop++) expect("null array", paths(0, 0, &q_short, drop), BAD, "null argument");
    expect("stats.struct_size", paths(0, 2, &q_short), BAD, SKEW);
    expect("stats.struct_size", paths(0, 0, &q_long), BAD, SKEW);
    for (uint32_t flags : {2u, 4u, 8u, 0x80000000u, 1u | 2u}) expect("flags", paths(17, flags, &qs), BAD, "flags other than RT_QUERY_DEVICE_POINTERS");
    for (uint32_t x : {0u, 2147483647u, 4294967295u})
        for (size_t at : {(size_t)0, n - 1}) {
            const uint32_t keep = rng[at].x;
            rng[at].x = x;
            expect("engine state", paths(17, 0, &qs), BAD, no_state(at, x));
            expect("engine state, device array", paths(0, DEV, &qs), BAD, "null argument");
            rng[at].x = keep;
        }
    for (int32_t depth : {17, 1000}) expect("ray_depth", paths(depth, 0, &qs), LIMIT, "ray_depth above 16");
    expect("null scene", paths(16, DEV, &qs), BAD, "null argument");
    expect("null scene, no record", rt_render_paths(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr), BAD, "null argument");

    std::printf("query_sanitize: %d refusals, all as expected\n", refusals);
    return 0;
}

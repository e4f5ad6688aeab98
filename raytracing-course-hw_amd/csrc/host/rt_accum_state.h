// struct rt_accum, struct rt_multi_accum and the header of the checkpoint, shared by the translation units that keep or read resumable
// state: rtamd_api.hip (rt_accum_*: one frame or one shard on one device), rtamd_multi.hip (rt_multi_accum_*: one sharded rt_accum
// per device and the checkpoint of the whole frame, which is the unsharded rt_accum's blob byte for byte) and rtamd_noise.hip
// (rt_noise_* / rt_multi_noise_*: the noise monitors, which only read the state between slices) and rtamd_denoise.hip (rt_accum_denoise:
// the preview filter, which only reads it too and keeps the frame's guide planes here).
#pragma once
#include <cstring>
#include <string>
#include <vector>
#include "rt_scene.h"

#define ACCUM_MAGIC 0x43415452u   // "RTAC" read as a little-endian word
#define ACCUM_VERSION 1u
#define ACCUM_HEADER_BYTES 128u
#define ACCUM_SLOT_BYTES 24u
enum { AH_MAGIC, AH_VERSION, AH_HEADER_BYTES, AH_SLOT_BYTES, AH_WIDTH, AH_HEIGHT, AH_INTEGRATOR, AH_RAY_DEPTH, AH_TILE_W, AH_TILE_H,
       AH_SHARD_INDEX, AH_SHARD_COUNT, AH_PIXSLOTS, AH_SAMPLES, AH_TRIANGLES, AH_LIGHTS, AH_LIGHT_HASH, AH_WORDS };
static const char *const accum_field_names[AH_WORDS] = {"magic", "format version", "header size", "bytes per pixel slot", "width", "height", "integrator",
    "ray depth", "tile width", "tile height", "shard index", "shard count", "pixel slots", "samples", "triangle count of the scene", "light count of the scene",
    "light order of the scene (hash)"};

struct rt_accum {
    rt_scene *scene = nullptr;
    rt_render_params params{};      // as given to rt_accum_create; samples is set per slice
    rtamd::RenderView view{};       // the frame's geometry (resolve_tiles)
    uint32_t n_pixslots = 0;
    uint32_t *d_state = nullptr;
    int32_t samples = 0;            // per pixel so far
    int32_t sample_limit = 0;       // the path records' sample index field (choose_pipeline)
    std::string broken;             // first error of a slice that failed under way: the state is half advanced
    uint64_t loads = 0;             // how often rt_accum_load has replaced the state (a noise monitor's batches end there)
    float *d_guides = nullptr;      // rt_accum_denoise: albedo, normal, depth, emission of the frame (10 floats per pixel), made by its first call
    ~rt_accum() { if (d_state) (void)hipFree(d_state); if (d_guides) (void)hipFree(d_guides); }
};

// One sharded rt_accum per device entry of an rt_multi (shard i of N on that entry's stream; none for an entry that gets no tile).
// With one entry the rt_accum IS the unsharded one.
struct rt_multi;
struct rt_multi_accum {
    rt_multi *multi = nullptr;
    rt_render_params params{};       // of the unsharded frame, as given
    int tile = 32;
    rtamd::RenderView frame{};       // geometry of the unsharded frame: 8x8 tiles, shard 0 of 1
    uint32_t frame_slots = 0;        // ceil(W/8) * ceil(H/8) * 64
    std::vector<rt_accum *> shard;   // per device entry; null = an empty shard
    std::vector<size_t> elems;       // floats (or bytes) of each shard's compact picture
    int32_t samples = 0, sample_limit = 0;
    std::string broken;              // first error of a call that failed under way on some device
    uint64_t loads = 0;              // how often rt_multi_accum_load has replaced the shards' states
    ~rt_multi_accum() { for (rt_accum *a : shard) if (a) rt_accum_destroy(a); }
};

// The 128-byte header of the checkpoint of a frame (or shard) of geometry `R` with `n_pixslots` pixel slots after `samples` samples.
static inline void accum_header(const rt_scene *scene, int integrator, const rtamd::RenderView &R, uint32_t n_pixslots, int32_t samples, uint32_t *h) {
    memset(h, 0, ACCUM_HEADER_BYTES);
    h[AH_MAGIC] = ACCUM_MAGIC; h[AH_VERSION] = ACCUM_VERSION; h[AH_HEADER_BYTES] = ACCUM_HEADER_BYTES; h[AH_SLOT_BYTES] = ACCUM_SLOT_BYTES;
    h[AH_WIDTH] = (uint32_t)R.width; h[AH_HEIGHT] = (uint32_t)R.height; h[AH_INTEGRATOR] = (uint32_t)integrator; h[AH_RAY_DEPTH] = (uint32_t)R.ray_depth;
    h[AH_TILE_W] = (uint32_t)R.tile_w; h[AH_TILE_H] = (uint32_t)R.tile_h; h[AH_SHARD_INDEX] = (uint32_t)R.shard_index; h[AH_SHARD_COUNT] = (uint32_t)R.shard_count;
    h[AH_PIXSLOTS] = n_pixslots; h[AH_SAMPLES] = (uint32_t)samples;
    h[AH_TRIANGLES] = scene->info.n_triangles; h[AH_LIGHTS] = scene->info.n_lights;
    uint32_t hash = 2166136261u; // FNV-1a over the bytes of the light order, least significant first
    for (uint32_t v : scene->light_order) for (int b = 0; b < 4; b++) { hash ^= (v >> (8 * b)) & 255u; hash *= 16777619u; }
    h[AH_LIGHT_HASH] = hash;
}
static inline void accum_header(const rt_accum *a, uint32_t *h) { accum_header(a->scene, a->params.integrator, a->view, a->n_pixslots, a->samples, h); }

// What a loader refuses in a blob of `size` bytes, before any state is replaced: `want` is the header of the frame that loads it, `state`
// the bytes of state behind the header.  Returns the blob's sample count, or the rt_status with `who` in front of the message.
static inline int accum_check_blob(const uint32_t *want, const void *blob, size_t size, int32_t sample_limit, size_t state, const std::string &who) {
    if (size < ACCUM_HEADER_BYTES) return rtamd::fail(RT_ERR_INVALID_ARG, who + "truncated blob (shorter than its header)");
    uint32_t got[ACCUM_HEADER_BYTES / 4];
    memcpy(got, blob, ACCUM_HEADER_BYTES);
    for (int f = 0; f < AH_WORDS; f++)
        if (f != AH_SAMPLES && got[f] != want[f])
            return rtamd::fail(RT_ERR_INVALID_ARG, who + "the blob does not belong to this frame: " + accum_field_names[f] + " is " + std::to_string(got[f]) +
                                                       ", expected " + std::to_string(want[f]));
    if (got[AH_SAMPLES] >= (uint32_t)sample_limit) return rtamd::fail(RT_ERR_INVALID_ARG, who + "samples beyond the path records' sample index");
    if (size < ACCUM_HEADER_BYTES + state) return rtamd::fail(RT_ERR_INVALID_ARG, who + "truncated blob (" + std::to_string(size) + " bytes, " + std::to_string(ACCUM_HEADER_BYTES + state) + " expected)");
    return (int)got[AH_SAMPLES];
}

// fn(i), an rt_status, on the calling thread for every device entry i of n that has a device (device_of(i) >= 0), with that device
// current: entries 1 .. n-1 first and entry 0 last, so that device 0 is the current device again afterwards.  Stops at the first
// status that is not RT_OK and returns it.  The parallel sibling is rtamd_multi.hip's fan_out.
template <class DeviceOf, class Fn> static inline int each_device(size_t n, DeviceOf device_of, Fn fn) {
    for (size_t k = 1; k <= n; k++) {
        const size_t i = k % n;
        if (device_of(i) < 0) continue;
        HIP_CHECK(hipSetDevice(device_of(i)));
        if (const int rc = fn(i)) return rc;
    }
    return RT_OK;
}

namespace rtamd {
// What rt_accum_render refuses before it launches anything (a broken state, n_samples, the sample-index limit, a pipeline without
// resumable state); RT_OK = the slice would be launched.  Host only; `who` prefixes the message.
int accum_check_slice(const rt_accum *a, int32_t n_samples, const std::string &who);
// What rt_noise_estimate would refuse of monitor `n`, and that it watches `a` (rtamd_noise.hip); RT_OK = an estimate can be taken.  Host only.
int noise_estimate_ready(const rt_noise *n, const rt_accum *a, const std::string &who);
} // namespace rtamd

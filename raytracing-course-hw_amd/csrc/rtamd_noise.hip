// Noise monitors of resumable renders (include/rtamd.h: rt_noise_* on an rt_accum, rt_multi_noise_* on an rt_multi_accum): per-pixel
// standard error of the picture's luminance by batch means over the slices (device/rt_noise.h), and the figures of the frame summed on
// the host in double, in the order of the frame's 8x8 sub-tiles, row-major -- so a sharded frame gives the unsharded frame's figures bit
// for bit.  Nothing here writes an rt_accum: the monitors read its state between slices, on its device and its stream.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "host/rt_accum_state.h"
#include "device/rt_noise.h"

using namespace rtamd;

struct rt_noise {
    rt_accum *accum = nullptr;
    float *d_stats = nullptr;        // y0, yp, m2: n_pixslots floats each
    NoiseTile *d_tiles = nullptr;    // n_pixslots / 64
    int32_t batches = 0, observed = 0; // B and N of device/rt_noise.h
    int32_t samples_seen = 0;        // rt_accum_samples at the last update / snapshot
    uint64_t loads_seen = 0;         // rt_accum::loads at the last snapshot
    ~rt_noise() {
        if (d_stats) (void)hipFree(d_stats);
        if (d_tiles) (void)hipFree(d_tiles);
    }
};

struct rt_multi_noise {
    rt_multi_accum *accum = nullptr;
    std::vector<rt_noise *> shard;   // one monitor per non-empty shard of the rt_multi_accum, null for an empty one
    uint64_t loads_seen = 0;         // rt_multi_accum::loads at the last snapshot
    ~rt_multi_noise() { for (rt_noise *n : shard) if (n) rt_noise_destroy(n); }
};

namespace {

unsigned noise_blocks(uint32_t n_pixslots) { return (n_pixslots + 255u) / 256u; }

NoiseView noise_view(const rt_noise *n) {
    NoiseView V{};
    const size_t slots = n->accum->n_pixslots;
    V.accum = n->accum->d_state;
    V.y0 = n->d_stats; V.yp = n->d_stats + slots; V.m2 = n->d_stats + 2 * slots;
    V.tiles = n->d_tiles;
    return V;
}
RenderView noise_frame(const rt_noise *n) {
    RenderView R = n->accum->view;
    R.n_pixslots = n->accum->n_pixslots;
    return R;
}

// The refusal every call makes of a monitor whose accumulator is broken.
int noise_usable(const rt_accum *a, const std::string &who) {
    if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "the accumulator is broken: an earlier slice failed and left the state half advanced (" + a->broken + ")");
    return RT_OK;
}

// The launches below run on the accumulator's stream; its device is the current one (the entry points and each_device see to that).
// create / reset: the sums as they are, no batch yet
int noise_snapshot(rt_noise *n, const std::string &who) {
    rt_accum *a = n->accum;
    if (const int rc = noise_usable(a, who)) return rc;
    hipStream_t stream = (hipStream_t)a->params.stream;
    if (a->n_pixslots) {
        hipLaunchKernelGGL(dev::noise_snapshot_kernel, dim3(noise_blocks(a->n_pixslots)), dim3(256), 0, stream, noise_frame(n), noise_view(n));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    n->batches = 0; n->observed = 0;
    n->samples_seen = a->samples; n->loads_seen = a->loads;
    return RT_OK;
}

// what rt_noise_update refuses, before anything is launched: the statistics stay as they were
int noise_update_check(const rt_noise *n, const std::string &who) {
    const rt_accum *a = n->accum;
    if (const int rc = noise_usable(a, who)) return rc;
    if (a->loads != n->loads_seen) return fail(RT_ERR_INVALID_ARG, who + "rt_accum_load has replaced the state since the monitor's last snapshot: its batches do not continue, call rt_noise_reset");
    if (a->samples <= n->samples_seen) return fail(RT_ERR_INVALID_ARG, who + "no samples since the last update (a batch needs at least one)");
    return RT_OK;
}

void noise_update(rt_noise *n) {
    rt_accum *a = n->accum;
    const int32_t batch = a->samples - n->samples_seen;
    hipStream_t stream = (hipStream_t)a->params.stream;
    if (a->n_pixslots) {
        NoiseView V = noise_view(n);
        V.n = (float)batch; V.N = (float)n->observed; V.N1 = (float)(n->observed + batch); V.first = n->observed == 0;
        hipLaunchKernelGGL(dev::noise_update_kernel, dim3(noise_blocks(a->n_pixslots)), dim3(256), 0, stream, noise_frame(n), V);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    n->batches += 1; n->observed += batch; n->samples_seen = a->samples;
}

int noise_estimate_check(const rt_noise *n, const std::string &who) {
    const rt_accum *a = n->accum;
    if (const int rc = noise_usable(a, who)) return rc;
    if (a->loads != n->loads_seen) return fail(RT_ERR_INVALID_ARG, who + "rt_accum_load has replaced the state since the monitor's last snapshot: call rt_noise_reset");
    if (n->batches < 2) return fail(RT_ERR_INVALID_ARG, who + std::to_string(n->batches) + " batches so far: the scatter of batch means needs at least 2");
    return RT_OK;
}

// Elements of the map: one float per pixel in the layout of rt_accum_resolve.
size_t noise_map_elems(const rt_noise *n) {
    const RenderView &R = n->accum->view;
    return R.shard_count > 1 ? (size_t)n->accum->n_pixslots : (size_t)R.width * R.height;
}

// Launches the estimate on the monitor's stream: the map to `d_se` (device memory, nullable), the sub-tile entries to `tiles`
// (host, n_pixslots / 64).  Returns with the copies queued; the caller synchronises the stream.
void noise_estimate_launch(rt_noise *n, float *d_se, NoiseTile *tiles) {
    rt_accum *a = n->accum;
    hipStream_t stream = (hipStream_t)a->params.stream;
    if (!a->n_pixslots) return;
    NoiseView V = noise_view(n);
    V.dof = (float)(n->batches - 1); V.d = (float)a->samples;
    V.out_se = d_se;
    hipLaunchKernelGGL(dev::noise_estimate_kernel, dim3(noise_blocks(a->n_pixslots)), dim3(256), 0, stream, noise_frame(n), V);
    HIP_CHECK(hipGetLastError());
    if (tiles) HIP_CHECK(hipMemcpyAsync(tiles, n->d_tiles, (size_t)(a->n_pixslots / 64u) * sizeof(NoiseTile), hipMemcpyDeviceToHost, stream));
}

// Sub-tile `w` of the shard -> its place among the frame's 8x8 sub-tiles (ceil(W/8) per row); false: wholly outside the image.
bool noise_frame_subtile(const RenderView &R, uint32_t w, size_t &place) {
    const uint32_t sub_x = (uint32_t)R.tile_w >> 3, sub_per_tile = sub_x * ((uint32_t)R.tile_h >> 3);
    const uint32_t st = w / sub_per_tile, sub = w % sub_per_tile;
    const uint32_t gt = R.shard_count > 1 ? (uint32_t)R.shard_index + st * (uint32_t)R.shard_count : st;
    const uint32_t gx = (gt % (uint32_t)R.tiles_x) * sub_x + sub % sub_x, gy = (gt / (uint32_t)R.tiles_x) * ((uint32_t)R.tile_h >> 3) + sub / sub_x;
    const uint32_t sub_w = ((uint32_t)R.width + 7u) >> 3, sub_h = ((uint32_t)R.height + 7u) >> 3;
    place = (size_t)gy * sub_w + gx;
    return gx < sub_w && gy < sub_h;
}
void noise_place_tiles(const RenderView &R, const std::vector<NoiseTile> &tiles, std::vector<NoiseTile> &frame) {
    for (size_t w = 0; w < tiles.size(); w++) {
        size_t place;
        if (noise_frame_subtile(R, (uint32_t)w, place)) frame[place] = tiles[w];
    }
}

// The figures of a frame (or of a shard: the sub-tiles of the other shards are absent, i.e. zero) from its sub-tile entries in frame order.
void noise_summarise(const std::vector<NoiseTile> &frame, const rt_noise *n, rt_noise_summary *s) {
    uint64_t pixels = 0, nonfinite = 0;
    double se2 = 0, lum = 0, worst = 0;
    for (const NoiseTile &t : frame) {
        nonfinite += t.nonfinite;
        if (!t.pixels) continue;
        pixels += t.pixels;
        se2 += (double)t.sum_se2;
        lum += (double)t.sum_luminance;
        const double mean = (double)t.sum_se2 / (double)t.pixels;
        if (mean > worst) worst = mean;
    }
    s->batches = n->batches; s->samples_observed = n->observed; s->samples_total = n->accum->samples;
    s->pixels = pixels; s->nonfinite_pixels = nonfinite;
    s->mean_luminance = pixels ? lum / (double)pixels : 0.0;
    s->rms_error = pixels ? std::sqrt(se2 / (double)pixels) : 0.0;
    s->noise = s->mean_luminance != 0.0 ? s->rms_error / s->mean_luminance : 0.0;
    s->worst_tile_noise = s->mean_luminance != 0.0 ? std::sqrt(worst) / s->mean_luminance : 0.0;
}

size_t noise_frame_subtiles(const RenderView &R) { return (size_t)(((uint32_t)R.width + 7u) >> 3) * (((uint32_t)R.height + 7u) >> 3); }

} // namespace

int rtamd::noise_estimate_ready(const rt_noise *n, const rt_accum *a, const std::string &who) {
    if (n->accum != a) return fail(RT_ERR_INVALID_ARG, who + "the monitor watches another accumulator");
    return noise_estimate_check(n, who);
}

extern "C" {

int rt_noise_create(rt_accum *a, rt_noise **out) {
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, "rt_noise_create: null argument");
    *out = nullptr;
    return guarded("rt_noise_create: ", [&]() -> int {
        std::unique_ptr<rt_noise> n(new rt_noise);
        n->accum = a;
        HIP_CHECK(hipSetDevice(a->scene->device));
        const size_t slots = a->n_pixslots ? a->n_pixslots : 64u;
        HIP_CHECK(hipMalloc((void **)&n->d_stats, 3 * slots * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&n->d_tiles, (slots / 64u) * sizeof(NoiseTile)));
        HIP_CHECK(hipMemsetAsync(n->d_stats, 0, 3 * slots * sizeof(float), (hipStream_t)a->params.stream)); // padding slots are never written again
        if (const int rc = noise_snapshot(n.get(), "rt_noise_create: ")) return rc;
        *out = n.release();
        return RT_OK;
    });
}

void rt_noise_destroy(rt_noise *n) {
    if (n) (void)hipSetDevice(n->accum->scene->device);
    delete n;
}

int rt_noise_reset(rt_noise *n) {
    if (!n) return fail(RT_ERR_INVALID_ARG, "rt_noise_reset: null argument");
    return guarded("rt_noise_reset: ", [&]() -> int {
        HIP_CHECK(hipSetDevice(n->accum->scene->device));
        return noise_snapshot(n, "rt_noise_reset: ");
    });
}

int rt_noise_batches(const rt_noise *n) {
    if (!n) return fail(RT_ERR_INVALID_ARG, "rt_noise_batches: null argument");
    return n->batches;
}

int rt_noise_update(rt_noise *n) {
    if (!n) return fail(RT_ERR_INVALID_ARG, "rt_noise_update: null argument");
    return guarded("rt_noise_update: ", [&]() -> int {
        if (const int rc = noise_update_check(n, "rt_noise_update: ")) return rc;
        HIP_CHECK(hipSetDevice(n->accum->scene->device));
        noise_update(n);
        return RT_OK;
    });
}

int rt_noise_estimate(rt_noise *n, uint32_t flags, float *out_se, rt_noise_summary *summary) {
    if (summary && summary->struct_size != sizeof(rt_noise_summary)) return fail(RT_ERR_INVALID_ARG, "rt_noise_estimate: struct_size mismatch (ABI skew)");
    if (!n) return fail(RT_ERR_INVALID_ARG, "rt_noise_estimate: null argument");
    if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, "rt_noise_estimate: flags other than RT_FLAG_OUT_DEVICE");
    return guarded("rt_noise_estimate: ", [&]() -> int {
        if (const int rc = noise_estimate_check(n, "rt_noise_estimate: ")) return rc;
        if (!out_se && !summary) return RT_OK;
        rt_accum *a = n->accum;
        HIP_CHECK(hipSetDevice(a->scene->device));
        hipStream_t stream = (hipStream_t)a->params.stream;
        StagedOut se(out_se, flags, noise_map_elems(n), sizeof(float));
        std::vector<NoiseTile> tiles(a->n_pixslots / 64u);
        noise_estimate_launch(n, (float *)se.dev, tiles.data());
        se.copy_back(stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        if (summary) {
            std::vector<NoiseTile> frame(noise_frame_subtiles(a->view), NoiseTile{0.f, 0.f, 0u, 0u});
            noise_place_tiles(a->view, tiles, frame);
            noise_summarise(frame, n, summary);
        }
        return RT_OK;
    });
}

// ---- the same on an rt_multi_accum: one rt_noise per non-empty shard, each on that shard's device and stream ----------------------------

#define MN_ENTER(name)                                                                                                                       \
    if (!n) return fail(RT_ERR_INVALID_ARG, name ": null argument");                                                                          \
    if (!n->accum->broken.empty()) return fail(RT_ERR_INVALID_ARG, name ": the accumulator is broken: an earlier call failed under way and left the state half advanced (" + n->accum->broken + ")")

// the HIP device of shard i's monitor, -1 for an empty shard (each_device)
static int noise_device(const rt_multi_noise *n, size_t i) { return n->shard[i] ? n->shard[i]->accum->scene->device : -1; }

int rt_multi_noise_create(rt_multi_accum *a, rt_multi_noise **out) {
    if (!a || !out) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_create: null argument");
    *out = nullptr;
    return guarded("rt_multi_noise_create: ", [&]() -> int {
        if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_create: the accumulator is broken: an earlier call failed under way and left the state half advanced (" + a->broken + ")");
        std::unique_ptr<rt_multi_noise> n(new rt_multi_noise);
        n->accum = a;
        n->shard.assign(a->shard.size(), nullptr);
        for (size_t i = 0; i < a->shard.size(); i++)
            if (a->shard[i])
                if (const int rc = rt_noise_create(a->shard[i], &n->shard[i])) return fail(rc, std::string("rt_multi_noise_create: shard ") + std::to_string(i) + ": " + rt_last_error());
        n->loads_seen = a->loads;
        (void)hipSetDevice(a->shard[0]->scene->device);
        *out = n.release();
        return RT_OK;
    });
}

void rt_multi_noise_destroy(rt_multi_noise *n) { delete n; }

int rt_multi_noise_reset(rt_multi_noise *n) {
    return guarded("rt_multi_noise_reset: ", [&]() -> int {
        MN_ENTER("rt_multi_noise_reset");
        const int rc = each_device(n->shard.size(), [&](size_t i) { return noise_device(n, i); }, [&](size_t i) {
            const std::string who = "rt_multi_noise_reset: shard " + std::to_string(i) + ": ";
            return guarded(who, [&]() -> int { return noise_snapshot(n->shard[i], who); });
        });
        if (rc == RT_OK) n->loads_seen = n->accum->loads;
        return rc;
    });
}

int rt_multi_noise_batches(const rt_multi_noise *n) {
    if (!n) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_batches: null argument");
    return n->shard[0]->batches; // the first entry always has a tile; the shards advance together
}

int rt_multi_noise_update(rt_multi_noise *n) {
    return guarded("rt_multi_noise_update: ", [&]() -> int {
        MN_ENTER("rt_multi_noise_update");
        if (n->accum->loads != n->loads_seen) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_update: rt_multi_accum_load has replaced the state since the monitor's last snapshot: its batches do not continue, call rt_multi_noise_reset");
        for (rt_noise *s : n->shard) // every refusal before any device launches
            if (s) if (const int rc = noise_update_check(s, "rt_multi_noise_update: ")) return rc;
        return each_device(n->shard.size(), [&](size_t i) { return noise_device(n, i); }, [&](size_t i) {
            return guarded("rt_multi_noise_update: shard " + std::to_string(i) + ": ", [&]() -> int { noise_update(n->shard[i]); return RT_OK; });
        });
    });
}

int rt_multi_noise_estimate(rt_multi_noise *n, uint32_t flags, float *out_se, rt_noise_summary *summary) {
    if (summary && summary->struct_size != sizeof(rt_noise_summary)) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_estimate: struct_size mismatch (ABI skew)");
    return guarded("rt_multi_noise_estimate: ", [&]() -> int {
        MN_ENTER("rt_multi_noise_estimate");
        if (flags) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_estimate: flags must be 0 (the outputs are host memory)");
        if (n->accum->loads != n->loads_seen) return fail(RT_ERR_INVALID_ARG, "rt_multi_noise_estimate: rt_multi_accum_load has replaced the state since the monitor's last snapshot: call rt_multi_noise_reset");
        for (rt_noise *s : n->shard)
            if (s) if (const int rc = noise_estimate_check(s, "rt_multi_noise_estimate: ")) return rc;
        if (!out_se && !summary) return RT_OK;
        const size_t N = n->shard.size();
        const int width = n->accum->params.width, height = n->accum->params.height;
        const auto device_of = [&](size_t i) { return noise_device(n, i); };
        std::vector<std::vector<NoiseTile>> tiles(N);
        std::vector<std::vector<float>> se(N);
        std::vector<StagedOut> staged; // one per shard, freed on every way out
        staged.reserve(N);
        each_device(N, device_of, [&](size_t i) { // every device works on its own stream; the waits come after the last launch
            rt_noise *s = n->shard[i];
            if (out_se) se[i].resize(noise_map_elems(s));
            staged.emplace_back(se[i].data(), 0u, se[i].size(), sizeof(float));
            tiles[i].resize(s->accum->n_pixslots / 64u);
            noise_estimate_launch(s, (float *)staged.back().dev, tiles[i].data());
            staged.back().copy_back((hipStream_t)s->accum->params.stream);
            return RT_OK;
        });
        each_device(N, device_of, [&](size_t i) { HIP_CHECK(hipStreamSynchronize((hipStream_t)n->shard[i]->accum->params.stream)); return RT_OK; });
        if (out_se) { // the shards' compact maps -> the frame, on the host
            for (size_t i = 0; i < N; i++) {
                if (!n->shard[i]) continue;
                const RenderView &R = n->shard[i]->accum->view;
                if (R.shard_count <= 1) { memcpy(out_se, se[i].data(), se[i].size() * sizeof(float)); continue; }
                for (uint32_t st = 0; st < R.n_shard_tiles; st++) {
                    int x0, y0, w, h;
                    shard_tile_rect(R, st, x0, y0, w, h);
                    for (int ly = 0; ly < h; ly++)
                        memcpy(out_se + (size_t)(y0 + ly) * width + x0, se[i].data() + ((size_t)st * R.tile_h + ly) * R.tile_w, (size_t)w * sizeof(float));
                }
            }
        }
        if (summary) { // the shards' entries in the order of the frame's sub-tiles: the unsharded monitor's sum, term for term
            RenderView F{};
            F.width = width; F.height = height;
            std::vector<NoiseTile> frame(noise_frame_subtiles(F), NoiseTile{0.f, 0.f, 0u, 0u});
            for (size_t i = 0; i < N; i++)
                if (n->shard[i]) noise_place_tiles(n->shard[i]->accum->view, tiles[i], frame);
            noise_summarise(frame, n->shard[0], summary);
        }
        return RT_OK;
    });
}

} // extern "C"

// Multi-GPU render under the C-ABI (include/rtamd.h: rt_multi_*): one process, one rt_scene per HIP device, one host thread
// per device, the frame's 32x32 tiles dealt round-robin to the devices (the per-pixel seed y*W+x is global, so any deal gives
// the reference's pixels: hw8/src/sceneio.cpp:389-391), and ONE exchange step: every device PUSHES its compact shard buffer to its
// landing area on device 0 (hipMemcpyPeerAsync on the sender's own stream, straight after its render: each sender over its own xGMI
// link, in the direction peer access was enabled for, overlapping the slower shards' renders) and records an event; device 0's
// stream waits for each event and scatters that shard's tiles into the frame.  The host-side preparation of the scene (the replay of
// the reference's figure order) runs once and is shared by the devices' scenes (host/shared_prep.h).
// This is what `./run.sh scene.gltf W H SPP out.ppm` (csrc/cli/main.cpp) uses when more than one GPU is visible; the
// reference seam is the pixel loop of sceneio::renderScene driven from main (hw8/src/main.cpp:7-18).
// Resumable renders on the same devices (rt_multi_accum_*, second half of this file): one sharded rt_accum per device, the picture through
// the same exchange, and a checkpoint regrouped on device 0 into the unsharded rt_accum's own blob.
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "../../include/rtamd.h"
#include "device/rt_device.h"
#include "host/rt_accum_state.h"
#include "host/shared_prep.h"

using namespace rtamd;

namespace {

// shard `shard` of `count` holds the tiles shard, shard + count, ... in order (layout of rt_render_params); one thread per element
template <class T>
__global__ void assemble_tiles_kernel(const T *shard_buf, T *frame, int width, int height, int tile, int tiles_x, int shard, int count, uint32_t n_tiles) {
    const size_t per_tile = (size_t)tile * tile * 3;
    const size_t n = (size_t)n_tiles * per_tile;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t st = (uint32_t)(i / per_tile);
        const uint32_t r = (uint32_t)(i % per_tile);
        const int ly = (int)(r / (3u * tile)), lx = (int)((r / 3u) % tile), c = (int)(r % 3u);
        const uint32_t gt = (uint32_t)shard + st * (uint32_t)count;
        const int x = (int)(gt % (uint32_t)tiles_x) * tile + lx, y = (int)(gt / (uint32_t)tiles_x) * tile + ly;
        if (x < width && y < height) frame[((size_t)y * width + x) * 3 + c] = shard_buf[i];
    }
}

// Resumable state between the order of a shard (rt_accum of shard `shard` of `count`: the 8x8 sub-tiles of its tiles) and the frame order
// of the portable checkpoint (device/rt_device.h shard_slot_to_frame_slot).  A state is n x {sum r, g, b, engine} as uint4, then n x {saved,
// has_saved} as uint2.  One thread per slot of the shard: a wave moves one sub-tile, 1 KB + 512 B, contiguous on both sides.
struct Regroup { int tile, tiles_x, sub_w, sub_h; uint32_t shard, count, n_slots, frame_slots; };
__global__ __launch_bounds__(256) void shard_to_frame_kernel(const uint32_t *shard_state, uint32_t *frame_state, Regroup G) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(shard_state);
    const uint2 *s2 = reinterpret_cast<const uint2 *>(shard_state + 4 * (size_t)G.n_slots);
    uint4 *f4 = reinterpret_cast<uint4 *>(frame_state);
    uint2 *f2 = reinterpret_cast<uint2 *>(frame_state + 4 * (size_t)G.frame_slots);
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < G.n_slots; s += gridDim.x * 256u) {
        uint32_t f;
        if (!rtamd::dev::shard_slot_to_frame_slot(G.tile, G.tiles_x, G.sub_w, G.sub_h, G.shard, G.count, s, f)) continue; // a padding sub-tile
        f4[f] = s4[s]; f2[f] = s2[s];
    }
}
// ... and back; the shard's padding sub-tiles get the zeros a fresh state has there (accum_seed_kernel)
__global__ __launch_bounds__(256) void frame_to_shard_kernel(const uint32_t *frame_state, uint32_t *shard_state, Regroup G) {
    const uint4 *f4 = reinterpret_cast<const uint4 *>(frame_state);
    const uint2 *f2 = reinterpret_cast<const uint2 *>(frame_state + 4 * (size_t)G.frame_slots);
    uint4 *s4 = reinterpret_cast<uint4 *>(shard_state);
    uint2 *s2 = reinterpret_cast<uint2 *>(shard_state + 4 * (size_t)G.n_slots);
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < G.n_slots; s += gridDim.x * 256u) {
        uint32_t f;
        const bool in_frame = rtamd::dev::shard_slot_to_frame_slot(G.tile, G.tiles_x, G.sub_w, G.sub_h, G.shard, G.count, s, f);
        s4[s] = in_frame ? f4[f] : make_uint4(0u, 0u, 0u, 0u);
        s2[s] = in_frame ? f2[f] : make_uint2(0u, 0u);
    }
}

// The host threads of a call, one per device: joined on every way out, so that a thread that could not be started (emplace_back
// throws std::system_error) leaves the started ones finished behind it instead of a std::terminate in their destructors.
struct Threads {
    std::vector<std::thread> th;
    void join() { for (auto &t : th) if (t.joinable()) t.join(); }
    ~Threads() { join(); }
};

struct DeviceSlot {
    int device = 0;
    rt_scene *scene = nullptr;
    hipStream_t stream = nullptr;
    float *d_rgb = nullptr;       // this device's shard, float
    uint8_t *d_rgb8 = nullptr;    // this device's shard, u8
    size_t cap_rgb = 0, cap_rgb8 = 0; // bytes (grow)
    hipEvent_t done = nullptr;    // recorded on `stream` after this device's shard has landed on device 0
};

} // namespace

struct rt_multi {
    std::vector<DeviceSlot> dev;
    // on device 0: landing areas of the other devices' shards and the assembled frame
    std::vector<float *> land_rgb;
    std::vector<uint8_t *> land_rgb8;
    std::vector<size_t> land_cap_rgb, land_cap_rgb8;
    float *frame_rgb = nullptr;
    uint8_t *frame_rgb8 = nullptr;
    size_t frame_cap_rgb = 0, frame_cap_rgb8 = 0;
    // on device 0, for the checkpoints of rt_multi_accum: landing areas of the other devices' states and the state in frame order
    std::vector<uint32_t *> land_state;
    std::vector<size_t> land_cap_state;
    uint32_t *frame_state = nullptr;
    size_t frame_cap_state = 0;
    hipEvent_t state_ready = nullptr; // recorded on device 0's stream when a loaded state has been regrouped for every shard
    ~rt_multi() {
        for (size_t i = 0; i < dev.size(); i++) {
            if (!dev[i].scene && !dev[i].stream && !dev[i].d_rgb && !dev[i].d_rgb8) continue; // nothing was created on it (it may not even exist)
            (void)hipSetDevice(dev[i].device);
            if (dev[i].scene) rt_scene_destroy(dev[i].scene);
            if (dev[i].d_rgb) (void)hipFree(dev[i].d_rgb);
            if (dev[i].d_rgb8) (void)hipFree(dev[i].d_rgb8);
            if (dev[i].stream) (void)hipStreamDestroy(dev[i].stream);
            if (dev[i].done) (void)hipEventDestroy(dev[i].done);
        }
        if (!dev.empty() && dev[0].scene) (void)hipSetDevice(dev[0].device);
        for (float *p : land_rgb) if (p) (void)hipFree(p);
        for (uint8_t *p : land_rgb8) if (p) (void)hipFree(p);
        if (frame_rgb) (void)hipFree(frame_rgb);
        if (frame_rgb8) (void)hipFree(frame_rgb8);
        for (uint32_t *p : land_state) if (p) (void)hipFree(p);
        if (frame_state) (void)hipFree(frame_state);
        if (state_ready) (void)hipEventDestroy(state_ready);
        (void)hipGetLastError(); // a failed teardown call must not surface in somebody else's next launch check
    }
};

// fn(i), an rt_status with its message in rt_last_error, for every device entry i of n that has a device (device_of(i) >= 0), each on
// its own host thread with that device current; all threads are joined on every way out.  Returns the first failure in entry order:
// its status, and `who` + "device N: " + its message.  The serial sibling is each_device (host/rt_accum_state.h).
template <class DeviceOf, class Fn> static int fan_out(const std::string &who, int n, DeviceOf device_of, Fn fn) {
    std::vector<int> rc((size_t)n, RT_OK);
    std::vector<std::string> err((size_t)n);
    {
        Threads threads;
        for (int i = 0; i < n; i++)
            if (device_of(i) >= 0)
                threads.th.emplace_back([&, i] {
                    rc[i] = guarded("", [&]() -> int { // nothing leaves a thread either; the outer guard is for the copy of the message
                        const int r = guarded("", [&]() -> int {
                            if (hipSetDevice(device_of(i)) != hipSuccess) return fail(RT_ERR_HIP, "hipSetDevice failed");
                            return fn(i);
                        });
                        if (r != RT_OK) err[i] = rt_last_error();
                        return r;
                    });
                });
    }
    for (int i = 0; i < n; i++)
        if (rc[i] != RT_OK) return fail(rc[i], who + "device " + std::to_string(device_of(i)) + ": " + err[i]);
    return RT_OK;
}

// The exchange step of a frame, shared by rt_multi_render and rt_multi_accum_resolve.  Every device fills its compact shard buffers
// from its own host thread (`produce(i, d_rgb, d_rgb8)`, an rt_status with the message left in rt_last_error; elems[i] == 0: an
// empty shard, not called) and pushes them to its landing area on device 0 (hipMemcpyPeerAsync on its own stream, then an event);
// device 0's stream waits for each event and scatters that shard's tiles into the frame, which is read back to the host or, with
// out_dev, assembled in the caller's memory on device 0.  One device: its buffers hold the plain frame, which is copied out.
template <class Produce>
static int exchange_frame(rt_multi *m, const std::string &who, int width, int height, int tile, bool out_dev, float *out_rgb, uint8_t *out_rgb8,
                          const std::vector<size_t> &elems, Produce produce) {
    const int N = (int)m->dev.size();
    // landing areas on device 0 and the frame, before any thread starts (allocations on device 0 from this thread only)
    const int dev0 = m->dev[0].device;
    HIP_CHECK(hipSetDevice(dev0));
    hipStream_t s0 = m->dev[0].stream;
    const size_t frame_elems = (size_t)width * height * 3;
    float *frame_rgb = nullptr;
    uint8_t *frame_rgb8 = nullptr;
    if (N > 1) {
        if (out_rgb) { if (out_dev) frame_rgb = out_rgb; else { grow(m->frame_rgb, m->frame_cap_rgb, frame_elems * sizeof(float)); frame_rgb = m->frame_rgb; } }
        if (out_rgb8) { if (out_dev) frame_rgb8 = out_rgb8; else { grow(m->frame_rgb8, m->frame_cap_rgb8, frame_elems); frame_rgb8 = m->frame_rgb8; } }
        for (int i = 1; i < N; i++) {
            if (elems[i] == 0) continue;
            if (out_rgb) grow(m->land_rgb[i], m->land_cap_rgb[i], elems[i] * sizeof(float));
            if (out_rgb8) grow(m->land_rgb8[i], m->land_cap_rgb8[i], elems[i]);
        }
    }
    // every device fills its shard from its own host thread and pushes it to device 0 as soon as it is done
    const int rc = fan_out(who, N, [&](int i) { return m->dev[i].device; }, [&](int i) -> int {
        DeviceSlot &d = m->dev[i];
        if (elems[i] == 0) return RT_OK; // more devices than tiles
        if (out_rgb) grow(d.d_rgb, d.cap_rgb, elems[i] * sizeof(float));
        if (out_rgb8) grow(d.d_rgb8, d.cap_rgb8, elems[i]);
        if (const int r = produce(i, out_rgb ? d.d_rgb : nullptr, out_rgb8 ? d.d_rgb8 : nullptr)) return r;
        if (i > 0 && N > 1) { // the push: this device's stream, this device's link
            hipError_t e = hipSuccess;
            if (out_rgb) e = hipMemcpyPeerAsync(m->land_rgb[i], dev0, d.d_rgb, d.device, elems[i] * sizeof(float), d.stream);
            if (e == hipSuccess && out_rgb8) e = hipMemcpyPeerAsync(m->land_rgb8[i], dev0, d.d_rgb8, d.device, elems[i], d.stream);
            if (e == hipSuccess) e = hipEventRecord(d.done, d.stream);
            if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("shard push: ") + hipGetErrorString(e));
        }
        return RT_OK;
    });
    if (rc != RT_OK) return rc;
    // tiles -> frame on device 0, each shard as soon as its push has landed
    HIP_CHECK(hipSetDevice(dev0));
    if (N == 1) { frame_rgb = m->dev[0].d_rgb; frame_rgb8 = m->dev[0].d_rgb8; }
    else {
        const int tiles_x = (width + tile - 1) / tile, tiles_y = (height + tile - 1) / tile;
        const uint32_t total_tiles = (uint32_t)tiles_x * (uint32_t)tiles_y;
        for (int i = 0; i < N; i++) {
            if (elems[i] == 0) continue;
            const uint32_t n_tiles = (total_tiles - (uint32_t)i + (uint32_t)N - 1) / (uint32_t)N;
            const float *src_rgb = i ? m->land_rgb[i] : m->dev[0].d_rgb;
            const uint8_t *src_rgb8 = i ? m->land_rgb8[i] : m->dev[0].d_rgb8;
            if (i > 0) HIP_CHECK(hipStreamWaitEvent(s0, m->dev[i].done, 0));
            const unsigned blocks = (unsigned)((elems[i] + 255) / 256 < 65535 ? (elems[i] + 255) / 256 : 65535);
            if (out_rgb) hipLaunchKernelGGL(assemble_tiles_kernel<float>, dim3(blocks), dim3(256), 0, s0, src_rgb, frame_rgb, width, height, tile, tiles_x, i, N, n_tiles);
            if (out_rgb8) hipLaunchKernelGGL(assemble_tiles_kernel<uint8_t>, dim3(blocks), dim3(256), 0, s0, src_rgb8, frame_rgb8, width, height, tile, tiles_x, i, N, n_tiles);
        }
        HIP_CHECK(hipGetLastError());
    }
    if (!out_dev) {
        if (out_rgb) HIP_CHECK(hipMemcpyAsync(out_rgb, frame_rgb, frame_elems * sizeof(float), hipMemcpyDeviceToHost, s0));
        if (out_rgb8) HIP_CHECK(hipMemcpyAsync(out_rgb8, frame_rgb8, frame_elems, hipMemcpyDeviceToHost, s0));
    } else if (N == 1) {
        if (out_rgb) HIP_CHECK(hipMemcpyAsync(out_rgb, frame_rgb, frame_elems * sizeof(float), hipMemcpyDeviceToDevice, s0));
        if (out_rgb8) HIP_CHECK(hipMemcpyAsync(out_rgb8, frame_rgb8, frame_elems, hipMemcpyDeviceToDevice, s0));
    }
    HIP_CHECK(hipStreamSynchronize(s0));
    return RT_OK;
}

// What a frame on all devices of `m` needs settled before anything runs, for rt_multi_render (`render`) and rt_multi_accum_create: the
// refusals the two share, the square tile, and per device entry the rt_render_params of its shard (shard i of N on that entry's
// stream; with one entry the unsharded frame) and the elements of its compact picture (0: more entries than tiles).
struct FramePlan {
    int tile = 32;
    std::vector<rt_render_params> p;
    std::vector<size_t> elems;
};
static int plan_frame(const rt_multi *m, const rt_render_params *params, const std::string &who, bool render, FramePlan &P) {
    if (params->struct_size != sizeof(rt_render_params)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (params->shard_count > 1) return fail(RT_ERR_INVALID_ARG, who + "the frame is sharded over the devices here; shard_count must be 0 or 1");
    if (render && params->integrator == RT_INTEGRATOR_HW1) return fail(RT_ERR_UNSUPPORTED, who + "the hw1 caster renders unsharded frames only"); // an rt_accum refuses hw1 itself
    P.tile = params->tile_w > 0 ? params->tile_w : 32;
    if (params->tile_h > 0 && params->tile_h != P.tile) return fail(RT_ERR_INVALID_ARG, who + "square tiles only");
    const int N = (int)m->dev.size();
    P.p.assign((size_t)N, *params);
    P.elems.assign((size_t)N, 0);
    for (int i = 0; i < N; i++) {
        rt_render_params &p = P.p[i];
        p.shard_index = N > 1 ? i : 0; p.shard_count = N > 1 ? N : 1; p.tile_w = p.tile_h = P.tile;
        p.stream = m->dev[i].stream;
        rt_render_params q = p;
        q.samples = 1; // rt_output_elems looks at it; whether the frame has samples is the caller's business
        P.elems[i] = N > 1 ? rt_output_elems(&q) : (size_t)(params->width > 0 && params->height > 0 ? (size_t)params->width * params->height * 3 : 0);
    }
    return RT_OK;
}

// rt_stats of a call on all devices from the shards' (empty shards left out): sums, except the times of devices that work side by side
static void sum_stats(const std::vector<rt_stats> &st, const std::vector<size_t> &work, rt_stats *stats) {
    memset(stats, 0, sizeof *stats);
    for (size_t i = 0; i < st.size(); i++) {
        if (work[i] == 0) continue;
        stats->kernel_ms = st[i].kernel_ms > stats->kernel_ms ? st[i].kernel_ms : stats->kernel_ms;            // the devices render side by side
        stats->dominant_kernel_ms = st[i].dominant_kernel_ms > stats->dominant_kernel_ms ? st[i].dominant_kernel_ms : stats->dominant_kernel_ms;
        stats->samples += st[i].samples;
        stats->closest_hit_queries += st[i].closest_hit_queries; stats->light_pdf_queries += st[i].light_pdf_queries;
        stats->node_visits += st[i].node_visits; stats->triangle_tests += st[i].triangle_tests;
        stats->launches += st[i].launches; stats->dominant_kernel_launches += st[i].dominant_kernel_launches;
        stats->exact_closest_hits += st[i].exact_closest_hits; stats->exact_light_sums += st[i].exact_light_sums;
        stats->pipeline = st[i].pipeline;
    }
}

extern "C" {

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_multi_create(const rt_scene_desc *desc, const int *devices, int n_devices, rt_multi **out) {
    if (!desc || !out || n_devices < 1 || n_devices > 64) return fail(RT_ERR_INVALID_ARG, "rt_multi_create: bad argument (1..64 devices)");
    *out = nullptr;
    const int visible = rt_device_count();
    if (visible == 0) return fail(RT_ERR_NO_DEVICE, "rt_multi_create: no HIP device available (this library has no CPU fallback)");
    return guarded("rt_multi_create: ", [&]() -> int { // also std::bad_alloc and the std::system_error of a thread that could not start
        std::unique_ptr<rt_multi> m(new rt_multi());
        rtamd::SharedPrep prep; // one host-side preparation for all devices
        m->dev.resize((size_t)n_devices);
        for (int i = 0; i < n_devices; i++) {
            m->dev[i].device = devices ? devices[i] : i;
            if (m->dev[i].device < 0 || m->dev[i].device >= visible) return fail(RT_ERR_INVALID_ARG, "rt_multi_create: device index out of range");
        }
        // one scene per device; the host-side preparation (BVH replay) of each runs on its own thread
        const int rc = fan_out("rt_multi_create: ", n_devices, [&](int i) { return m->dev[i].device; }, [&](int i) -> int {
            if (const int r = rtamd::scene_create_shared(desc, &m->dev[i].scene, &prep)) return r;
            if (hipStreamCreateWithFlags(&m->dev[i].stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&m->dev[i].done, hipEventDisableTiming) != hipSuccess)
                return fail(RT_ERR_HIP, "stream / event creation failed");
            return RT_OK;
        });
        if (rc != RT_OK) return rc;
        // peer access from every sender towards device 0 — the direction of its push — where the hardware offers it (hipMemcpyPeerAsync
        // stages through the host otherwise)
        for (int i = 1; i < n_devices; i++) {
            if (m->dev[i].device == m->dev[0].device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, m->dev[i].device, m->dev[0].device) == hipSuccess && can) {
                (void)hipSetDevice(m->dev[i].device);
                hipError_t e = hipDeviceEnablePeerAccess(m->dev[0].device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            }
        }
        (void)hipSetDevice(m->dev[0].device);
        m->land_rgb.assign((size_t)n_devices, nullptr); m->land_rgb8.assign((size_t)n_devices, nullptr);
        m->land_cap_rgb.assign((size_t)n_devices, 0); m->land_cap_rgb8.assign((size_t)n_devices, 0);
        m->land_state.assign((size_t)n_devices, nullptr); m->land_cap_state.assign((size_t)n_devices, 0);
        HIP_CHECK(hipEventCreateWithFlags(&m->state_ready, hipEventDisableTiming));
        *out = m.release();
        return RT_OK;
    });
}

void rt_multi_destroy(rt_multi *m) { delete m; }

int rt_multi_render(rt_multi *m, const rt_render_params *params, float *out_rgb, uint8_t *out_rgb8, rt_stats *stats) {
    if (!m || !params) return fail(RT_ERR_INVALID_ARG, "rt_multi_render: null argument");
    return guarded("rt_multi_render: ", [&]() -> int {
        const double t0 = now_ms();
        FramePlan P;
        if (const int rc = plan_frame(m, params, "rt_multi_render: ", true, P)) return rc;
        for (rt_render_params &p : P.p) p.flags = params->flags | RT_FLAG_OUT_DEVICE;
        if (params->width <= 0 || params->height <= 0 || params->samples <= 0) return fail(RT_ERR_INVALID_ARG, "rt_multi_render: width, height and samples must be positive");
        std::vector<rt_stats> st(P.p.size());
        for (auto &x : st) memset(&x, 0, sizeof x);
        const int rc = exchange_frame(m, "rt_multi_render: ", params->width, params->height, P.tile, (params->flags & RT_FLAG_OUT_DEVICE) != 0, out_rgb, out_rgb8, P.elems,
                                      [&](int i, float *d_rgb, uint8_t *d_rgb8) { return rt_render(m->dev[i].scene, &P.p[i], d_rgb, d_rgb8, &st[i]); });
        if (rc != RT_OK) return rc;
        if (stats) {
            sum_stats(st, P.elems, stats);
            stats->total_ms = now_ms() - t0; // host wall time of the whole call: renders, exchange, read-back
        }
        return RT_OK;
    });
}

// ---- resumable renders on all devices (include/rtamd.h: rt_multi_accum_*) ---------------------------------------------------
// One sharded rt_accum per device entry (struct rt_multi_accum, host/rt_accum_state.h), advanced side
// by side; the picture goes through the exchange of rt_multi_render; the checkpoint is regrouped on device 0 into the frame order,
// where it is the blob of the unsharded single-device rt_accum.  With one entry the rt_accum IS that unsharded one.
static Regroup regroup_of(const rt_multi_accum *a, int i) {
    Regroup G;
    G.tile = a->tile; G.tiles_x = (a->params.width + a->tile - 1) / a->tile; G.sub_w = a->frame.tiles_x; G.sub_h = a->frame.tiles_y;
    G.shard = (uint32_t)i; G.count = (uint32_t)a->shard.size(); G.n_slots = a->shard[i]->n_pixslots; G.frame_slots = a->frame_slots;
    return G;
}
static unsigned regroup_blocks(uint32_t n_slots) { return (n_slots + 255u) / 256u < 65535u ? (n_slots + 255u) / 256u : 65535u; }

int rt_multi_accum_create(rt_multi *m, const rt_render_params *params, rt_multi_accum **out) {
    if (!m || !params || !out) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_create: null argument");
    *out = nullptr;
    return guarded("rt_multi_accum_create: ", [&]() -> int {
        FramePlan P;
        if (const int rc = plan_frame(m, params, "rt_multi_accum_create: ", false, P)) return rc;
        const int N = (int)m->dev.size();
        std::unique_ptr<rt_multi_accum> a(new rt_multi_accum());
        a->multi = m; a->params = *params; a->params.samples = 0; a->params.shard_index = 0; a->params.shard_count = 1; a->tile = P.tile;
        a->shard.assign((size_t)N, nullptr); a->elems = P.elems;
        a->sample_limit = 0;
        for (int i = 0; i < N; i++) {
            if (i > 0 && a->elems[i] == 0) continue; // more devices than tiles; the first entry always has a tile, and makes every refusal
            HIP_CHECK(hipSetDevice(m->dev[i].device));
            const int rc = rt_accum_create(m->dev[i].scene, &P.p[i], &a->shard[i]); // its samples field is ignored there
            if (rc != RT_OK) return fail(rc, "rt_multi_accum_create: device " + std::to_string(m->dev[i].device) + ": " + rt_last_error());
            if (a->sample_limit == 0 || a->shard[i]->sample_limit < a->sample_limit) a->sample_limit = a->shard[i]->sample_limit;
        }
        std::string err;
        rt_render_params q = a->params;
        q.samples = 1;
        if (!rtamd::resolve_tiles(&q, a->frame, err)) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_create: " + err);
        a->frame_slots = (uint32_t)a->frame.tiles_x * (uint32_t)a->frame.tiles_y * 64u; // below 2^30: rt_accum_create has taken shard 0 of this frame
        HIP_CHECK(hipSetDevice(m->dev[0].device));
        *out = a.release();
        return RT_OK;
    });
}

void rt_multi_accum_destroy(rt_multi_accum *a) { delete a; }

int rt_multi_accum_samples(const rt_multi_accum *a) {
    if (!a) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_samples: null argument");
    return a->samples;
}

#define MA_ENTER(name)                                                                                                                      \
    if (!a) return fail(RT_ERR_INVALID_ARG, name ": null argument");                                                                          \
    if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, name ": an earlier call failed under way and left the state half advanced (" + a->broken + ")")
// a failure after the devices have started: the object is broken from here on
#define MA_BREAK(rc_) do { a->broken = rt_last_error(); return (rc_); } while (0)

// the HIP device of entry i's shard, -1 for an empty shard (fan_out, each_device)
static int shard_device(const rt_multi_accum *a, size_t i) { return a->shard[i] ? a->multi->dev[i].device : -1; }

int rt_multi_accum_render(rt_multi_accum *a, int32_t n_samples, rt_stats *stats) {
    return guarded("rt_multi_accum_render: ", [&]() -> int {
        MA_ENTER("rt_multi_accum_render");
        rt_multi *m = a->multi;
        const int N = (int)a->shard.size();
        const double t0 = now_ms();
        if (n_samples <= 0) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_render: n_samples must be positive");
        if ((int64_t)a->samples + n_samples >= (int64_t)a->sample_limit)
            return fail(RT_ERR_LIMIT, "rt_multi_accum_render: " + std::to_string(a->samples) + " + " + std::to_string(n_samples) + " samples per pixel do not fit the path records' sample index (below " + std::to_string(a->sample_limit) + " on some device)");
        for (int i = 0; i < N; i++) // every refusal before any device launches: the state stays as it was
            if (a->shard[i]) if (const int rc = rtamd::accum_check_slice(a->shard[i], n_samples, "rt_multi_accum_render: device " + std::to_string(m->dev[i].device) + ": ")) return rc;
        std::vector<rt_stats> st((size_t)N);
        for (auto &x : st) memset(&x, 0, sizeof x);
        const int rc = guarded("rt_multi_accum_render: ", [&]() -> int { // a thread that could not be started: the others have run
            return fan_out("rt_multi_accum_render: ", N, [&](int i) { return shard_device(a, (size_t)i); }, [&](int i) { return rt_accum_render(a->shard[i], n_samples, &st[i]); });
        });
        (void)hipSetDevice(m->dev[0].device);
        if (rc != RT_OK) MA_BREAK(rc);
        a->samples += n_samples;
        if (stats) {
            sum_stats(st, a->elems, stats);
            stats->samples = (uint64_t)a->params.width * (uint64_t)a->params.height * (uint64_t)n_samples;
            stats->reference_exact = 1;
            for (int i = 0; i < N; i++) if (a->shard[i]) stats->reference_exact &= st[i].reference_exact;
            stats->total_ms = now_ms() - t0;
        }
        return RT_OK;
    });
}

int rt_multi_accum_resolve(rt_multi_accum *a, uint32_t flags, float *out_rgb, uint8_t *out_rgb8) {
    return guarded("rt_multi_accum_resolve: ", [&]() -> int {
        MA_ENTER("rt_multi_accum_resolve");
        if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_resolve: flags other than RT_FLAG_OUT_DEVICE");
        if (a->samples <= 0) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_resolve: no samples yet (a picture needs at least one)");
        if (!out_rgb && !out_rgb8) return RT_OK;
        // the state is only read; each device resolves its shard on device in the compact layout (accum_resolve_kernel)
        return exchange_frame(a->multi, "rt_multi_accum_resolve: ", a->params.width, a->params.height, a->tile, (flags & RT_FLAG_OUT_DEVICE) != 0, out_rgb, out_rgb8, a->elems,
                              [&](int i, float *d_rgb, uint8_t *d_rgb8) { return rt_accum_resolve(a->shard[i], RT_FLAG_OUT_DEVICE, d_rgb, d_rgb8); });
    });
}

// The buffers on device 0 that a checkpoint passes through: the state in frame order and the landing areas of the other devices' states.
static void grow_state_buffers(rt_multi_accum *a) {
    rt_multi *m = a->multi;
    grow(m->frame_state, m->frame_cap_state, (size_t)a->frame_slots * ACCUM_SLOT_BYTES);
    for (size_t i = 1; i < a->shard.size(); i++)
        if (a->shard[i]) grow(m->land_state[i], m->land_cap_state[i], (size_t)a->shard[i]->n_pixslots * ACCUM_SLOT_BYTES);
}

// Save: every device pushes its shard's state to its landing area on device 0 (its own stream, an event), device 0 scatters each
// landed shard into the frame-order buffer and copies header + buffer to the host once.
int rt_multi_accum_save(rt_multi_accum *a, void *blob, size_t capacity) {
    return guarded("rt_multi_accum_save: ", [&]() -> int {
        MA_ENTER("rt_multi_accum_save");
        if (!blob) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_save: null argument");
        const size_t state = (size_t)a->frame_slots * ACCUM_SLOT_BYTES;
        if (capacity < ACCUM_HEADER_BYTES + state) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_save: buffer smaller than rt_accum_state_bytes of the unsharded frame");
        rt_multi *m = a->multi;
        const int N = (int)a->shard.size();
        const int dev0 = m->dev[0].device;
        HIP_CHECK(hipSetDevice(dev0));
        if (N == 1) { // the unsharded rt_accum itself
            const int rc = rt_accum_save(a->shard[0], blob, capacity);
            return rc == RT_OK ? rc : fail(rc, std::string("rt_multi_accum_save: ") + rt_last_error());
        }
        hipStream_t s0 = m->dev[0].stream;
        grow_state_buffers(a);
        each_device((size_t)N, [&](size_t i) { return i ? shard_device(a, i) : -1; }, [&](size_t i) { // the pushes: each on its device's stream, behind that device's last slice
            HIP_CHECK(hipMemcpyPeerAsync(m->land_state[i], dev0, a->shard[i]->d_state, m->dev[i].device, (size_t)a->shard[i]->n_pixslots * ACCUM_SLOT_BYTES, m->dev[i].stream));
            HIP_CHECK(hipEventRecord(m->dev[i].done, m->dev[i].stream));
            return RT_OK;
        });
        HIP_CHECK(hipSetDevice(dev0));
        for (int i = 0; i < N; i++) {
            if (!a->shard[i]) continue;
            if (i > 0) HIP_CHECK(hipStreamWaitEvent(s0, m->dev[i].done, 0));
            const Regroup G = regroup_of(a, i);
            hipLaunchKernelGGL(shard_to_frame_kernel, dim3(regroup_blocks(G.n_slots)), dim3(256), 0, s0, i ? m->land_state[i] : a->shard[0]->d_state, m->frame_state, G);
        }
        HIP_CHECK(hipGetLastError());
        uint32_t h[ACCUM_HEADER_BYTES / 4];
        accum_header(m->dev[0].scene, a->params.integrator, a->frame, a->frame_slots, a->samples, h);
        memcpy(blob, h, ACCUM_HEADER_BYTES);
        HIP_CHECK(hipMemcpyAsync((uint8_t *)blob + ACCUM_HEADER_BYTES, m->frame_state, state, hipMemcpyDeviceToHost, s0));
        HIP_CHECK(hipStreamSynchronize(s0));
        return RT_OK;
    });
}

// Load: the reverse.  The blob goes to device 0, which gathers every shard's slots out of the frame order (its own shard in place,
// the others into their landing areas); every other device then pulls its state over on its own stream.
int rt_multi_accum_load(rt_multi_accum *a, const void *blob, size_t size) {
    return guarded("rt_multi_accum_load: ", [&]() -> int {
        MA_ENTER("rt_multi_accum_load");
        if (!blob) return fail(RT_ERR_INVALID_ARG, "rt_multi_accum_load: null argument");
        rt_multi *m = a->multi;
        const int N = (int)a->shard.size();
        uint32_t want[ACCUM_HEADER_BYTES / 4];
        accum_header(m->dev[0].scene, a->params.integrator, a->frame, a->frame_slots, a->samples, want);
        const size_t state = (size_t)a->frame_slots * ACCUM_SLOT_BYTES;
        const int samples = accum_check_blob(want, blob, size, a->sample_limit, state, "rt_multi_accum_load: ");
        if (samples < 0) return samples;
        const int dev0 = m->dev[0].device;
        HIP_CHECK(hipSetDevice(dev0));
        if (N == 1) { // the unsharded rt_accum itself
            const int rc = rt_accum_load(a->shard[0], blob, size);
            if (rc != RT_OK) return fail(rc, std::string("rt_multi_accum_load: ") + rt_last_error());
            a->samples = samples;
            a->loads++;
            return RT_OK;
        }
        hipStream_t s0 = m->dev[0].stream;
        grow_state_buffers(a);
        // from here on the devices' states are being overwritten: a failure leaves the object broken
        a->loads++;
        const int rc = guarded("rt_multi_accum_load: ", [&]() -> int {
            HIP_CHECK(hipMemcpyAsync(m->frame_state, (const uint8_t *)blob + ACCUM_HEADER_BYTES, state, hipMemcpyHostToDevice, s0));
            for (int i = 0; i < N; i++) {
                if (!a->shard[i]) continue;
                const Regroup G = regroup_of(a, i);
                hipLaunchKernelGGL(frame_to_shard_kernel, dim3(regroup_blocks(G.n_slots)), dim3(256), 0, s0, m->frame_state, i ? m->land_state[i] : a->shard[0]->d_state, G);
                HIP_CHECK(hipGetLastError());
            }
            HIP_CHECK(hipEventRecord(m->state_ready, s0));
            each_device((size_t)N, [&](size_t i) { return i ? shard_device(a, i) : -1; }, [&](size_t i) { // the pulls, each on its device's stream
                HIP_CHECK(hipStreamWaitEvent(m->dev[i].stream, m->state_ready, 0));
                HIP_CHECK(hipMemcpyPeerAsync(a->shard[i]->d_state, m->dev[i].device, m->land_state[i], dev0, (size_t)a->shard[i]->n_pixslots * ACCUM_SLOT_BYTES, m->dev[i].stream));
                return RT_OK;
            });
            return each_device((size_t)N, [&](size_t i) { return shard_device(a, i); }, [&](size_t i) { HIP_CHECK(hipStreamSynchronize(m->dev[i].stream)); return RT_OK; });
        });
        if (rc != RT_OK) {
            (void)hipSetDevice(dev0);
            MA_BREAK(rc);
        }
        for (int i = 0; i < N; i++) if (a->shard[i]) a->shard[i]->samples = samples;
        a->samples = samples;
        return RT_OK;
    });
}

} // extern "C"

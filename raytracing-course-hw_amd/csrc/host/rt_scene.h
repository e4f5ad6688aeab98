// struct rt_scene, the frame geometry and the small helpers that the two translation units of the render path share:
// rtamd_scene.hip creates and destroys a scene, rtamd_api.hip renders it (and keeps its per-render state in it).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../../include/rtamd.h"
#include "../device/rt_types.h"
#include "../device/rt_types_hw5.h"
#include "../device/rt_types_hw6.h"
#include "../device/rt_types_txt.h"
#include "../device/rt_types_wf.h"
#include "rt_guard.h"

namespace rtamd {
namespace { // internal linkage: the library exports none of these helpers

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Device allocation freed on every way out of its scope, unless release() hands it on.
struct OwnedDev {
    void *p = nullptr;
    OwnedDev() = default;
    explicit OwnedDev(void *q) : p(q) {}
    OwnedDev(const OwnedDev &) = delete;
    OwnedDev &operator=(const OwnedDev &) = delete;
    OwnedDev(OwnedDev &&o) : p(o.release()) {}
    ~OwnedDev() { if (p) (void)hipFree(p); }
    void *release() { void *q = p; p = nullptr; return q; }
};

// A device buffer that a call needs `need` bytes of: kept when it is large enough, else freed and allocated anew.
template <class T> void grow(T *&p, size_t &have, size_t need) {
    if (have >= need) return;
    if (p) (void)hipFree(p);
    p = nullptr; have = 0;
    HIP_CHECK(hipMalloc((void **)&p, need));
    have = need;
}

// An output of `elems` elements that the caller wants at `out`: device memory with RT_FLAG_OUT_DEVICE, which the kernel then writes
// itself, else host memory, which gets a device buffer of this call (dev), the copy back queued by copy_back(), freed on every way out.
struct StagedOut {
    void *dev;          // what the kernel writes; null = no such output
    void *host = nullptr;
    size_t bytes = 0;
    OwnedDev buf;
    StagedOut(void *out, uint32_t flags, size_t elems, size_t elem_size) : dev(out) {
        if (!out || (flags & RT_FLAG_OUT_DEVICE)) return;
        dev = nullptr;
        if (!elems) return;
        bytes = elems * elem_size;
        HIP_CHECK(hipMalloc(&buf.p, bytes));
        host = out; dev = buf.p;
    }
    void copy_back(hipStream_t stream) const { if (buf.p) HIP_CHECK(hipMemcpyAsync(host, buf.p, bytes, hipMemcpyDeviceToHost, stream)); }
};

template <class T> T *upload(const std::vector<T> &v, uint64_t &bytes) {
    OwnedDev d;
    const size_t n = v.size() * sizeof(T), dummy = sizeof(T) > 16 ? sizeof(T) : 16;
    if (v.empty()) { // keep pointers valid: one dummy element
        HIP_CHECK(hipMalloc(&d.p, dummy));
        HIP_CHECK(hipMemset(d.p, 0, dummy));
    } else {
        HIP_CHECK(hipMalloc(&d.p, n));
        HIP_CHECK(hipMemcpy(d.p, v.data(), n, hipMemcpyHostToDevice));
        bytes += n;
    }
    return (T *)d.release();
}

// Geometry of a frame and of its shards (include/rtamd.h rt_render_params), for the renders and rt_unshard.
inline bool resolve_tiles(const rt_render_params *p, RenderView &R, std::string &err) {
    if (p->width <= 0 || p->height <= 0 || p->samples <= 0) { err = "width, height and samples must be positive"; return false; }
    if ((int64_t)p->width * p->height >= 2147483647LL) { err = "image too large for the per-pixel seed (y*W+x must stay below 2^31-1)"; return false; }
    R.width = p->width; R.height = p->height; R.samples = p->samples;
    R.ray_depth = p->ray_depth > 0 ? p->ray_depth : 6;
    if (R.ray_depth > RT_MAX_DEPTH) { err = "ray_depth above RT_MAX_DEPTH (16)"; return false; }
    R.shard_count = p->shard_count > 1 ? p->shard_count : 1;
    R.shard_index = p->shard_count > 1 ? p->shard_index : 0;
    if (R.shard_index < 0 || R.shard_index >= R.shard_count) { err = "shard_index out of range"; return false; }
    if (R.shard_count > 1) {
        R.tile_w = p->tile_w > 0 ? p->tile_w : 32;
        R.tile_h = p->tile_h > 0 ? p->tile_h : 32;
        if ((R.tile_w & 7) || (R.tile_h & 7)) { err = "tile_w and tile_h must be multiples of 8"; return false; }
    } else {
        R.tile_w = R.tile_h = 8;
    }
    R.tiles_x = (R.width + R.tile_w - 1) / R.tile_w;
    R.tiles_y = (R.height + R.tile_h - 1) / R.tile_h;
    uint32_t total = (uint32_t)R.tiles_x * (uint32_t)R.tiles_y;
    R.n_shard_tiles = total > (uint32_t)R.shard_index ? (total - (uint32_t)R.shard_index + (uint32_t)R.shard_count - 1) / (uint32_t)R.shard_count : 0;
    return true;
}

// The part of the shard's tile `st` that lies inside the image: its corner and size in pixels.
inline void shard_tile_rect(const RenderView &R, uint32_t st, int &x0, int &y0, int &w, int &h) {
    const uint32_t gt = R.shard_count > 1 ? (uint32_t)R.shard_index + st * (uint32_t)R.shard_count : st;
    x0 = (int)(gt % (uint32_t)R.tiles_x) * R.tile_w; y0 = (int)(gt / (uint32_t)R.tiles_x) * R.tile_h;
    w = R.width - x0 < R.tile_w ? R.width - x0 : R.tile_w; h = R.height - y0 < R.tile_h ? R.height - y0 : R.tile_h;
}

} // namespace
} // namespace rtamd

struct rt_scene {
    int device = 0;
    rtamd::SceneView view{};
    rtamd::SceneView6 view6{};
    rtamd::SceneViewTxt viewt{};
    rtamd::SceneView5 view5{};
    bool txt_has_triangles = false; // TRIANGLE figures exist only in the hw5 grammar: such a scene renders with RT_INTEGRATOR_HW5 only
    int flavor = RT_INTEGRATOR_HW8; // which integrator this scene was prepared for
    bool hw6_lds_stack = false, hw6_pt_stack = false;
    uint32_t light_walk_depth = 0;   // hw8: depth of the tree the persistent kernel's light walker uses
    std::vector<void *> allocations;
    rt_scene_info info{};
    std::vector<uint32_t> light_order;
    uint32_t *d_work_counter = nullptr;
    unsigned long long *d_counters = nullptr; // CNT_SLOTS counters (rt_types.h CounterSlot)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    int n_cus = 256;
    // wavefront path state (grown on demand, reused across renders)
    rtamd::dev::WfView wf{};
    size_t wf_slots = 0, wf_levels = 0, wf_ctr_words = 0, wf_ovf_words = 0;
    int wf_pipes = 1;                // pipelines of the last wavefront render and the counter words of each
    size_t wf_ctr_block = 0;
    hipStream_t wf_streams[4] = {nullptr, nullptr, nullptr, nullptr}; // one per pipeline when a render uses more than one
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<void *> wf_allocs;
    float *d_partial = nullptr;      // throughput mode: per-stream pixel sums
    size_t partial_bytes = 0;
    std::vector<hipEvent_t> ev_pool; // brackets every launch of the dominant kernel when stats are requested
    unsigned long long *d_pt_debug = nullptr; // persistent pipeline: per workgroup {start, exit time, paths} (RTAMD_DEBUG_COUNTERS)
    void *pt_records = nullptr;      // persistent pipeline: path records of one pass
    uint32_t *pt_groups = nullptr;   // [cost per group | group_ofs (n_blocks + 1) | group_ids]: the re-deal between the phases of a frame
    size_t pt_record_bytes = 0, pt_group_bytes = 0;
    uint32_t pt_blocks = 0, pt_launches = 0;
    double pt_rebalance_ms = 0, pt_imbalance = 0;
    uint8_t *query_stage = nullptr;  // batched ray queries (rtamd_query.hip): the staging of one chunk, allocated by the first query
    size_t query_stage_bytes = 0;
    uint32_t *query_materials = nullptr; // material index by LOAD-order triangle, made by the first surface query (not part of info.device_bytes)
    uint8_t *path_stack = nullptr;   // rt_trace_paths: state and per-bounce stack of a chunk's paths, grown on demand (not part of info.device_bytes)
    size_t path_stack_bytes = 0;
    uint8_t *source_stage = nullptr; // rt_render_paths / rt_render_bake / rt_render_probes: the slots' state (probes: with their accumulators) and, with host arrays, the staging of one chunk (not part of info.device_bytes)
    size_t source_stage_bytes = 0;
    uint8_t *denoise_stage = nullptr; // preview filter (rtamd_denoise.hip): the working set of one frame, grown on demand (not part of info.device_bytes)
    size_t denoise_stage_bytes = 0;
    void free_wf() {
        for (void *p : wf_allocs) (void)hipFree(p);
        wf_allocs.clear();
        wf = rtamd::dev::WfView{};
        wf_slots = wf_levels = wf_ctr_words = wf_ovf_words = 0;
    }
    ~rt_scene() {
        free_wf();
        if (d_partial) (void)hipFree(d_partial);
        if (pt_records) (void)hipFree(pt_records);
        if (pt_groups) (void)hipFree(pt_groups);
        if (d_pt_debug) (void)hipFree(d_pt_debug);
        if (query_stage) (void)hipFree(query_stage);
        if (query_materials) (void)hipFree(query_materials);
        if (path_stack) (void)hipFree(path_stack);
        if (source_stage) (void)hipFree(source_stage);
        if (denoise_stage) (void)hipFree(denoise_stage);
        for (void *p : allocations) (void)hipFree(p);
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_stop) (void)hipEventDestroy(ev_stop);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (int h = 0; h < 4; h++) { if (wf_streams[h]) (void)hipStreamDestroy(wf_streams[h]); if (ev_join[h]) (void)hipEventDestroy(ev_join[h]); }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
    }
};

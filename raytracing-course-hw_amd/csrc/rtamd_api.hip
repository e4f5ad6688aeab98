// C-ABI of the render path (include/rtamd.h): every kernel that renders, the launch drivers, the statistics and the resumable renders.
// Scene creation and the file front-end are in rtamd_scene.hip.
// No CPU fallback exists: every entry point that needs the GPU fails with RT_ERR_NO_DEVICE / RT_ERR_HIP
// when HIP is unusable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "host/knobs.h"
#include "host/rt_scene.h"
#include "host/rt_accum_state.h"
#include "device/rt_kernels_hw8.h"
#include "device/rt_wavefront.h"
#include "device/rt_query.h"
#include "device/rt_query_surface.h"
#include "device/rt_query_scatter.h"
#include "device/rt_bake.h"
#include "device/rt_persistent.h"
#include "device/rt_adaptive.h"
#include "device/rt_views.h"
#include "device/rt_view_adaptive.h"
#include "device/rt_kernels_hw6.h"
#include "device/rt_persistent_hw6.h"
#include "device/rt_kernels_txt.h"
#include "device/rt_kernels_hw2.h"
#include "device/rt_kernels_hw4.h"
#include "device/rt_kernels_hw5.h"

using namespace rtamd;

extern "C" {

int rt_abi_version(void) { return RTAMD_ABI_VERSION; }

size_t rt_output_elems(const rt_render_params *p) {
    if (!p) return 0;
    size_t elems = 0; // what a refusal answers, without a message
    guarded("rt_output_elems: ", [&]() -> int {
        RenderView R{};
        std::string err;
        if (resolve_tiles(p, R, err)) elems = R.shard_count > 1 ? (size_t)R.n_shard_tiles * R.tile_w * R.tile_h * 3 : (size_t)R.width * R.height * 3;
        return RT_OK;
    });
    return elems;
}

// Rounds a pixel needs per camera sample: one per bounce; without the deepest-level shortcut the last bounce's pdf / clamp
// step takes one more.
static size_t wavefront_rounds(const SceneView &V, const RenderView &R) {
    return (size_t)(R.samples - R.sample_first) * ((size_t)R.ray_depth + (V.last_level_emission_only ? 0u : 1u));
}

// Wavefront driver: per round one traverse launch and one shade launch (device/rt_wavefront.h).
// No host synchronisation inside: queue lengths live in device memory, one counter block per round.
// RTAMD_WF_PIPELINES=n (experiment, default 1): cut the frame into n independent pipelines (disjoint path slots, own queues and
// counters), each a chain traverse -> shade -> traverse ... on its own stream, so that one pipeline's kernels could fill the CUs
// another leaves idle in the tail of a launch.  Pixels do not depend on the cut (paths never interact; tests force n = 2..4).
// Measured on the benchmark frame: 2 pipelines 281, 3 pipelines 258 against 304 Msamples/s with one -- the halved queues lose
// more to ramp-up and drain than the overlap returns -- so one pipeline stays the default.
#define WF_MAX_PIPES 4
static int wavefront_pipelines(uint32_t n_work) {
    const int v = env_int("RTAMD_WF_PIPELINES", 1);
    int p = v >= 1 && v <= WF_MAX_PIPES ? v : 1;
    while (p > 1 && n_work < (uint32_t)p) p--;
    return p;
}

// RTAMD_WF_SPLIT=a:b replaces the cost weights closest-hit : light query (the round pipeline's block split, the hw8 persistent kernel's
// choice of role); anything but two numbers in 1..255 leaves them alone.
static void env_cost_split(int &cost_t, int &cost_l) {
    int a = 0, b = 0;
    if (const char *e = env_str("RTAMD_WF_SPLIT")) if (sscanf(e, "%d:%d", &a, &b) == 2 && a > 0 && b > 0 && a < 256 && b < 256) { cost_t = a; cost_l = b; }
}

static void launch_wavefront(rt_scene *scene, const SceneView &V, const RenderView &R, uint32_t n_work, hipStream_t stream, bool count, bool time_trace) {
    const size_t n_slots = (size_t)n_work * 64;
    const size_t rounds = wavefront_rounds(V, R);
    const int pipes = wavefront_pipelines(n_work);
    const size_t ctr_block = (rounds + 2) * WF_CTR; // words per pipeline
    if (scene->wf_slots < n_slots || scene->wf_levels < (size_t)R.ray_depth || scene->wf_ctr_words < ctr_block * pipes) {
        scene->free_wf();
        auto alloc = [&](size_t bytes) { void *p = nullptr; HIP_CHECK(hipMalloc(&p, bytes)); scene->wf_allocs.push_back(p); return p; };
        scene->wf.r0 = (float4 *)alloc(n_slots * (16 * WF_REC_BASE + 32 * (size_t)R.ray_depth));
        scene->wf.q_trace[0] = (uint32_t *)alloc(n_slots * 4);
        scene->wf.q_trace[1] = (uint32_t *)alloc(n_slots * 4);
        scene->wf.q_light = (uint32_t *)alloc(n_slots * 4);
        scene->wf.ctr = (uint32_t *)alloc(ctr_block * WF_MAX_PIPES * 4);
        scene->wf.q_slow = (uint32_t *)alloc(n_slots * 4);
        scene->wf_slots = n_slots; scene->wf_levels = (size_t)R.ray_depth; scene->wf_ctr_words = ctr_block * WF_MAX_PIPES;
    }
    scene->wf_pipes = pipes; scene->wf_ctr_block = ctr_block;
    // Trees deeper than the LDS stacks use the SPILL kernel variant (bounds-checked stack with a global overflow area).
    // RTAMD_WF_LDS_STACK=n (testing): pretend the LDS stacks hold only n entries, which forces the SPILL variant and its overflow area.
    int lds_limit = env_int("RTAMD_WF_LDS_STACK", WF_STACK);
    if (lds_limit < 1 || lds_limit >= WF_STACK) lds_limit = WF_STACK;
    const bool spill = scene->info.bvh_depth > (uint32_t)lds_limit || scene->info.light_bvh_depth > (uint32_t)lds_limit;
    const size_t ovf_block = (size_t)scene->n_cus * 8u * 256u * WF_OVF; // words per pipeline: up to 8 persistent blocks per CU
    if (spill && scene->wf_ovf_words < ovf_block * pipes) {
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, ovf_block * pipes * 4u));
        scene->wf_allocs.push_back(p); // a smaller earlier area stays allocated until free_wf()
        scene->wf.ovf = (uint32_t *)p;
        scene->wf_ovf_words = ovf_block * pipes;
    }
    HIP_CHECK(hipMemsetAsync(scene->wf.ctr, 0, ctr_block * pipes * 4, stream));
    uint32_t blocks_per_cu = (uint32_t)env_int("RTAMD_WF_BLOCKS_PER_CU", 5);  // 5 x 30 KB of stacks fit the 160 KB LDS (which is handed out in 1280-byte granules: 32 KB blocks fit only 4 times)
    if (blocks_per_cu == 0u) blocks_per_cu = 5u;
    if (blocks_per_cu > 8u) blocks_per_cu = 8u;                               // a negative value ends here too
    const uint32_t persistent_blocks = (uint32_t)scene->n_cus * blocks_per_cu;
    int dyn256 = std::min(255, std::max(0, env_int("RTAMD_WF_DYNAMIC_256", 64))); // share of each queue (of 256) handed out dynamically at the tail
    if (env_flag("RTAMD_WF_STEAL_CHUNK")) dyn256 |= (env_positive("RTAMD_WF_STEAL_CHUNK", 64) & 255) << 8; // tuning: items per dynamic chunk (default 64)
    int split_a = 7, split_b = 8; // cost weights closest-hit : light query for the block split (two sweeps: 7:8 is ~1 % ahead of 1:1 and 8:7)
    env_cost_split(split_a, split_b);
    dyn256 |= (split_a << 16) | (split_b << 24);
    // leaf batch: lanes waiting at a leaf start their triangle tests when 20 of them wait -- or, in a thinly populated wave, a share
    // of the active lanes (RTAMD_WF_LEAF_SHARE_256, default 112/256; sweep: tools/tuning/sweep_leaf_share.sh); packed as batch | share << 16
    const int leaf_share = env_positive("RTAMD_WF_LEAF_SHARE_256", 112) & 0x7fff;
    const int t_refill = env_positive("RTAMD_TRACE_REFILL", WF_REFILL), t_batch = (env_positive("RTAMD_TRACE_LEAF_BATCH", WF_LEAF_BATCH) & 255) | (leaf_share << 16);
    const int l_refill = env_positive("RTAMD_LIGHT_REFILL", WF_REFILL), l_batch = (env_positive("RTAMD_LIGHT_LEAF_BATCH", WF_LEAF_BATCH) & 255) | (leaf_share << 16);
    const uint32_t shade_per_cu = (uint32_t)env_positive("RTAMD_WF_SHADE_BLOCKS_PER_CU", 16); // grid cap of wf_shade_kernel (grid-stride beyond it)
    unsigned long long *ctrs = count ? scene->d_counters : nullptr;
    if (time_trace) while (scene->ev_pool.size() < 2 * rounds * pipes) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); scene->ev_pool.push_back(e); }

    // the pipelines: contiguous ranges of 64-slot groups, the state arrays offset accordingly
    dev::WfView Wp[WF_MAX_PIPES];
    hipStream_t sp[WF_MAX_PIPES];
    uint32_t shade_blocks[WF_MAX_PIPES];
    if (pipes > 1 && !scene->wf_streams[0]) {
        for (int h = 0; h < WF_MAX_PIPES; h++) {
            HIP_CHECK(hipStreamCreateWithFlags(&scene->wf_streams[h], hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&scene->ev_join[h], hipEventDisableTiming));
        }
        HIP_CHECK(hipEventCreateWithFlags(&scene->ev_fork, hipEventDisableTiming));
    }
    const uint32_t stride = (uint32_t)WF_REC_BASE + 2u * (uint32_t)scene->wf_levels; // float4 per slot (the allocation's depth, >= this render's)
    uint32_t first = 0;
    for (int h = 0; h < pipes; h++) {
        const uint32_t groups = n_work / (uint32_t)pipes + ((uint32_t)h < n_work % (uint32_t)pipes ? 1u : 0u);
        const size_t base = (size_t)first * 64;
        dev::WfView W = scene->wf;
        W.stride = stride;
        W.r0 += base * stride;
        W.q_trace[0] += base; W.q_trace[1] += base; W.q_light += base; W.q_slow += base;
        W.ctr += (size_t)h * ctr_block;
        if (W.ovf) W.ovf += (size_t)h * ovf_block;
        W.n_slots = groups * 64u;
        W.slot_base = (uint32_t)base;
        Wp[h] = W;
        sp[h] = pipes > 1 ? scene->wf_streams[h] : stream;
        shade_blocks[h] = (W.n_slots + 255u) / 256u;
        if (shade_blocks[h] > (uint32_t)scene->n_cus * shade_per_cu) shade_blocks[h] = (uint32_t)scene->n_cus * shade_per_cu;
        first += groups;
    }
    if (pipes > 1) {
        HIP_CHECK(hipEventRecord(scene->ev_fork, stream));
        for (int h = 0; h < pipes; h++) HIP_CHECK(hipStreamWaitEvent(sp[h], scene->ev_fork, 0));
    }
    for (int h = 0; h < pipes; h++)
        hipLaunchKernelGGL(dev::wf_init_kernel, dim3((Wp[h].n_slots + 255u) / 256u), dim3(256), 0, sp[h], V, R, Wp[h]);
    const dim3 pb(persistent_blocks), tb(256);
    for (uint32_t r = 0; r < (uint32_t)rounds; r++) {
        for (int h = 0; h < pipes; h++) {
            const dev::WfView &W = Wp[h];
            hipStream_t st = sp[h];
            if (time_trace) HIP_CHECK(hipEventRecord(scene->ev_pool[2 * ((size_t)r * pipes + h)], st));
            if (spill) {
                if (count) hipLaunchKernelGGL((dev::wf_traverse_kernel<true, true>), pb, tb, 0, st, V, W, r, ctrs, t_refill, t_batch, l_refill, l_batch, dyn256, lds_limit);
                else hipLaunchKernelGGL((dev::wf_traverse_kernel<false, true>), pb, tb, 0, st, V, W, r, ctrs, t_refill, t_batch, l_refill, l_batch, dyn256, lds_limit);
            } else {
                if (count) hipLaunchKernelGGL((dev::wf_traverse_kernel<true, false>), pb, tb, 0, st, V, W, r, ctrs, t_refill, t_batch, l_refill, l_batch, dyn256, lds_limit);
                else hipLaunchKernelGGL((dev::wf_traverse_kernel<false, false>), pb, tb, 0, st, V, W, r, ctrs, t_refill, t_batch, l_refill, l_batch, dyn256, lds_limit);
            }
            if (time_trace) HIP_CHECK(hipEventRecord(scene->ev_pool[2 * ((size_t)r * pipes + h) + 1], st));
            if (!spill && V.n_lights) hipLaunchKernelGGL(dev::wf_light_exact_kernel, dim3((unsigned)scene->n_cus), dim3(64), 0, st, V, W, r);
            hipLaunchKernelGGL(dev::wf_shade_kernel, dim3(shade_blocks[h]), dim3(256), 0, st, V, R, W, r, ctrs);
            if (V.exact_boxes) hipLaunchKernelGGL(dev::wf_trace_exact_kernel, dim3((unsigned)scene->n_cus), dim3(64), 0, st, V, R, W, r, ctrs); // hits at a box boundary (~1e-5 of the paths)
        }
    }
    HIP_CHECK(hipGetLastError());
    if (pipes > 1)
        for (int h = 0; h < pipes; h++) {
            HIP_CHECK(hipEventRecord(scene->ev_join[h], sp[h]));
            HIP_CHECK(hipStreamWaitEvent(stream, scene->ev_join[h], 0));
        }
}

// Sample counts at which the launches of a persistent render stop (the last one = the frame).  Two phases: 1/16 of the samples under the
// round-robin deal, the rest after the re-deal.  RTAMD_PT_PHASES=3 deals the last quarter of the remaining samples once more, from the
// costs measured over the long middle phase — measured: no gain (hw6 practice6_2 191.7 vs 193.6 Msamples/s, headline 284.2 vs 284.6):
// what remains of the spread of the workgroups' exit times after one re-deal is not the amount of work but the serial samples of the
// slowest pixels.
static std::vector<int> phase_stops(bool rebalance, int phase0, int samples, bool small_population) {
    std::vector<int> stops;
    const char *explicit_stops = env_str("RTAMD_PT_STOPS"); // experiment: explicit sample counts at which the frame is re-dealt, e.g. "2,16"
    if (rebalance && explicit_stops) {
        int last = 0;
        for (const char *c = explicit_stops; *c;) {
            const int v = atoi(c);
            if (v > last && v < samples) { stops.push_back(v); last = v; }
            while (*c && *c != ',') c++;
            if (*c == ',') c++;
        }
        stops.push_back(samples);
        return stops;
    }
    if (rebalance) {
        // small populations (the deal is in quarter sub-tiles): a first re-deal after two samples already — the round-robin deal of the
        // first phase is the costly one there (slowest workgroup / mean 1.8 on hw6's 1024x1024 frame) — then the usual one
        if (small_population && phase0 > 2 && !env_flag("RTAMD_PT_PHASE0")) stops.push_back(2);
        stops.push_back(phase0);
        const int want = env_int("RTAMD_PT_PHASES", 2);
        const int mid = phase0 + (samples - phase0) * 3 / 4;
        if (want >= 3 && samples >= 64 && mid > phase0 && mid < samples) stops.push_back(mid);
    }
    stops.push_back(samples);
    return stops;
}

// Between the phases of a persistent render: read what every 8x8 sub-tile cost in the phase that just ended (PT_COST_*, rt_persistent.h)
// and how long every workgroup ran, and deal the sub-tiles again — longest processing time first onto the workgroup that would be done
// with it soonest (at most groups_per_block each); the lists go to d_ofs / d_ids for the next launch.
// Workgroups are not equally fast.  The five that share a CU are served oldest wave first, so at equal load they leave staggered
// (measured on the 1080p frame: 1,278 / 1,328 / 1,384 / 1,447 / 1,526 ms by launch order), and from the first exit on the CU runs with four
// waves per SIMD, then three ...  So the deal is by speed: speed(b) = (cost of the sub-tiles b owned) / (its run time) in the phase that
// just ended, and a sub-tile goes to the workgroup with the smallest load / speed.  `owner` (sub-tile -> workgroup of the phase that
// just ended; empty = the kernel's round-robin deal) is updated to the new deal.  d_times: per workgroup {start, exit, -} in 100 MHz
// ticks (PtParams::debug), nullable.  gamma_round / gamma_own: the kernel's speed model (below).
static void redeal_groups(rt_scene *scene, const uint32_t *d_cost, uint32_t *d_ofs, uint32_t *d_ids, uint32_t groups, uint32_t blocks, uint32_t groups_per_block,
                          double gamma_round, double gamma_own, hipStream_t stream, const unsigned long long *d_times, std::vector<uint32_t> *owner) {
    std::vector<uint32_t> cost(groups), ofs, ids, order(groups);
    HIP_CHECK(hipStreamSynchronize(stream));
    const double t0 = now_ms();
    HIP_CHECK(hipMemcpy(cost.data(), d_cost, (size_t)groups * 4, hipMemcpyDeviceToHost));
    std::vector<double> slowness(blocks, 1.0); // time per unit of cost, relative to the mean
    if (d_times && owner && !env_flag("RTAMD_PT_NO_SPEEDS")) {
        std::vector<unsigned long long> times((size_t)blocks * 3);
        HIP_CHECK(hipMemcpy(times.data(), d_times, times.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<double> had(blocks, 0.0);
        for (uint32_t g = 0; g < groups; g++) had[owner->empty() ? g % blocks : (*owner)[g]] += (double)cost[g] + 1.0;
        double sum = 0; uint32_t n = 0;
        for (uint32_t b = 0; b < blocks; b++) {
            const double dur = times[3 * b + 1] > times[3 * b] ? (double)(times[3 * b + 1] - times[3 * b]) : 0.0;
            slowness[b] = dur > 0 && had[b] > 0 ? dur / had[b] : 0.0;
            if (slowness[b] > 0) { sum += slowness[b]; n++; }
        }
        const double mean = n ? sum / n : 1.0;
        // The workgroups are dispatched in index order, one round of n_cus after the other, so the age rank of a workgroup on its CU is
        // its index / n_cus.  The measured slowness is split into the mean of the workgroup's round (the age effect: over-relaxed,
        // because a slow workgroup ran its last stretch with its faster neighbours already gone, so the phase shows less of a
        // difference than an even finish will: 2.0 measured best for the hw8 kernel on the 1080p frame — its youngest workgroups
        // still left last at 1.5 (exit times by dispatch round 1,028 / 1,024 / 1,035 / 1,071 / 1,118 ms) — and 1.5 for the hw6 kernel) and the
        // workgroup's own deviation from it (most of which is gone in the next phase: damped).
        gamma_round = env_float("RTAMD_PT_SPEED_GAMMA", gamma_round);
        gamma_own = env_float("RTAMD_PT_SPEED_GAMMA_OWN", gamma_own);
        const uint32_t round_size = scene->n_cus > 0 && blocks % (uint32_t)scene->n_cus == 0 ? (uint32_t)scene->n_cus : blocks;
        for (uint32_t r0 = 0; r0 < blocks; r0 += round_size) {
            double lsum = 0; uint32_t ln = 0;
            for (uint32_t b = r0; b < r0 + round_size; b++) if (slowness[b] > 0) { lsum += log(slowness[b] / mean); ln++; }
            const double lround = ln ? lsum / ln : 0.0;
            for (uint32_t b = r0; b < r0 + round_size; b++) {
                const double s = slowness[b] > 0 ? exp(gamma_round * lround + gamma_own * (log(slowness[b] / mean) - lround)) : exp(gamma_round * lround);
                slowness[b] = s < 0.5 ? 0.5 : (s > 2.0 ? 2.0 : s); // a workgroup with almost nothing to do says little about its speed
            }
        }
    }
    for (uint32_t g = 0; g < groups; g++) order[g] = g;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] != cost[b] ? cost[a] > cost[b] : a < b; });
    std::vector<std::pair<double, uint32_t>> heap; // (time at which the block is done with what it holds, block), min-heap
    heap.reserve(blocks);
    for (uint32_t b = 0; b < blocks; b++) heap.push_back({0.0, b});
    auto cmp = [](const std::pair<double, uint32_t> &a, const std::pair<double, uint32_t> &b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    std::vector<std::vector<uint32_t>> mine(blocks);
    uint64_t total = 0, before_max = 0;
    { std::vector<uint64_t> rr(blocks, 0); for (uint32_t g = 0; g < groups; g++) { rr[g % blocks] += cost[g]; total += cost[g]; } for (uint64_t v : rr) before_max = v > before_max ? v : before_max; }
    for (uint32_t g : order) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        auto &top = heap.back();
        mine[top.second].push_back(g);
        top.first += ((double)cost[g] + 1.0) * slowness[top.second]; // + 1: empty sub-tiles (padding) are spread evenly too
        if (mine[top.second].size() >= groups_per_block) heap.pop_back(); // full: out of the deal
        else std::push_heap(heap.begin(), heap.end(), cmp);
    }
    ofs.assign(blocks + 1, 0);
    if (owner) owner->assign(groups, 0);
    const bool by_cost = !env_flag("RTAMD_PT_NO_FRONT_FIRST"); // most expensive group first: the kernel's queues serve the front of the list first (PtParams::front_first)
    for (uint32_t b = 0; b < blocks; b++) {
        if (by_cost) std::sort(mine[b].begin(), mine[b].end(), [&](uint32_t x, uint32_t y) { return cost[x] != cost[y] ? cost[x] > cost[y] : x < y; });
        else std::sort(mine[b].begin(), mine[b].end());
        ofs[b] = (uint32_t)ids.size();
        ids.insert(ids.end(), mine[b].begin(), mine[b].end());
        if (owner) for (uint32_t g : mine[b]) (*owner)[g] = b;
    }
    ofs[blocks] = (uint32_t)ids.size();
    if (const char *dump = env_str("RTAMD_DUMP_DEAL")) { // diagnostic: what the re-deal gave every workgroup (tools/tuning/wg_balance.py)
        if (FILE *f = fopen(dump, "w")) {
            for (uint32_t b = 0; b < blocks; b++) {
                uint64_t load = 0;
                for (uint32_t g : mine[b]) load += cost[g];
                fprintf(f, "%u %zu %llu %.4f\n", b, mine[b].size(), (unsigned long long)load, slowness[b]);
            }
            fclose(f);
        }
    }
    HIP_CHECK(hipMemcpyAsync(d_ofs, ofs.data(), ofs.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream)); // the vectors go out of scope
    scene->pt_rebalance_ms += now_ms() - t0;
    if (total) scene->pt_imbalance = (double)before_max * blocks / (double)total; // slowest workgroup / mean under the round-robin deal
}

// Persistent dataflow driver (hw8 / hw7: device/rt_persistent.h, hw6: device/rt_persistent_hw6.h): ONE launch renders up to
// n_cus x per_cu x max_paths path slots; larger frames (or throughput mode with many streams) take several passes over disjoint slot
// ranges, each a complete render of its pixels.
//
// Load balance.  A workgroup owns its pixels for a whole launch, and pixels differ in cost (sky: one query per sample, a glossy
// interior: up to 2 x depth), so with the plain round-robin deal of the 8x8 sub-tiles the slowest workgroup ends 3 % (1080p on
// one GPU) to 12 % (a shard of 8) behind the mean.  A frame of >= 16 samples is therefore rendered in two phases: the first
// 1/16 of the samples with the round-robin deal while every workgroup counts the hits it shades per sub-tile, then the host
// re-deals the sub-tiles (longest processing time first onto the least loaded workgroup) and the second launch resumes every
// pixel from its record (pixel sum, random stream and the parked camera ray are all there; pixels do not depend on the deal).
// For hw6 the cost of a pixel spans 1 to 63 walks per sample (a wall against the glass bunny), so the deal matters far more.
// Every launch is bracketed by events when `time_trace` (ev_pool[2k], ev_pool[2k+1]).
//
// What the two kernels do not share is their PersistentKernel.
struct PersistentKernel {
    uint32_t max_paths;               // paths per workgroup (its LDS bitmap)
    int per_cu;                       // workgroups per CU
    int stack;                        // entries of a walker's stack column (P8_STACK, P6_STACK)
    size_t record_bytes;              // path record per slot
    int cost_t, cost_l;               // PtParams::cost_t / cost_l
    bool hw8_knobs;                   // RTAMD_WF_SPLIT, RTAMD_PT_PRIO and the RTAMD_TRACE_PIXEL dump apply
    double gamma_round, gamma_own;    // the re-deal's speed model (redeal_groups)
    // one launch of `blocks` workgroups over the path slots [slot_base, slot_base + n_slots) of `records`
    std::function<void(uint32_t blocks, const RenderView &R, const dev::PtParams &P, float4 *records, uint32_t slot_base, uint32_t n_slots)> launch;
};

static PersistentKernel hw8_persistent(const SceneView &V, int ray_depth, hipStream_t stream, bool count) {
    const uint32_t stride = (uint32_t)WF_REC_BASE + 2u * (uint32_t)ray_depth; // float4 per slot
    // kernel variant by the features this render can reach (fewer features, fewer spilled registers): the hw7 integrator has no
    // environment map; an hw8 render needs the environment lookup only when the scene has a map
    const int feat = V.hw7 ? WF_FEAT_HW7 : (V.env_image >= 0 ? WF_FEAT_ENV : 0);
    return {PT_MAX_PATHS, P8_PER_CU, P8_STACK, 16u * stride, 7, 8, true, 2.0, 0.3,
            [=, &V](uint32_t blocks, const RenderView &R, const dev::PtParams &P, float4 *records, uint32_t slot_base, uint32_t n_slots) {
                dev::WfView W{};
                W.r0 = records; W.stride = stride; W.n_slots = n_slots; W.slot_base = slot_base;
                const dim3 grid(blocks), block(P8_THREADS);
                if (R.src_mode == PT_SRC_VIEWS) { // a batch of cameras (rt_views_*): the source kernel compiled for them (WF_FEAT_VIEWS)
                    if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_VIEWS | WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_VIEWS>), grid, block, 0, stream, V, R, W, P);
                } else if (R.src_mode == PT_SRC_PIXELS) { // the pixels of another frame (rt_adaptive_*): the source kernel compiled for them (WF_FEAT_PIXELS)
                    if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_PIXELS | WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_PIXELS>), grid, block, 0, stream, V, R, W, P);
                } else if (R.src_mode == PT_SRC_PROBES) { // SH9 probes: the source kernel compiled with the side arrays (WF_FEAT_PROBES)
                    if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_PROBES | WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_PROBES>), grid, block, 0, stream, V, R, W, P);
                } else if (R.src_mode) { // a path source (device/rt_path_source.h; source_render below): hw8 only, no counting variant
                    if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE | WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_SOURCE>), grid, block, 0, stream, V, R, W, P);
                } else if (count) {
                    if (feat == WF_FEAT_HW7) hipLaunchKernelGGL((dev::pt_persistent_kernel<true, WF_FEAT_HW7>), grid, block, 0, stream, V, R, W, P);
                    else if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<true, WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<true, 0>), grid, block, 0, stream, V, R, W, P);
                } else {
                    if (feat == WF_FEAT_HW7) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_HW7>), grid, block, 0, stream, V, R, W, P);
                    else if (feat == WF_FEAT_ENV) hipLaunchKernelGGL((dev::pt_persistent_kernel<false, WF_FEAT_ENV>), grid, block, 0, stream, V, R, W, P);
                    else hipLaunchKernelGGL((dev::pt_persistent_kernel<false, 0>), grid, block, 0, stream, V, R, W, P);
                }
            }};
}

static PersistentKernel hw6_persistent(const SceneView6 &V, hipStream_t stream, bool count) {
    return {P6_MAX_PATHS, P6_PER_CU, P6_STACK, (size_t)P6_REC * sizeof(float4), 1, 1, false, 1.5, 0.4, // the record holds the path's frames
            [=, &V](uint32_t blocks, const RenderView &R, const dev::PtParams &P, float4 *records, uint32_t slot_base, uint32_t) {
                const dev::W6View W{records, slot_base};
                if (count) hipLaunchKernelGGL(dev::p6_persistent_kernel<true>, dim3(blocks), dim3(P6_THREADS), 0, stream, V, R, W, P);
                else hipLaunchKernelGGL(dev::p6_persistent_kernel<false>, dim3(blocks), dim3(P6_THREADS), 0, stream, V, R, W, P);
            }};
}

static void launch_persistent(rt_scene *scene, const PersistentKernel &k, const RenderView &R, uint32_t n_work, hipStream_t stream, bool count, bool time_trace) {
    const int n_samples = R.samples - R.sample_first; // of this launch sequence: a frame, or one slice of a resumable render (sample_first > 0)
    const uint32_t n_blocks_max = (uint32_t)env_positive("RTAMD_PT_BLOCKS", scene->n_cus * k.per_cu); // five 4-wave workgroups per CU (their LDS fills the CU)
    const uint64_t pass_cap = (uint64_t)n_blocks_max * (k.max_paths / 64);
    const uint32_t passes = (uint32_t)((n_work + pass_cap - 1) / pass_cap);
    const uint32_t pass_groups = (n_work + passes - 1) / passes;         // 8x8 sub-tiles (64 path slots) per pass
    // The unit of the deal: an 8x8 sub-tile, or — when a workgroup would hold fewer than sixteen of those (small frames, shards) — a
    // quarter of one (two pixel rows): a single heavy sub-tile must not outweigh a workgroup's fair share, and a workgroup whose load
    // is a few heavy pixels is bound by their serial samples.
    uint32_t group_shift = (uint64_t)pass_groups < 16ull * n_blocks_max ? 4u : 6u;
    if (const int v = env_int("RTAMD_PT_GROUP_SHIFT", 0); v == 4 || v == 5 || v == 6) group_shift = (uint32_t)v;
    const uint32_t sub = 6u - group_shift, groups_per_block = k.max_paths >> group_shift;
    grow(scene->pt_records, scene->pt_record_bytes, (size_t)pass_groups * 64 * k.record_bytes);
    grow(scene->pt_groups, scene->pt_group_bytes, (2 * ((size_t)pass_groups << sub) + n_blocks_max + 1) * 4);
    uint32_t *d_cost = scene->pt_groups, *d_ofs = d_cost + ((size_t)pass_groups << sub), *d_ids = d_ofs + n_blocks_max + 1;
    dev::PtParams P{};
    const int leaf_share = env_positive("RTAMD_WF_LEAF_SHARE_256", 112) & 0x7fff;
    P.refill = env_positive("RTAMD_TRACE_REFILL", WF_REFILL) | (env_positive("RTAMD_LIGHT_REFILL", env_positive("RTAMD_TRACE_REFILL", WF_REFILL)) << 16);
    P.leaf_batch = (env_positive("RTAMD_TRACE_LEAF_BATCH", 28) & 255) | (leaf_share << 16); // lanes that hold two leaves (or have nothing else left) before a leaf phase starts
    // RTAMD_PT_STACK_CAP=n (test knob): the walkers' columns count as full beyond n entries, so that a small scene reaches the endings of a
    // full column (the exact role redoes those queries: same pixels).  Counting launches only: the plain kernels hold the cap as an immediate.
    P.stack_cap = k.stack;
    if (const int v = env_int("RTAMD_PT_STACK_CAP", 0); count && v >= 1 && v < k.stack) P.stack_cap = v;
    P.shade_min = 0; // set per pass below
    P.shade_thr0 = env_positive("RTAMD_PT_SHADE_THR0", 128);
    P.shade_thr_step = env_positive("RTAMD_PT_SHADE_STEP", 512);
    P.cost_t = k.cost_t; P.cost_l = k.cost_l;
    if (k.hw8_knobs) {
        env_cost_split(P.cost_t, P.cost_l);
        P.prio = env_int("RTAMD_PT_PRIO", 0);
    }
    P.counters = scene->d_counters;
    // A wave still in the launch after this long gives up (the kernel cannot hang the GPU): RTAMD_PT_TIMEOUT_S, by default ten minutes or
    // — for long renders: 4K at thousands of samples — the time the launch would take at a twentieth of the usual rate, whichever is more.
    {
        const double expected_s = (double)n_work * 64.0 * (double)n_samples / 15e6;
        const double deadline_s = env_flag("RTAMD_PT_TIMEOUT_S") ? (double)env_positive("RTAMD_PT_TIMEOUT_S", 600) : (expected_s > 600.0 ? expected_s : 600.0);
        P.deadline_ticks = (unsigned long long)(deadline_s * 1e8);
    }
    // every workgroup leaves its start and exit time (the re-deal measures the workgroups' speeds with them)
    if (!scene->d_pt_debug) HIP_CHECK(hipMalloc((void **)&scene->d_pt_debug, (size_t)PT_DEBUG_BLOCKS * 3 * sizeof(unsigned long long)));
    if (n_blocks_max <= PT_DEBUG_BLOCKS) P.debug = scene->d_pt_debug;
    float4 *d_trace = nullptr;
    const uint32_t trace_cap = 1u << 16;
    if (k.hw8_knobs && count && env_str("RTAMD_TRACE_PIXEL") && env_str("RTAMD_TRACE_OUT")) { // diagnostic: tests/diagnostics/trace_pixel.py
        int tx = 0, ty = 0;
        if (sscanf(env_str("RTAMD_TRACE_PIXEL"), "%d,%d", &tx, &ty) == 2) {
            HIP_CHECK(hipMalloc((void **)&d_trace, (size_t)trace_cap * sizeof(float4)));
            HIP_CHECK(hipMemsetAsync(d_trace, 0, sizeof(float4), stream));
            P.trace_buf = d_trace; P.trace_cap = trace_cap; P.trace_pixel = ty * R.width + tx;
        }
    }
    // two phases when there is something to re-deal: enough samples, and several sub-tiles per workgroup
    const int phase0 = env_int("RTAMD_PT_PHASE0", n_samples / 16);
    const bool two_phase = !env_flag("RTAMD_PT_NO_REBALANCE") && phase0 >= 1 && phase0 < n_samples && ((uint64_t)pass_groups << sub) >= 4ull * n_blocks_max;
    std::vector<int> stops = phase_stops(two_phase, phase0, n_samples, group_shift < 6u);
    for (int &stop : stops) stop += R.sample_first; // the records count a pixel's samples from the start of its frame
    const uint32_t phases = (uint32_t)stops.size();
    if (time_trace) while (scene->ev_pool.size() < 2 * (size_t)passes * phases) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); scene->ev_pool.push_back(e); }
    uint32_t first = 0, launch = 0;
    scene->pt_blocks = 0; scene->pt_rebalance_ms = 0; scene->pt_imbalance = 0;
    std::vector<uint32_t> owner; // sub-tile -> workgroup of the phase in flight
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t groups = n_work - first < pass_groups ? n_work - first : pass_groups;
        const uint32_t n_units = groups << sub;   // groups of the deal
        P.n_groups = n_units; P.group_shift = group_shift;
        const uint32_t blocks = n_units < n_blocks_max ? n_units : n_blocks_max;
        if (blocks > scene->pt_blocks) scene->pt_blocks = blocks;
        // a wave turns shader when this many paths wait: a pool of a few hundred paths cannot let its paths wait for a full wave of them
        // (measured: 1,620 paths per workgroup 32 > 64 > 16; 820 and 200 paths per workgroup 16 > 32 > 64)
        P.shade_min = env_positive("RTAMD_PT_SHADE_MIN", ((uint64_t)groups * 64u) / blocks >= 1536u ? 32 : 16);
        for (uint32_t ph = 0; ph < phases; ph++) {
            RenderView Rp = R;
            Rp.sample_stop = stops[ph];
            P.resume = ph ? 1u : 0u;
            P.group_cost = ph + 1 < phases ? d_cost : nullptr;   // every phase but the last measures for the next re-deal
            P.group_ofs = ph ? d_ofs : nullptr;
            P.group_ids = ph ? d_ids : nullptr;
            P.front_first = ph && !env_flag("RTAMD_PT_NO_FRONT_FIRST") ? 1u : 0u;
            if (ph == 0) owner.clear(); // the kernel's round-robin deal
            if (ph >= 1) redeal_groups(scene, d_cost, d_ofs, d_ids, n_units, blocks, groups_per_block, k.gamma_round, k.gamma_own, stream, P.debug, &owner);
            if (P.debug) HIP_CHECK(hipMemsetAsync(scene->d_pt_debug, 0, (size_t)PT_DEBUG_BLOCKS * 3 * sizeof(unsigned long long), stream));
            if (time_trace) HIP_CHECK(hipEventRecord(scene->ev_pool[2 * launch], stream));
            k.launch(blocks, Rp, P, (float4 *)scene->pt_records, first * 64u, groups * 64u);
            if (time_trace) HIP_CHECK(hipEventRecord(scene->ev_pool[2 * launch + 1], stream));
            launch++;
        }
        first += groups;
    }
    HIP_CHECK(hipGetLastError());
    scene->pt_launches = launch;
    if (d_trace) { // diagnostic dump: raw float32, 4 words header (count first), then 16 words per consumed hit record
        std::vector<float4> h(trace_cap);
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipMemcpy(h.data(), d_trace, (size_t)trace_cap * sizeof(float4), hipMemcpyDeviceToHost));
        (void)hipFree(d_trace);
        if (FILE *f = fopen(env_str("RTAMD_TRACE_OUT"), "wb")) { fwrite(h.data(), sizeof(float4), trace_cap, f); fclose(f); }
    }
}

// The kernels that render a frame.  hw8 / hw7: the persistent dataflow pipeline, the round pipeline or the megakernel; hw6: its own
// persistent pipeline or its per-lane path machine; hw1..hw5: one kernel each.
enum class Pipeline { Persistent8, Persistent6, Rounds, Mega6, Mega8, Hw1, Hw2, Hw3, Hw4, Hw5 };

// hw8 / hw7: persistent dataflow pipeline (default) | round pipeline (RTAMD_KERNEL=wavefront, and for trees deeper than the LDS stack
// columns) | megakernel (RTAMD_KERNEL=mega, and for trees deeper than the round kernels' stacks).
// The persistent pipeline is the default at every size: it takes reference-exact box decisions at no measurable cost for the exact
// walks themselves (they hide behind the other waves of the workgroup), keeps a small path population — a shard of a multi-GPU
// frame — near the full rate, and since round 3 (five waves per SIMD, four-wide grid nodes, postponed leaves) it is a third faster
// than the round pipeline on a full 1080p frame.  The round pipeline stands in for trees deeper than the LDS stack columns, then with
// its exact kernels on (a serial walk of the reference tree, ~1.5 ms, sits on the critical path of every round); chosen explicitly
// (RTAMD_KERNEL=wavefront, reported in `rounds_chosen`) it keeps the padded box test's answer unless RTAMD_ROUNDS_EXACT=1.
// RTAMD_AUTO_GROUPS_PER_CU=n: opt into the round pipeline from n sub-tiles per CU on.  RTAMD_WF_LDS_STACK (testing) takes the round
// pipeline's spill variant.
// hw6: the persistent pipeline (device/rt_persistent_hw6.h) when both own trees fit its stack columns; RTAMD_KERNEL=mega and
// RTAMD_HW6_SCRATCH_STACK keep the per-lane path machine.
static Pipeline choose_pipeline(const rt_scene *scene, int integrator, const RenderView &R, uint32_t n_work, int streams, bool &rounds_chosen) {
    const char *ksel = env_str("RTAMD_KERNEL");
    const bool mega = ksel && strcmp(ksel, "mega") == 0;
    rounds_chosen = ksel && strcmp(ksel, "wavefront") == 0;
    switch (integrator) { // the .txt scenes' integrators
    case RT_INTEGRATOR_HW1: return Pipeline::Hw1;
    case RT_INTEGRATOR_HW2: return Pipeline::Hw2;
    case RT_INTEGRATOR_HW3: return Pipeline::Hw3;
    case RT_INTEGRATOR_HW4: return Pipeline::Hw4;
    case RT_INTEGRATOR_HW5: return Pipeline::Hw5;
    }
    if (scene->flavor == RT_INTEGRATOR_HW6)
        return scene->hw6_pt_stack && !mega && !env_flag("RTAMD_HW6_SCRATCH_STACK") ? Pipeline::Persistent6 : Pipeline::Mega6;
    const rt_scene_info &I = scene->info;
    if (mega || I.bvh_depth > WF_STACK + WF_OVF || I.light_bvh_depth > 64 || I.n_triangles >= 0x40000000u // light depth: 64-bit frame mask
        || R.samples / streams >= (1 << 25)) // the path record keeps the sample index in 25 bits
        return Pipeline::Mega8;
    if (rounds_chosen || I.bvh_depth > P8_STACK || scene->light_walk_depth > P8_STACK || env_flag("RTAMD_WF_LDS_STACK")) return Pipeline::Rounds;
    const uint64_t auto_groups = (uint64_t)env_int("RTAMD_AUTO_GROUPS_PER_CU", 0);
    if (!ksel && auto_groups && (uint64_t)n_work * (uint64_t)streams >= auto_groups * (uint64_t)scene->n_cus) return Pipeline::Rounds;
    return Pipeline::Persistent8;
}

// RTAMD_DEBUG_COUNTERS after a persistent render: launches and re-deal, where the waves' time went (counting renders) and when the
// workgroups of the last launch left; RTAMD_DUMP_WG=file: start / exit time (ms after the first start) and paths of each of them
// (tools/tuning/wg_balance.py).
static void report_persistent(rt_scene *scene, bool hw6, const char *kernel, bool count, const unsigned long long *h_cnt) {
    const bool times = scene->d_pt_debug && scene->pt_blocks <= PT_DEBUG_BLOCKS;
    const unsigned long long *role = h_cnt + CNT_ROLE_TIME;
    const double tt = (double)(role[0] + role[1] + role[2] + role[3] + role[4]);
    auto nz = [](unsigned long long d) { return (double)(d ? d : 1); }; // a denominator that may be zero
    if (hw6) {
        fprintf(stderr, "[rtamd] persistent hw6 pipeline: %u launches; re-deal %.2f ms on the host (slowest workgroup / mean under the round-robin deal: %.3f); light sums through the slow role %llu of %llu; exact closest-hit walks %llu of %llu, exact light sums %llu\n",
                scene->pt_launches, scene->pt_rebalance_ms, scene->pt_imbalance, h_cnt[CNT_P6_SLOW_LIGHT], h_cnt[CNT_LIGHT], h_cnt[CNT_EXACT_CLOSEST], h_cnt[CNT_CLOSEST], h_cnt[CNT_P6_EXACT_LIGHT]);
        if (count) {
            fprintf(stderr, "[rtamd] persistent hw6 kernel, light sums in the slow role by number of hits (0..14, 15+):");
            for (int b = 0; b < 16; b++) fprintf(stderr, " %llu", h_cnt[CNT_P6_SLOW_HITS + b]);
            fprintf(stderr, "\n");
            fprintf(stderr, "[rtamd] persistent hw6 kernel, wave time by role: closest-hit walks %.1f %%, light walks %.1f %%, shading %.1f %%, slow light sums %.1f %%, idle %.1f %%\n",
                    100 * role[0] / tt, 100 * role[1] / tt, 100 * role[2] / tt, 100 * role[3] / tt, 100 * role[4] / tt);
        }
    } else if (times && count) {
        const unsigned long long *iters = h_cnt + CNT_P8_WALK_ITERS, n_light = h_cnt[CNT_LIGHT];
        fprintf(stderr, "[rtamd] persistent kernel, wave time by role: closest-hit walks %.1f %%, light walks %.1f %%, shading %.1f %%, exact walks %.2f %%, idle %.1f %%; "
                        "walker lane utilisation: closest hit %.1f of 64 (%llu wave iterations), light %.1f of 64 (%llu); %llu stints, %llu shade batches of %.1f paths\n",
                100 * role[0] / tt, 100 * role[1] / tt, 100 * role[2] / tt, 100 * role[3] / tt, 100 * role[4] / tt,
                (double)iters[1] / nz(iters[0]), iters[0], (double)iters[3] / nz(iters[2]), iters[2],
                h_cnt[CNT_P8_STINTS], h_cnt[CNT_P8_SHADE_BATCHES], (double)h_cnt[CNT_P8_SHADE_ITEMS] / nz(h_cnt[CNT_P8_SHADE_BATCHES]));
        for (int w = 0; w < 2; w++) {
            const unsigned long long *part = h_cnt + CNT_P8_WALK_TIME + 3 * w, *leaf = h_cnt + CNT_P8_LEAF_ITERS + 2 * w;
            const double tw = (double)(part[0] + part[1] + part[2]);
            fprintf(stderr, "[rtamd]   %s walker's wave time: hand-off and refill %.1f %%, inner nodes %.1f %%, leaves %.1f %%; leaf passes %llu with %.1f of 64 lanes\n",
                    w ? "light" : "closest-hit", 100 * part[0] / tw, 100 * part[1] / tw, 100 * part[2] / tw, leaf[0], (double)leaf[1] / nz(leaf[0]));
        }
        {
            const unsigned long long *ts = h_cnt + CNT_P8_SHADE_TIME, *ls = h_cnt + CNT_P8_SHADE_LANES, nb = h_cnt[CNT_P8_SHADE_BATCHES];
            static const char *const section[5] = {"record load, gate and pending bounce", "attributes and textures", "Mix::sample", "BRDF and pdf", "path end"};
            fprintf(stderr, "[rtamd]   shader's wave time (%.0f cycles per batch):", (double)role[2] / nz(nb));
            for (int k = 0; k < 5; k++) fprintf(stderr, " %s %.1f %% (%.0f cycles, %.1f lanes per batch)%s", section[k], 100.0 * ts[k] / nz(role[2]), (double)ts[k] / nz(nb), (double)ls[k] / nz(nb), k < 4 ? "," : "");
            fprintf(stderr, "; the rest (%.1f %%): pop, settled light sums, pushes; hits at the deepest level: %.2f lanes per batch\n",
                    100.0 * (1.0 - (double)(ts[0] + ts[1] + ts[2] + ts[3] + ts[4]) / nz(role[2])), (double)h_cnt[CNT_P8_SHADE_LAST] / nz(nb));
        }
        const unsigned long long *handoff = h_cnt + CNT_P8_HANDOFF_TIME, tests = h_cnt[CNT_P8_LIGHT_TESTS], hits = h_cnt[CNT_P8_LIGHT_HITS], *reach = h_cnt + CNT_P8_LIGHT_REACH;
        fprintf(stderr, "[rtamd]   closest-hit walker's hand-off points: %llu; of their time: publishing finished walks %.1f %%, taking new ones from the bitmap %.1f %%, reading their rays %.1f %% (the rest: the test itself)\n",
                h_cnt[CNT_P8_HANDOFFS], 100.0 * handoff[0] / nz(h_cnt[CNT_P8_WALK_TIME]), 100.0 * handoff[1] / nz(h_cnt[CNT_P8_WALK_TIME]), 100.0 * handoff[2] / nz(h_cnt[CNT_P8_WALK_TIME]));
        for (int q = 0; q < 3; q++) {
            const unsigned long long *pop = h_cnt + CNT_P8_POPS + 3 * q;
            fprintf(stderr, "[rtamd]   pops of the %s queue: %llu, %.1f paths from %.2f claimed words each\n", q == 0 ? "closest-hit" : q == 1 ? "light" : "shade",
                    pop[0], (double)pop[1] / nz(pop[0]), (double)pop[2] / nz(pop[0]));
        }
        fprintf(stderr, "[rtamd]   light tests %llu (%.2f per light sum), hits %llu (%.2f per light sum); triangle tests of closest-hit walks %llu (%.2f per query)\n",
                tests, (double)tests / nz(n_light), hits, (double)hits / nz(n_light), h_cnt[CNT_TRI_TESTS] - tests, (double)(h_cnt[CNT_TRI_TESTS] - tests) / nz(h_cnt[CNT_CLOSEST]));
        fprintf(stderr, "[rtamd]   light sums whose walk ends at the light tree's root %llu (%.1f %%), one level below it %llu (%.1f %%); settled by the shader: level %d\n",
                reach[0], 100.0 * reach[0] / nz(n_light), reach[1], 100.0 * reach[1] / nz(n_light), PT_LIGHT_SETTLE);
    }
    if (!times) return;
    std::vector<unsigned long long> dbg((size_t)scene->pt_blocks * 3);
    HIP_CHECK(hipMemcpy(dbg.data(), scene->d_pt_debug, dbg.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, tmin = ~0ull, tmax = 0; double tsum = 0;
    for (uint32_t b = 0; b < scene->pt_blocks; b++) if (dbg[3 * b] && dbg[3 * b] < t0) t0 = dbg[3 * b];
    for (uint32_t b = 0; b < scene->pt_blocks; b++) { unsigned long long e = dbg[3 * b + 1] - t0; tmin = e < tmin ? e : tmin; tmax = e > tmax ? e : tmax; tsum += (double)e; }
    if (const char *dump = env_str("RTAMD_DUMP_WG")) {
        if (FILE *f = fopen(dump, "w")) {
            for (uint32_t b = 0; b < scene->pt_blocks; b++) fprintf(f, "%u %.4f %.4f %llu\n", b, (dbg[3 * b] - t0) * 1e-5, (dbg[3 * b + 1] - t0) * 1e-5, dbg[3 * b + 2]);
            fclose(f);
        }
    }
    if (!hw6)
        fprintf(stderr, "[rtamd] persistent pipeline: %u launches; re-deal of the sub-tiles took %.2f ms on the host (slowest workgroup / mean under the round-robin deal: %.3f)\n",
                scene->pt_launches, scene->pt_rebalance_ms, scene->pt_imbalance);
    fprintf(stderr, "[rtamd] %s (last launch): %u workgroups, exit times min / mean / max = %.3f / %.3f / %.3f ms after the first start",
            kernel, scene->pt_blocks, tmin * 1e-5, tsum / scene->pt_blocks * 1e-5, tmax * 1e-5);
    if (!hw6) fprintf(stderr, "; exact closest hits %llu, exact light sums %llu of %llu + %llu queries", h_cnt[CNT_EXACT_CLOSEST], h_cnt[CNT_EXACT_LIGHT], h_cnt[CNT_CLOSEST], h_cnt[CNT_LIGHT]);
    fprintf(stderr, "\n");
}

// Resumable renders advance the kernels that can park and resume a path: both persistent pipelines and the round pipeline.
// Returns what stands in the way, or null.
static const char *accum_unsupported(Pipeline pipe, const rt_render_params *p) {
    if (p->sample_streams > 1) return "throughput mode (sample_streams > 1) has no resumable state";
    if (p->flags & ~RT_FLAG_COUNTERS) return "flags other than RT_FLAG_COUNTERS do not apply to a resumable render (the outputs are named at rt_accum_resolve)";
    switch (pipe) {
    case Pipeline::Persistent8: case Pipeline::Persistent6: case Pipeline::Rounds: return nullptr;
    case Pipeline::Mega8: return "the hw8 / hw7 megakernel is in effect (RTAMD_KERNEL=mega, or a tree beyond the persistent and round kernels' limits): a resumable render needs the persistent or the round pipeline";
    case Pipeline::Mega6: return "the hw6 per-lane path machine is in effect (RTAMD_KERNEL=mega, RTAMD_HW6_SCRATCH_STACK, or a tree beyond the persistent hw6 kernel's stacks): a resumable render needs the persistent hw6 pipeline";
    default: return "the hw1 .. hw5 integrators have no resumable state (RT_INTEGRATOR_HW6 / HW7 / HW8 only)";
    }
}

// One slice of a resumable render (rt_accum_render): every pixel goes from sample `first` to `first + p->samples` of its stream,
// from and to `state` (RenderView::accum) instead of from a seed and to a pixel.
struct AccumSlice { uint32_t *state; int32_t first; };

// What the checks of a frame settle for its launch and its statistics.
struct Frame {
    RenderView R{};
    SceneView V8{};            // per-render copy of the hw8 view: the hw7 replay switches and the exactness are render parameters, not scene state
    Pipeline pipe = Pipeline::Persistent8;
    bool rounds_chosen = false, count = false, time_trace = false;
    uint32_t n_work = 0;       // 8x8 sub-tiles of this shard
    uint32_t blocks = 0;       // workgroups of the one-kernel pipelines; 0 = nothing to render
    int streams = 1;
    float txt_tan_fov_y = 0;
    uint32_t launches = 0;
};

// ray_depth a render may ask of RT_INTEGRATOR_HWn (hw1 has none of its own; for it, hw7 and hw8 resolve_tiles has checked RT_MAX_DEPTH).
static const int max_ray_depth[RT_INTEGRATOR_HW8 + 1] = {0, RT_MAX_DEPTH, RT2_MAX_DEPTH, RT3_MAX_DEPTH, RT4_MAX_DEPTH, RT4_MAX_DEPTH, RT6_MAX_DEPTH, RT_MAX_DEPTH, RT_MAX_DEPTH};

// Part one of a render: argument and limit checks, in the order in which each error has always won; fills `F`.  Host only.
// scene.cpp:181 — evaluated on the host in float exactly like the reference; for the render launch and for rt_camera_rays
static float frame_tan_fov_x(const SceneView &V, int32_t width, int32_t height) { return V.tan_fov_y * width / height; }

static int check_frame(const rt_scene *scene, const rt_render_params *p, const AccumSlice *slice, const std::string &who, Frame &F) {
    if (!scene || !p) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (p->struct_size != sizeof(rt_render_params)) return fail(RT_ERR_INVALID_ARG, who + "struct_size mismatch (ABI skew)");
    if (p->integrator < RT_INTEGRATOR_HW1 || p->integrator > RT_INTEGRATOR_HW8) return fail(RT_ERR_UNSUPPORTED, who + "unknown integrator");
    const bool txt_scene = scene->flavor == RT_INTEGRATOR_HW3;
    const bool txt_integrator = p->integrator >= RT_INTEGRATOR_HW1 && p->integrator <= RT_INTEGRATOR_HW5;
    const bool hw7 = p->integrator == RT_INTEGRATOR_HW7; // renders a scene prepared for hw8 with hw7's material model (no textures)
    if (txt_scene != txt_integrator || (!txt_scene && p->integrator != scene->flavor && !(hw7 && scene->flavor == RT_INTEGRATOR_HW8)))
        return fail(RT_ERR_INVALID_ARG, who + "this scene was prepared for integrator " + std::to_string(scene->flavor) +
                                            " (hw6 scenes carry no vertex normals, hw8 scenes do)");
    RenderView &R = F.R;
    std::string err;
    if (!resolve_tiles(p, R, err)) return fail(RT_ERR_INVALID_ARG, who + "" + err);
    F.count = (p->flags & RT_FLAG_COUNTERS) != 0;
    R.work_counter = scene->d_work_counter;
    R.counters = F.count ? scene->d_counters : nullptr;
    R.tan_fov_x = frame_tan_fov_x(scene->view, R.width, R.height);
    // scene.cpp:176 — evaluated on the host in float exactly like the reference
    R.inv_samples = (float)(1.0 / R.samples);
    const uint32_t n_work = F.n_work = R.n_shard_tiles * (uint32_t)((R.tile_w >> 3) * (R.tile_h >> 3));
    const int streams = F.streams = p->sample_streams > 1 ? p->sample_streams : 1;
    if (slice) { // sample indices are absolute, in the records as in RenderView
        R.accum = slice->state; R.sample_first = slice->first; R.samples += slice->first;
        R.n_pixslots = n_work * 64u;
    }
    R.sample_stop = R.samples;
    if (p->reserved != 0) return fail(RT_ERR_INVALID_ARG, who + "reserved must be 0");
    if ((p->flags & (RT_FLAG_SAMPLE_SEEDS | RT_FLAG_RUSSIAN_ROULETTE)) && streams <= 1)
        return fail(RT_ERR_INVALID_ARG, who + "RT_FLAG_SAMPLE_SEEDS / RT_FLAG_RUSSIAN_ROULETTE change the estimator and belong to throughput mode (sample_streams > 1)");
    if (streams > 1) { // throughput mode (include/rtamd.h: sample_streams)
        if (p->integrator != RT_INTEGRATOR_HW8 && p->integrator != RT_INTEGRATOR_HW7 && p->integrator != RT_INTEGRATOR_HW6) return fail(RT_ERR_UNSUPPORTED, who + "sample_streams > 1 is implemented for RT_INTEGRATOR_HW6 / HW7 / HW8 only");
        if (p->integrator == RT_INTEGRATOR_HW6 && (p->flags & (RT_FLAG_SAMPLE_SEEDS | RT_FLAG_RUSSIAN_ROULETTE))) return fail(RT_ERR_UNSUPPORTED, who + "RT_FLAG_SAMPLE_SEEDS / RT_FLAG_RUSSIAN_ROULETTE are implemented for RT_INTEGRATOR_HW7 / HW8 only");
        if (streams > 256 || R.samples % streams != 0) return fail(RT_ERR_INVALID_ARG, who + "samples must be a multiple of sample_streams (at most 256 streams)");
        if ((int64_t)R.width * R.height * streams >= 2147483647LL) return fail(RT_ERR_INVALID_ARG, who + "width*height*sample_streams must stay below 2^31-1 (stream seeds)");
        if ((uint64_t)n_work * 64u * (uint64_t)streams >= 0x40000000ull) return fail(RT_ERR_LIMIT, who + "too many path slots (pixels of this shard x sample_streams)");
    }
    F.blocks = std::min((uint32_t)scene->n_cus * 16u, n_work);
    F.pipe = choose_pipeline(scene, p->integrator, R, n_work, streams, F.rounds_chosen);
    if (slice) if (const char *why = accum_unsupported(F.pipe, p)) return fail(RT_ERR_UNSUPPORTED, who + why);
    if (streams > 1 && F.pipe != Pipeline::Persistent8 && F.pipe != Pipeline::Rounds && F.pipe != Pipeline::Persistent6) return fail(RT_ERR_UNSUPPORTED, who + "sample_streams > 1 needs the persistent / round kernels (RTAMD_KERNEL=mega or a tree beyond their limits is in effect)");
    // the integrators' own limits; hw3's ray_depth has always been looked at before the TRIANGLE figures, the others' after them
    const int max_depth = max_ray_depth[p->integrator];
    const bool too_deep = R.ray_depth > max_depth;
    auto deep = [&] { return fail(RT_ERR_LIMIT, who + "hw" + std::to_string(p->integrator) + " ray_depth above " + std::to_string(max_depth)); }; // RT_INTEGRATOR_HWn = n
    if (too_deep && p->integrator == RT_INTEGRATOR_HW3) return deep();
    if (txt_scene && scene->txt_has_triangles && p->integrator != RT_INTEGRATOR_HW5) return fail(RT_ERR_INVALID_ARG, who + "a .txt scene with TRIANGLE figures renders with RT_INTEGRATOR_HW5 only");
    if (too_deep) return deep();
    if (p->integrator == RT_INTEGRATOR_HW5 && (scene->info.bvh_depth > RT5_STACK || scene->info.light_bvh_depth > RT5_STACK)) return fail(RT_ERR_LIMIT, who + "hw5 BVH deeper than 64");
    if (p->integrator == RT_INTEGRATOR_HW4 && scene->viewt.n_light_prims > RT4_MAX_LIGHTS) return fail(RT_ERR_LIMIT, who + "hw4 supports at most 32 emissive box/ellipsoid lights");
    if (p->integrator == RT_INTEGRATOR_HW1 && R.shard_count > 1) return fail(RT_ERR_UNSUPPORTED, who + "the hw1 caster renders unsharded frames only");
    const bool float_tan = p->integrator == RT_INTEGRATOR_HW1 || p->integrator == RT_INTEGRATOR_HW2;
    F.txt_tan_fov_y = (float_tan ? scene->viewt.tan_fov_x_f : scene->viewt.tan_fov_x) * R.height / R.width; // hw3/src/scene.cpp:101
    F.V8 = scene->view;
    if (hw7) { F.V8.hw7 = 1; F.V8.last_level_emission_only = 0; F.V8.env_image = -1; }
    // Exactness follows the scene, not the pipeline: when the persistent pipeline cannot take the scene (a tree deeper than its
    // stack columns), the round pipeline runs with its exact kernels on.  Only an explicit RTAMD_KERNEL=wavefront (the yardstick
    // of the benchmarks; RTAMD_ROUNDS_EXACT=1 switches the exact kernels on there too) and the megakernel, which has no gate,
    // keep the padded boxes' answer — and say so in rt_stats.reference_exact.
    if (F.pipe != Pipeline::Persistent8 && (F.pipe != Pipeline::Rounds || (F.rounds_chosen && !env_flag("RTAMD_ROUNDS_EXACT")))) F.V8.exact_boxes = 0;
    if (!F.V8.exact_boxes) F.V8.cull_k = 4.8e-7f; // no exact walks to feed: the walkers look behind the best hit by the tie tolerance only
    return RT_OK;
}

// Part two: the launches of the frame on `stream`, between the scene's two events.  want_times: rt_stats are asked for.
static void launch_frame(rt_scene *scene, const rt_render_params *p, Frame &F, hipStream_t stream, bool want_times) {
    RenderView &R = F.R;
    const SceneView &V8 = F.V8;
    const uint32_t n_work = F.n_work, blocks = F.blocks;
    const int streams = F.streams;
    const bool count = F.count;
    HIP_CHECK(hipMemsetAsync(scene->d_work_counter, 0, 4, stream));
    HIP_CHECK(hipMemsetAsync(scene->d_counters, 0, CNT_BYTES, stream));
    if (count && env_flag("RTAMD_DEBUG_COUNTERS")) HIP_CHECK(hipMemsetAsync(scene->d_counters + CNT_WANT_HISTOGRAMS, 1, 1, stream)); // asks the counting kernels for the in-flight histograms
    HIP_CHECK(hipEventRecord(scene->ev_start, stream));
    if (blocks) {
        if (streams > 1) { // throughput mode (include/rtamd.h: sample_streams): K path slots per pixel, `samples` per stream, a partial-sum buffer and a final reduction
            R.streams = streams; R.n_pixslots = n_work * 64u; R.seed_stride = (uint32_t)R.width * (uint32_t)R.height;
            R.total_samples = (uint32_t)R.samples;
            R.sample_seeds = (p->flags & RT_FLAG_SAMPLE_SEEDS) ? 1u : 0u;
            R.rr_depth = (p->flags & RT_FLAG_RUSSIAN_ROULETTE) ? 2 : 0;
            R.samples /= streams;                           // per stream; inv_samples stays 1 / (all samples of the pixel)
            R.sample_stop = R.samples;
            grow(scene->d_partial, scene->partial_bytes, (size_t)streams * R.n_pixslots * 3 * sizeof(float));
            R.partial = scene->d_partial;
        }
        const uint32_t n_slot_groups = n_work * (uint32_t)streams; // 64-slot groups of all streams
        F.launches = 1;
        switch (F.pipe) {
        case Pipeline::Persistent8:
        case Pipeline::Persistent6:
            F.time_trace = want_times;
            launch_persistent(scene, F.pipe == Pipeline::Persistent8 ? hw8_persistent(V8, R.ray_depth, stream, count) : hw6_persistent(scene->view6, stream, count),
                              R, n_slot_groups, stream, count, F.time_trace);
            F.launches = scene->pt_launches;
            break;
        case Pipeline::Rounds:
            // every traverse launch is bracketed by events when stats are wanted -- up to 64 k rounds (e.g. 10,922 spp at depth 6)
            F.time_trace = want_times && wavefront_rounds(V8, R) * (size_t)wavefront_pipelines(n_slot_groups) <= 65536;
            launch_wavefront(scene, V8, R, n_slot_groups, stream, count, F.time_trace);
            F.launches = (uint32_t)scene->wf_pipes * (1 + 2 * (uint32_t)wavefront_rounds(V8, R));
            break;
        case Pipeline::Mega6:
            if (scene->hw6_lds_stack && !env_flag("RTAMD_HW6_SCRATCH_STACK")) hipLaunchKernelGGL(dev::render_hw6_kernel<true>, dim3(blocks), dim3(64), 0, stream, scene->view6, R, n_work);
            else hipLaunchKernelGGL(dev::render_hw6_kernel<false>, dim3(blocks), dim3(64), 0, stream, scene->view6, R, n_work);
            break;
        case Pipeline::Mega8:
            if (count) hipLaunchKernelGGL(dev::render_hw8_kernel<true>, dim3(blocks), dim3(64), 0, stream, V8, R, n_work);
            else hipLaunchKernelGGL(dev::render_hw8_kernel<false>, dim3(blocks), dim3(64), 0, stream, V8, R, n_work);
            break;
        case Pipeline::Hw1: {
            uint32_t npx = (uint32_t)R.width * (uint32_t)R.height;
            hipLaunchKernelGGL(dev::render_hw1_kernel, dim3((npx + 255) / 256), dim3(256), 0, stream, scene->viewt, R.width, R.height, F.txt_tan_fov_y, R.out_rgb, R.out_rgb8);
            break;
        }
        case Pipeline::Hw2: hipLaunchKernelGGL(dev::render_hw2_kernel, dim3(blocks), dim3(64), 0, stream, scene->viewt, R, F.txt_tan_fov_y, n_work); break;
        case Pipeline::Hw3: hipLaunchKernelGGL(dev::render_hw3_kernel, dim3(blocks), dim3(64), 0, stream, scene->viewt, R, F.txt_tan_fov_y, n_work); break;
        case Pipeline::Hw4: hipLaunchKernelGGL(dev::render_hw4_kernel, dim3(blocks), dim3(64), 0, stream, scene->viewt, R, F.txt_tan_fov_y, n_work); break;
        case Pipeline::Hw5: hipLaunchKernelGGL(dev::render_hw5_kernel, dim3(blocks), dim3(64), 0, stream, scene->view5, R, F.txt_tan_fov_y, n_work); break;
        }
        HIP_CHECK(hipGetLastError());
        if (streams > 1) {
            hipLaunchKernelGGL(dev::wf_reduce_streams_kernel, dim3((R.n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
            HIP_CHECK(hipGetLastError());
            F.launches++;
        }
    }
    HIP_CHECK(hipEventRecord(scene->ev_stop, stream));
}

// Part three: wait for the frame, read its counters (rt_types.h CounterSlot), report what the kernels gave up on, print the
// RTAMD_DEBUG_COUNTERS report and fill `stats` (nullable).  t0: when the render began.
static int collect_frame(rt_scene *scene, const Frame &F, hipStream_t stream, rt_stats *stats, double t0, const std::string &who) {
    const RenderView &R = F.R;
    const SceneView &V8 = F.V8;
    const Pipeline pipe = F.pipe;
    const bool count = F.count, time_trace = F.time_trace, debug = env_flag("RTAMD_DEBUG_COUNTERS");
    unsigned long long h_cnt[CNT_SLOTS] = {0};
    HIP_CHECK(hipMemcpyAsync(h_cnt, scene->d_counters, CNT_BYTES, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream)); // render is synchronous on return
    const bool ran_persistent = F.blocks && (pipe == Pipeline::Persistent8 || pipe == Pipeline::Persistent6);
    const bool ran_rounds = F.blocks && pipe == Pipeline::Rounds;
    if (ran_persistent) {
        const bool hw6 = pipe == Pipeline::Persistent6;
        const char *kernel = hw6 ? "persistent hw6 kernel" : "persistent kernel";
        if (!hw6) h_cnt[CNT_CLOSEST] -= std::min(h_cnt[CNT_DISCARDED], h_cnt[CNT_CLOSEST]); // speculative closest-hit queries that the clamp step discarded are not part of the algorithm
        if (debug) report_persistent(scene, hw6, kernel, count, h_cnt);
        if (h_cnt[CNT_DEADLINE]) return fail(RT_ERR_LIMIT, who + "the " + kernel + " ran into its launch deadline (" + std::to_string(h_cnt[CNT_DEADLINE]) + " waves; RTAMD_PT_TIMEOUT_S raises it); the frame is incomplete");
        if (h_cnt[CNT_LOST_PATH]) return fail(RT_ERR_HIP, who + "the " + kernel + " lost a path (" + std::to_string(h_cnt[CNT_LOST_PATH]) + " waves gave up waiting); the frame is incomplete");
    }
    auto round_counters = [&] { // of the round pipeline: WF_CTR words per round and pipeline
        std::vector<uint32_t> ctr(scene->wf_ctr_block * scene->wf_pipes);
        HIP_CHECK(hipMemcpy(ctr.data(), scene->wf.ctr, ctr.size() * 4, hipMemcpyDeviceToHost));
        return ctr;
    };
    if (count && ran_rounds) { // queries = lengths of the per-round queues
        size_t rounds = wavefront_rounds(V8, R);
        const std::vector<uint32_t> ctr = round_counters();
        for (int h = 0; h < scene->wf_pipes; h++)
            for (size_t r = 0; r < rounds; r++) {
                const uint32_t *c = ctr.data() + (size_t)h * scene->wf_ctr_block + WF_CTR * r;
                h_cnt[CNT_CLOSEST] += c[0];
                if (scene->info.n_lights) { h_cnt[CNT_LIGHT] += c[1]; h_cnt[CNT_WF_SLOW_LIGHT] += c[4]; }
            }
        h_cnt[CNT_CLOSEST] -= h_cnt[CNT_DISCARDED]; // speculative closest-hit queries that the clamp step discarded are not part of the algorithm
        h_cnt[CNT_EXACT_LIGHT] = h_cnt[CNT_WF_SLOW_LIGHT]; // light sums finished by the exact kernel
    }
    // The two histograms are the round pipeline's (CNT_WF_HIST_*).  After a persistent hw8 render the same lines print what that kernel
    // keeps in those slots (CNT_ROLE_TIME .. CNT_P8_LIGHT_REACH, then CNT_P8_POPS and zeros), and the last line's CNT_WF_* slots are the round pipeline's
    // too (after a persistent hw6 render slot 11 is CNT_P6_EXACT_LIGHT): kept as they are, see profiles/r08_api_split.txt.
    if (count && debug && (pipe == Pipeline::Persistent8 || pipe == Pipeline::Rounds)) { // wave iterations a query stays in flight, buckets of 32
        fprintf(stderr, "[rtamd] closest-hit queries by in-flight wave iterations (x32):");
        for (int b = 0; b < 16; b++) fprintf(stderr, " %llu", h_cnt[CNT_WF_HIST_CLOSEST + b]);
        fprintf(stderr, "\n[rtamd] light queries by in-flight wave iterations (x32):");
        for (int b = 0; b < 16; b++) fprintf(stderr, " %llu", h_cnt[CNT_WF_HIST_LIGHT + b]);
        fprintf(stderr, "\n");
    }
    if (count && debug)
        fprintf(stderr, "[rtamd] light queries finished by the exact kernel: %llu of %llu; trace kernel: wave node-iterations %llu, leaf phases %llu (lanes %llu), refills %llu; lane node visits %llu, tri tests %llu\n",
                h_cnt[CNT_WF_SLOW_LIGHT], h_cnt[CNT_LIGHT], h_cnt[CNT_WF_NODE_ITERS], h_cnt[CNT_WF_LEAF_PHASES], h_cnt[CNT_WF_LEAF_LANES], h_cnt[CNT_WF_REFILLS],
                h_cnt[CNT_WF_LANE_NODES], h_cnt[CNT_WF_LANE_TRIS]);
    if (!stats) return RT_OK;
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop));
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = ms;
    stats->total_ms = now_ms() - t0;
    stats->launches = F.launches;
    stats->pipeline = ran_persistent ? RT_PIPELINE_PERSISTENT : ran_rounds ? RT_PIPELINE_ROUNDS : RT_PIPELINE_SINGLE;
    stats->reference_exact = pipe == Pipeline::Hw5 ? 1u : pipe == Pipeline::Persistent6 ? (F.blocks && scene->view6.exact_boxes ? 1u : 0u)
                             : ((ran_persistent || ran_rounds) && V8.exact_boxes == 1u ? 1u : 0u);
    if (ran_persistent) {
        double sum = 0;
        for (uint32_t pp = 0; time_trace && pp < scene->pt_launches; pp++) { float e = 0; HIP_CHECK(hipEventElapsedTime(&e, scene->ev_pool[2 * pp], scene->ev_pool[2 * pp + 1])); sum += e; }
        stats->dominant_kernel_ms = time_trace ? sum : ms; stats->dominant_kernel_launches = scene->pt_launches;
        stats->exact_closest_hits = h_cnt[CNT_EXACT_CLOSEST];
        stats->exact_light_sums = pipe == Pipeline::Persistent6 ? h_cnt[CNT_P6_EXACT_LIGHT] : h_cnt[CNT_EXACT_LIGHT];
    } else if (ran_rounds && time_trace) {
        stats->exact_closest_hits = h_cnt[CNT_EXACT_CLOSEST]; stats->exact_light_sums = h_cnt[CNT_EXACT_LIGHT]; // counting renders only
        size_t rounds = wavefront_rounds(V8, R);
        double sum = 0;
        const size_t n_launch = rounds * (size_t)scene->wf_pipes; // with more than one pipeline a launch shares the GPU with the other pipelines' kernels
        for (size_t r = 0; r < n_launch; r++) { float e = 0; HIP_CHECK(hipEventElapsedTime(&e, scene->ev_pool[2 * r], scene->ev_pool[2 * r + 1])); sum += e; }
        stats->dominant_kernel_ms = sum; stats->dominant_kernel_launches = (uint32_t)n_launch;
        if (const char *path = env_str("RTAMD_DUMP_ROUNDS")) { // diagnostic: per launch of the traverse kernel its queue lengths and duration
            const std::vector<uint32_t> ctr = round_counters();
            if (FILE *f = fopen(path, "a")) { // appended: one block per render
                fprintf(f, "round,pipeline,closest_hit_queries,light_queries,traverse_ms\n");
                for (size_t r = 0; r < rounds; r++)
                    for (int h = 0; h < scene->wf_pipes; h++) {
                        float e = 0; (void)hipEventElapsedTime(&e, scene->ev_pool[2 * (r * scene->wf_pipes + h)], scene->ev_pool[2 * (r * scene->wf_pipes + h) + 1]);
                        const uint32_t *c = ctr.data() + (size_t)h * scene->wf_ctr_block + WF_CTR * r;
                        fprintf(f, "%zu,%d,%u,%u,%.4f\n", r, h, c[0], c[1], e);
                    }
                fclose(f);
            }
        }
    } else { stats->dominant_kernel_ms = ms; stats->dominant_kernel_launches = F.launches; }
    uint64_t px = 0; // pixels of this shard that lie inside the image
    for (uint32_t st = 0; st < R.n_shard_tiles; st++) {
        int x0, y0, w, h;
        shard_tile_rect(R, st, x0, y0, w, h);
        px += (uint64_t)w * h;
    }
    stats->samples = px * (uint64_t)(R.samples - R.sample_first) * (uint64_t)F.streams;
    stats->closest_hit_queries = h_cnt[CNT_CLOSEST]; stats->light_pdf_queries = h_cnt[CNT_LIGHT];
    stats->node_visits = h_cnt[CNT_NODE_VISITS]; stats->triangle_tests = h_cnt[CNT_TRI_TESTS];
    return RT_OK;
}

// rt_render, and with `slice` rt_accum_render: the same checks, pipelines, launches and statistics.
static int render_frame(rt_scene *scene, const rt_render_params *p, float *out_rgb, uint8_t *out_rgb8, rt_stats *stats, const AccumSlice *slice) {
    const std::string who = slice ? "rt_accum_render: " : "rt_render: ";
    return guarded(who, [&]() -> int {
        Frame F;
        if (const int rc = check_frame(scene, p, slice, who, F)) return rc;
        const double t0 = now_ms();
        HIP_CHECK(hipSetDevice(scene->device));
        hipStream_t stream = (hipStream_t)p->stream;
        const size_t elems = rt_output_elems(p);
        StagedOut rgb(out_rgb, p->flags, elems, sizeof(float)), rgb8(out_rgb8, p->flags, elems, 1);
        F.R.out_rgb = (float *)rgb.dev; F.R.out_rgb8 = (uint8_t *)rgb8.dev;
        launch_frame(scene, p, F, stream, stats != nullptr);
        rgb.copy_back(stream);
        rgb8.copy_back(stream);
        return collect_frame(scene, F, stream, stats, t0, who);
    });
}

int rt_render(rt_scene *scene, const rt_render_params *p, float *out_rgb, uint8_t *out_rgb8, rt_stats *stats) {
    return render_frame(scene, p, out_rgb, out_rgb8, stats, nullptr);
}

// ---- resumable renders (include/rtamd.h: rt_accum_*) ---------------------------------------------------------------------
// The state lives in one device allocation indexed by pixel slot of the shard (RenderView::accum, device/rt_wavefront.h
// accum_enter / accum_leave): it belongs to the rt_accum, not to the scene's path records, so passes, phases, re-deals and
// other renders on the scene do not touch it.  The blob of rt_accum_save is a 128-byte header and that allocation, verbatim.
// struct rt_accum and the header are in host/rt_accum_state.h, shared with rtamd_multi.hip (rt_multi_accum_*).
// Geometry of a resumable frame from its params (host only); false with `err` set for params no rt_accum can be made of.
static bool accum_geometry(const rt_render_params *p, RenderView &R, uint32_t &n_pixslots, std::string &err) {
    if (!p) { err = "null params"; return false; }
    if (p->struct_size != sizeof(rt_render_params)) { err = "struct_size mismatch (ABI skew)"; return false; }
    if (p->reserved != 0) { err = "reserved must be 0"; return false; }
    if (p->integrator != RT_INTEGRATOR_HW8 && p->integrator != RT_INTEGRATOR_HW7 && p->integrator != RT_INTEGRATOR_HW6) { err = "resumable renders exist for RT_INTEGRATOR_HW6 / HW7 / HW8 only"; return false; }
    rt_render_params q = *p;
    q.samples = 1; // ignored here
    if (!resolve_tiles(&q, R, err)) return false;
    if (R.ray_depth > max_ray_depth[p->integrator]) { err = "ray_depth above the integrator's limit"; return false; }
    const uint64_t slots = (uint64_t)R.n_shard_tiles * (uint64_t)((R.tile_w >> 3) * (R.tile_h >> 3)) * 64u;
    if (slots >= 0x40000000ull) { err = "too many pixel slots"; return false; }
    n_pixslots = (uint32_t)slots;
    return true;
}

size_t rt_accum_state_bytes(const rt_render_params *p) {
    size_t bytes = 0; // what a refusal answers
    guarded("rt_accum_state_bytes: ", [&]() -> int {
        RenderView R{};
        uint32_t n = 0;
        std::string err;
        if (!accum_geometry(p, R, n, err)) return fail(RT_ERR_INVALID_ARG, "rt_accum_state_bytes: " + err);
        bytes = (size_t)ACCUM_HEADER_BYTES + (size_t)n * ACCUM_SLOT_BYTES;
        return RT_OK;
    });
    return bytes;
}

int rt_accum_create(rt_scene *scene, const rt_render_params *p, rt_accum **out) {
    if (!scene || !p || !out) return fail(RT_ERR_INVALID_ARG, "rt_accum_create: null argument");
    *out = nullptr;
    return guarded("rt_accum_create: ", [&]() -> int {
    if (p->struct_size == sizeof(rt_render_params)) {
        if (p->sample_streams > 1) return fail(RT_ERR_UNSUPPORTED, std::string("rt_accum_create: ") + accum_unsupported(Pipeline::Persistent8, p));
        if (p->integrator >= RT_INTEGRATOR_HW1 && p->integrator <= RT_INTEGRATOR_HW5) return fail(RT_ERR_UNSUPPORTED, std::string("rt_accum_create: ") + accum_unsupported(Pipeline::Hw1, p));
    }
    std::unique_ptr<rt_accum> a(new rt_accum);
    std::string err;
    if (!accum_geometry(p, a->view, a->n_pixslots, err)) return fail(RT_ERR_INVALID_ARG, "rt_accum_create: " + err);
    const bool hw7 = p->integrator == RT_INTEGRATOR_HW7;
    if (scene->flavor == RT_INTEGRATOR_HW3 || (p->integrator != scene->flavor && !(hw7 && scene->flavor == RT_INTEGRATOR_HW8)))
        return fail(RT_ERR_INVALID_ARG, "rt_accum_create: this scene was prepared for integrator " + std::to_string(scene->flavor));
    bool rounds_chosen = false;
    a->view.samples = 1;
    const Pipeline pipe = choose_pipeline(scene, p->integrator, a->view, a->n_pixslots / 64u, 1, rounds_chosen);
    if (const char *why = accum_unsupported(pipe, p)) return fail(RT_ERR_UNSUPPORTED, std::string("rt_accum_create: ") + why);
    a->scene = scene; a->params = *p; a->params.samples = 0;
    a->sample_limit = pipe == Pipeline::Persistent6 ? 1 << 24 : 1 << 25; // sample index bits of p6_pack / wf_pack
    HIP_CHECK(hipSetDevice(scene->device));
    hipStream_t stream = (hipStream_t)p->stream;
    HIP_CHECK(hipMalloc((void **)&a->d_state, (size_t)(a->n_pixslots ? a->n_pixslots : 1u) * ACCUM_SLOT_BYTES));
    if (a->n_pixslots) {
        RenderView R = a->view;
        R.accum = a->d_state; R.n_pixslots = a->n_pixslots;
        hipLaunchKernelGGL(dev::accum_seed_kernel, dim3((a->n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    *out = a.release();
    return RT_OK;
    });
}

void rt_accum_destroy(rt_accum *a) {
    if (a) (void)hipSetDevice(a->scene->device);
    delete a;
}

int rt_accum_samples(const rt_accum *a) {
    if (!a) return fail(RT_ERR_INVALID_ARG, "rt_accum_samples: null argument");
    return a->samples;
}

extern "C++" {
// what can be refused is refused before anything is launched: the state stays as it was
int rtamd::accum_check_slice(const rt_accum *a, int32_t n_samples, const std::string &who) {
    if (!a) return fail(RT_ERR_INVALID_ARG, who + "null argument");
    if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, who + "an earlier slice failed and left the state half advanced (" + a->broken + ")");
    if (n_samples <= 0) return fail(RT_ERR_INVALID_ARG, who + "n_samples must be positive");
    if ((int64_t)a->samples + n_samples >= (int64_t)a->sample_limit)
        return fail(RT_ERR_LIMIT, who + std::to_string(a->samples) + " + " + std::to_string(n_samples) + " samples per pixel do not fit the path records' sample index (below " + std::to_string(a->sample_limit) + ")");
    RenderView R = a->view;
    R.samples = a->samples + n_samples;
    bool rounds_chosen = false;
    if (const char *why = accum_unsupported(choose_pipeline(a->scene, a->params.integrator, R, a->n_pixslots / 64u, 1, rounds_chosen), &a->params)) return fail(RT_ERR_UNSUPPORTED, who + why);
    return RT_OK;
}
}

int rt_accum_render(rt_accum *a, int32_t n_samples, rt_stats *stats) {
    return guarded("rt_accum_render: ", [&]() -> int {
        if (const int rc = accum_check_slice(a, n_samples, "rt_accum_render: ")) return rc;
        rt_render_params p = a->params;
        p.samples = n_samples;
        const AccumSlice slice{a->d_state, a->samples};
        const int rc = render_frame(a->scene, &p, nullptr, nullptr, stats, &slice);
        if (rc != RT_OK) { a->broken = rt_last_error(); return rc; } // the slice failed under way: the state is half advanced
        a->samples += n_samples;
        return RT_OK;
    });
}

int rt_accum_resolve(rt_accum *a, uint32_t flags, float *out_rgb, uint8_t *out_rgb8) {
    if (!a) return fail(RT_ERR_INVALID_ARG, "rt_accum_resolve: null argument");
    return guarded("rt_accum_resolve: ", [&]() -> int {
        if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, "rt_accum_resolve: an earlier slice failed and left the state half advanced (" + a->broken + ")");
        if (flags & ~RT_FLAG_OUT_DEVICE) return fail(RT_ERR_INVALID_ARG, "rt_accum_resolve: flags other than RT_FLAG_OUT_DEVICE");
        if (a->samples <= 0) return fail(RT_ERR_INVALID_ARG, "rt_accum_resolve: no samples yet (a picture needs at least one)");
        HIP_CHECK(hipSetDevice(a->scene->device));
        hipStream_t stream = (hipStream_t)a->params.stream;
        RenderView R = a->view;
        const size_t elems = R.shard_count > 1 ? (size_t)R.n_shard_tiles * R.tile_w * R.tile_h * 3 : (size_t)R.width * R.height * 3;
        StagedOut rgb(out_rgb, flags, elems, sizeof(float)), rgb8(out_rgb8, flags, elems, 1);
        R.out_rgb = (float *)rgb.dev; R.out_rgb8 = (uint8_t *)rgb8.dev;
        R.accum = a->d_state; R.n_pixslots = a->n_pixslots;
        R.samples = a->samples;
        R.inv_samples = (float)(1.0 / a->samples); // scene.cpp:176, as rt_render(samples = d) evaluates it
        if (a->n_pixslots && (out_rgb || out_rgb8)) {
            hipLaunchKernelGGL(dev::accum_resolve_kernel, dim3((a->n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
            HIP_CHECK(hipGetLastError());
        }
        rgb.copy_back(stream);
        rgb8.copy_back(stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        return RT_OK;
    });
}

int rt_accum_save(rt_accum *a, void *blob, size_t capacity) {
    if (!a || !blob) return fail(RT_ERR_INVALID_ARG, "rt_accum_save: null argument");
    return guarded("rt_accum_save: ", [&]() -> int {
        if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, "rt_accum_save: an earlier slice failed and left the state half advanced (" + a->broken + ")");
        const size_t state = (size_t)a->n_pixslots * ACCUM_SLOT_BYTES;
        if (capacity < ACCUM_HEADER_BYTES + state) return fail(RT_ERR_INVALID_ARG, "rt_accum_save: buffer smaller than rt_accum_state_bytes");
        HIP_CHECK(hipSetDevice(a->scene->device));
        hipStream_t stream = (hipStream_t)a->params.stream;
        uint32_t h[ACCUM_HEADER_BYTES / 4];
        accum_header(a, h);
        memcpy(blob, h, ACCUM_HEADER_BYTES);
        if (state) HIP_CHECK(hipMemcpyAsync((uint8_t *)blob + ACCUM_HEADER_BYTES, a->d_state, state, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return RT_OK;
    });
}

int rt_accum_load(rt_accum *a, const void *blob, size_t size) {
    if (!a || !blob) return fail(RT_ERR_INVALID_ARG, "rt_accum_load: null argument");
    return guarded("rt_accum_load: ", [&]() -> int {
        if (!a->broken.empty()) return fail(RT_ERR_INVALID_ARG, "rt_accum_load: an earlier slice failed and left the state half advanced (" + a->broken + ")");
        uint32_t want[ACCUM_HEADER_BYTES / 4];
        accum_header(a, want);
        const size_t state = (size_t)a->n_pixslots * ACCUM_SLOT_BYTES;
        const int samples = accum_check_blob(want, blob, size, a->sample_limit, state, "rt_accum_load: ");
        if (samples < 0) return samples;
        HIP_CHECK(hipSetDevice(a->scene->device));
        hipStream_t stream = (hipStream_t)a->params.stream;
        a->loads++; // from here on the state is being replaced: the batches of a noise monitor end here
        if (state) HIP_CHECK(hipMemcpyAsync(a->d_state, (const uint8_t *)blob + ACCUM_HEADER_BYTES, state, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        a->samples = samples;
        return RT_OK;
    });
}

} // extern "C"

// ---- batched ray queries: the launches of one chunk (device/rt_query.h; the host side is rtamd_query.hip) -------------------------------
// The geometry of the round pipeline's traverse launch at its defaults: RQ_BLOCKS_PER_CU blocks of 256 per CU with 30 KB of stack columns
// each, refill at 16 idle lanes, leaf batch 20 or 112/256 of the active lanes, a quarter of the list handed out dynamically; fewer blocks
// when the chunk has fewer rays than their lanes.  Not tuned for the queries (profiles/r20_ray_queries.txt).
namespace {

struct QueryGeometry { SceneView V; int lds_limit; bool spill_scene, deep_lights; unsigned walk_blocks, flat_blocks, exact_blocks; };

QueryGeometry query_geometry(const rt_scene *scene, uint32_t n) {
    QueryGeometry G;
    G.V = scene->view;
    if (G.V.exact_boxes != 1u) { G.V.exact_boxes = 0u; G.V.n_tripwire_groups = 0u; G.V.cull_k = 4.8e-7f; } // no gate: the tie tolerance only, as check_frame sets it
    G.lds_limit = WF_STACK;
    G.spill_scene = scene->info.bvh_depth > (uint32_t)WF_STACK;
    G.deep_lights = scene->info.light_bvh_depth > (uint32_t)WF_STACK;
    const unsigned need = (n + 255u) / 256u;
    G.walk_blocks = std::max(1u, std::min((unsigned)scene->n_cus * RQ_BLOCKS_PER_CU, need));
    G.flat_blocks = std::max(1u, std::min((unsigned)scene->n_cus * 16u, need));
    G.exact_blocks = std::max(1u, std::min((unsigned)scene->n_cus, (n + 63u) / 64u));
    return G;
}
const int rq_refill = WF_REFILL, rq_leaf_batch = WF_LEAF_BATCH | (112 << 16), rq_dyn = 64;

// RTAMD_WF_LDS_STACK=n (testing), as the round pipeline takes it: the occlusion walk pretends its LDS stacks hold only n entries, so an
// ordinary scene runs the SPILL variant.  The closest-hit and light-pdf launches keep WF_STACK.
int query_lds_limit() {
    const int limit = env_int("RTAMD_WF_LDS_STACK", WF_STACK);
    return limit < 1 || limit >= WF_STACK ? WF_STACK : limit;
}

} // namespace

size_t rtamd::query_ovf_words(const rt_scene *scene) {
    return scene->info.bvh_depth > (uint32_t)query_lds_limit() ? (size_t)scene->n_cus * RQ_BLOCKS_PER_CU * 256u * WF_OVF : 0u;
}

uint32_t rtamd::query_launch_closest(const rt_scene *scene, const QueryView &Q, hipStream_t stream) {
    const QueryGeometry G = query_geometry(scene, Q.n);
    hipLaunchKernelGGL(dev::rq_classify_kernel<false>, dim3(G.flat_blocks), dim3(256), 0, stream, G.V, Q, 0u);
    uint32_t launches = 2;
    if (!Q.reference_walk) {
        if (G.spill_scene) hipLaunchKernelGGL(dev::rq_closest_kernel<true>, dim3(G.walk_blocks), dim3(256), 0, stream, G.V, Q, rq_refill, rq_leaf_batch, rq_dyn, G.lds_limit);
        else hipLaunchKernelGGL(dev::rq_closest_kernel<false>, dim3(G.walk_blocks), dim3(256), 0, stream, G.V, Q, rq_refill, rq_leaf_batch, rq_dyn, G.lds_limit);
        hipLaunchKernelGGL(dev::rq_resolve_kernel, dim3(G.flat_blocks), dim3(256), 0, stream, G.V, Q);
        launches += 2;
    }
    hipLaunchKernelGGL(dev::rq_closest_exact_kernel, dim3(G.exact_blocks), dim3(64), 0, stream, G.V, Q);
    HIP_CHECK(hipGetLastError());
    return launches;
}

uint32_t rtamd::query_launch_light_pdf(const rt_scene *scene, const QueryView &Q, hipStream_t stream) {
    const QueryGeometry G = query_geometry(scene, Q.n);
    const bool lean = !Q.reference_walk && !G.deep_lights;
    hipLaunchKernelGGL(dev::rq_classify_kernel<true>, dim3(G.flat_blocks), dim3(256), 0, stream, G.V, Q, lean ? 0u : 1u);
    if (lean) hipLaunchKernelGGL(dev::rq_light_kernel, dim3(G.walk_blocks), dim3(256), 0, stream, G.V, Q, rq_refill, rq_leaf_batch, rq_dyn);
    hipLaunchKernelGGL(dev::rq_light_exact_kernel, dim3(G.exact_blocks), dim3(64), 0, stream, G.V, Q);
    HIP_CHECK(hipGetLastError());
    return lean ? 3u : 2u;
}

uint32_t rtamd::query_launch_occluded(const rt_scene *scene, const QueryView &Q, hipStream_t stream) {
    QueryGeometry G = query_geometry(scene, Q.n);
    G.lds_limit = query_lds_limit();
    G.spill_scene = scene->info.bvh_depth > (uint32_t)G.lds_limit;
    hipLaunchKernelGGL(dev::rq_classify_occluded_kernel, dim3(G.flat_blocks), dim3(256), 0, stream, G.V, Q);
    uint32_t launches = 2;
    if (!Q.reference_walk) {
        if (G.spill_scene) hipLaunchKernelGGL(dev::rq_any_kernel<true>, dim3(G.walk_blocks), dim3(256), 0, stream, G.V, Q, rq_refill, rq_leaf_batch, rq_dyn, G.lds_limit);
        else hipLaunchKernelGGL(dev::rq_any_kernel<false>, dim3(G.walk_blocks), dim3(256), 0, stream, G.V, Q, rq_refill, rq_leaf_batch, rq_dyn, G.lds_limit);
        hipLaunchKernelGGL(dev::rq_any_resolve_kernel, dim3(G.flat_blocks), dim3(256), 0, stream, G.V, Q);
        launches += 2;
    }
    hipLaunchKernelGGL(dev::rq_any_exact_kernel, dim3(G.exact_blocks), dim3(64), 0, stream, G.V, Q);
    HIP_CHECK(hipGetLastError());
    return launches;
}

// The first-hit layer (device/rt_query_surface.h): flat launches, one lane per record.
uint32_t rtamd::query_launch_material_table(const rt_scene *scene, uint32_t *table, hipStream_t stream) {
    const uint32_t n = scene->view.n_tris;
    if (!n) return 0u;
    hipLaunchKernelGGL(dev::rq_material_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, scene->view, table);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_surface(const rt_scene *scene, const SurfaceView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_surface_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_environment(const rt_scene *scene, const EnvironmentView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_environment_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_camera_rays(const rt_scene *scene, const CameraView &V, hipStream_t stream) {
    CameraView C = V;
    C.tan_fov_x = frame_tan_fov_x(scene->view, V.width, V.height);
    hipLaunchKernelGGL(dev::rq_camera_rays_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, C);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_guides(const rt_scene *scene, const GuidesView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_guides_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

// The bounce step (device/rt_query_scatter.h): flat launches, one lane per record; the light walk between them is query_launch_light_pdf.
uint32_t rtamd::query_launch_scatter_sample(const rt_scene *scene, const ScatterView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_scatter_sample_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_scatter_finish(const rt_scene *scene, const ScatterView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_scatter_finish_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_bsdf_rays(const rt_scene *scene, const ScatterView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_bsdf_rays_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_bsdf_finish(const rt_scene *scene, const ScatterView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_bsdf_finish_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_path_advance(const rt_scene *scene, const PathView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_path_advance_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

// The baker (device/rt_bake.h): flat launches, one lane per record, per slot, per float of the answer.
uint32_t rtamd::query_launch_bake_rays(const rt_scene *scene, const BakeView &B, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_bake_rays_kernel, dim3(query_geometry(scene, B.n).flat_blocks), dim3(256), 0, stream, scene->view, B);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_bake_advance(const rt_scene *scene, const PathView &V, const BakeView &B, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_bake_advance_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, scene->view, V, B);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_bake_resolve(const rt_scene *scene, const BakeView &B, hipStream_t stream) {
    hipLaunchKernelGGL(dev::rq_bake_resolve_kernel, dim3(query_geometry(scene, B.n).flat_blocks), dim3(256), 0, stream, scene->view, B);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

// ---- rt_render_paths / rt_render_bake / rt_render_probes: a caller's paths through the persistent hw8 kernel (device/rt_path_source.h) -------
uint32_t rtamd::query_launch_source_pack(const rt_scene *scene, const SourceView &V, hipStream_t stream) {
    hipLaunchKernelGGL(V.mode == PT_SRC_PROBES ? dev::rq_probes_pack_kernel : dev::rq_source_pack_kernel, dim3(query_geometry(scene, V.n_pixslots).flat_blocks), dim3(256), 0, stream, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

uint32_t rtamd::query_launch_source_unpack(const rt_scene *scene, const SourceView &V, hipStream_t stream) {
    hipLaunchKernelGGL(V.mode == PT_SRC_PROBES ? dev::rq_probes_unpack_kernel : dev::rq_source_unpack_kernel, dim3(query_geometry(scene, V.n).flat_blocks), dim3(256), 0, stream, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}

namespace {
// The strip frame of `slots` record indices (device/rt_path_source.h): 8 pixels wide, one 8x8 sub-tile per 64 slots, unsharded.
rt_render_params source_params(uint32_t slots, int32_t ray_depth, int32_t samples) {
    rt_render_params p{};
    p.struct_size = sizeof(rt_render_params);
    p.width = 8; p.height = 8 * (int32_t)((slots + 63u) / 64u);
    p.samples = samples; p.ray_depth = ray_depth;
    p.integrator = RT_INTEGRATOR_HW8;
    return p;
}
int source_frame(const rt_scene *scene, const rt_render_params &p, const AccumSlice &slice, const std::string &who, Frame &F) {
    if (const int rc = check_frame(scene, &p, &slice, who, F)) return rc;
    if (F.pipe != Pipeline::Persistent8)
        return fail(RT_ERR_UNSUPPORTED, who + "the persistent hw8 kernel does not take this scene or environment (RTAMD_KERNEL=wavefront|mega, or a tree beyond its stack columns): there is no fallback, rt_trace_paths / rt_bake serve it");
    return RT_OK;
}
} // namespace

int rtamd::source_check(const rt_scene *scene, uint32_t slots, int32_t ray_depth, int32_t samples, const std::string &who) {
    Frame F;
    return source_frame(scene, source_params(slots, ray_depth, samples), AccumSlice{nullptr, 0}, who, F);
}

int rtamd::source_render(rt_scene *scene, const SourceChunk &C, hipStream_t stream, SourceResult &res, const std::string &who) {
    const rt_render_params p = source_params(C.n, C.ray_depth, C.samples);
    const AccumSlice slice{C.state, 0};
    Frame F;
    if (const int rc = source_frame(scene, p, slice, who, F)) return rc;
    const double t0 = now_ms();
    F.R.src_mode = C.mode; F.R.src_n = C.n; F.R.src_rays = C.rays; F.R.src_points = C.points; F.R.src_streams = C.streams;
    if (C.mode == PT_SRC_PROBES) F.R.src_sh = C.sh; // shares its room with src_rays (RenderView), which mode 3 has none of
    if (C.mode == PT_SRC_PIXELS) { // likewise: the pixel words, and the real frame's constants where the points and streams of modes 2 and 3 are
        F.R.src_pixels = C.pixels;
        F.R.src_frame[0] = C.frame_w; F.R.src_frame[1] = C.frame_h;
        F.R.src_tan_fov_x = frame_tan_fov_x(scene->view, C.frame_w, C.frame_h);
    }
    if (C.mode == PT_SRC_VIEWS) { // the pixel and view words, the cameras where the points are, the views' frame where the streams are
        F.R.src_pixels = C.pixels;
        F.R.src_cameras = C.cameras;
        F.R.src_wh = (uint32_t)C.frame_w | ((uint32_t)C.frame_h << 16);
    }
    launch_frame(scene, &p, F, stream, true);
    rt_stats st{};
    if (const int rc = collect_frame(scene, F, stream, &st, t0, who)) return rc;
    unsigned long long no_path = 0;
    HIP_CHECK(hipMemcpy(&no_path, scene->d_counters + CNT_SRC_NO_PATH, sizeof no_path, hipMemcpyDeviceToHost)); // the launch is over (collect_frame waited)
    res.kernel_ms = st.kernel_ms; res.launches = st.launches; res.reference_exact = st.reference_exact;
    res.exact_walks = st.exact_closest_hits + st.exact_light_sums; res.no_path = no_path;
    return RT_OK;
}

// ---- rt_adaptive_*: the flat kernels around the pixel source (device/rt_adaptive.h; the host side is rtamd_adaptive.hip) ---------------------
namespace {
template <class K> uint32_t adaptive_launch(K kernel, const rt_scene *scene, uint32_t lanes, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    if (!lanes) return 0u;
    hipLaunchKernelGGL(kernel, dim3(query_geometry(scene, lanes).flat_blocks), dim3(256), 0, stream, R, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}
} // namespace

uint32_t rtamd::adaptive_launch_gather(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    return adaptive_launch(dev::ad_gather_kernel, scene, V.strip_slots, R, V, stream);
}
uint32_t rtamd::adaptive_launch_scatter(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    return adaptive_launch(dev::ad_scatter_kernel, scene, V.n_list * 64u, R, V, stream);
}
uint32_t rtamd::adaptive_launch_resolve(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    return adaptive_launch(dev::ad_resolve_kernel, scene, R.n_pixslots, R, V, stream);
}
uint32_t rtamd::adaptive_launch_update(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    return adaptive_launch(dev::ad_update_kernel, scene, V.n_list * 64u, R, V, stream);
}
uint32_t rtamd::adaptive_launch_estimate(const rt_scene *scene, const RenderView &R, const AdaptiveView &V, hipStream_t stream) {
    return adaptive_launch(dev::ad_estimate_kernel, scene, R.n_pixslots, R, V, stream);
}
void rtamd::adaptive_launch_seed(const rt_scene *, const RenderView &R, hipStream_t stream) {
    if (!R.n_pixslots) return;
    hipLaunchKernelGGL(dev::accum_seed_kernel, dim3((R.n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
    HIP_CHECK(hipGetLastError());
}
float rtamd::adaptive_tan_fov_x(const rt_scene *scene, int32_t width, int32_t height) { return frame_tan_fov_x(scene->view, width, height); }

// ---- rt_views_*: the flat kernels around the view source (device/rt_views.h; the host side is rtamd_views.hip) -------------------------------
uint32_t rtamd::views_launch_gather(const rt_scene *scene, const RenderView &R, const ViewsView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::vw_gather_kernel, dim3(query_geometry(scene, V.strip_slots).flat_blocks), dim3(256), 0, stream, R, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}
uint32_t rtamd::views_launch_scatter(const rt_scene *scene, const RenderView &R, const ViewsView &V, hipStream_t stream) {
    hipLaunchKernelGGL(dev::vw_scatter_kernel, dim3(query_geometry(scene, V.strip_slots).flat_blocks), dim3(256), 0, stream, R, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}
void rtamd::views_launch_seed(const rt_scene *, const RenderView &R, hipStream_t stream) {
    hipLaunchKernelGGL(dev::accum_seed_kernel, dim3((R.n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
    HIP_CHECK(hipGetLastError());
}
void rtamd::views_launch_resolve(const rt_scene *, const RenderView &R, hipStream_t stream) {
    hipLaunchKernelGGL(dev::accum_resolve_kernel, dim3((R.n_pixslots + 255u) / 256u), dim3(256), 0, stream, R);
    HIP_CHECK(hipGetLastError());
}

// ---- rt_view_adaptive_*: the flat kernels around the view source over a strip of sub-tiles (device/rt_view_adaptive.h; the host side is
// rtamd_view_adaptive.hip) -------------------------------------------------------------------------------------------------------------
namespace {
template <class K> uint32_t view_adaptive_launch(K kernel, const rt_scene *scene, uint32_t lanes, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    if (!lanes) return 0u;
    hipLaunchKernelGGL(kernel, dim3(query_geometry(scene, lanes).flat_blocks), dim3(256), 0, stream, R, V);
    HIP_CHECK(hipGetLastError());
    return 1u;
}
} // namespace

uint32_t rtamd::view_adaptive_launch_gather(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    return view_adaptive_launch(dev::va_gather_kernel, scene, V.strip_slots, R, V, stream);
}
uint32_t rtamd::view_adaptive_launch_scatter(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    return view_adaptive_launch(dev::va_scatter_kernel, scene, V.n_list * 64u, R, V, stream);
}
uint32_t rtamd::view_adaptive_launch_update(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    return view_adaptive_launch(dev::va_update_kernel, scene, V.n_list * 64u, R, V, stream);
}
uint32_t rtamd::view_adaptive_launch_estimate(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    return view_adaptive_launch(dev::va_estimate_kernel, scene, V.count * 64u, R, V, stream);
}
uint32_t rtamd::view_adaptive_launch_resolve(const rt_scene *scene, const RenderView &R, const ViewAdaptiveView &V, hipStream_t stream) {
    return view_adaptive_launch(dev::va_resolve_kernel, scene, R.n_pixslots, R, V, stream);
}

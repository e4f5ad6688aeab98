// Persistent dataflow form of the hw8 replay path tracer: ONE launch renders the frame, no rounds and no global barrier.
//
// The reference's per-pixel loop (hw8/src/scene.cpp:84-177) is a chain of dependent stages per pixel — closest hit
// (bvh.h:111-142) -> shade / sample (scene.cpp:99-156) -> light-pdf sum (distributions.h:148-165) -> throughput update
// (scene.cpp:158-164) -> next bounce or next sample — and the chain of one pixel never depends on another pixel's.  The
// round-based pipeline of rt_wavefront.h runs each stage as a kernel over all pixels and pays a machine-wide drain at every
// kernel boundary (the launch ends with its longest walk).  Here the dependency is kept PER PATH:
//
//   * five 4-wave workgroups per CU (one wave per SIMD each: five waves per SIMD at <= 96 VGPRs) each own a fixed, interleaved
//     share of the pixel slots (8x8 sub-tiles dealt round-robin to the workgroups); the path records stay in HBM in the layout
//     of rt_wavefront.h, but only this workgroup touches them, so hand-offs between its waves need workgroup-scope ordering
//     only (one CU, one L1: `s_waitcnt` + LDS);
//   * the stage a path waits for is one bit per path in an LDS bitmap (need_trace / need_light / need_shade / ...); a wave
//     that wants work claims set bits with LDS atomics (one word per lane, rotating cursor: round-robin service, no
//     capacity limit, no ring to overflow);
//   * every wave picks a role when it is idle (the scheduler loop of pt_run, the one kernel body of this file's kernel and of
//     rt_persistent_hw6.h's): closest-hit walker, light-sum walker or shader, by the populations of the bitmaps; walkers keep
//     their lanes full by refilling idle lanes from the bitmap; a shader takes up to 64 paths, finishes their pending bounce,
//     shades the new hit and sets the bits of what each path needs next;
//   * the walkers read four-wide nodes on a 16-bit grid (rt_types.h GpuNode4Q: two tree levels per 64-byte fetch, the ray in grid
//     coordinates), park the leaves they meet for a common leaf phase, and leave what only a few lanes need (a light hit's pdf
//     term, the record of a walk that has ended) for once per pass;
//   * the speculative pairing of rt_wavefront.h is kept: a bounce's sampled direction is traced for the next hit at the
//     same time as its light-pdf sum is walked; a 2-bit "pending" field per path joins the two (whoever finishes last sets
//     need_shade).
//
// What this removes: 3 x spp x depth kernel launches, the global queue atomics, the per-round drain (every launch of the round
// pipeline waited for its longest walk), and the idle memory system during traversal / idle ALUs during shading (the roles
// overlap on every CU).  A path advances as fast as its own chain allows, which is what lets a small frame (a shard of a
// multi-GPU render) run near the full rate.
//
// Reference-exact box decisions (hw8/src/primitives.cpp:29-53,163-165).  The walkers prune with a cheap conservative test on
// padded boxes, so they find a superset of the triangles the reference's own slab test lets through.  A hit is accepted
// as it stands when the hit point lies robustly inside its triangle's box (pt_box_robust: then every ancestor box passes the
// reference's test whatever the rounding) and no second triangle was hit within a few ulp of it; the rare others are walked
// again by the `exact` role with the reference's arithmetic on the unpadded boxes of the reference tree (ref_closest_hit,
// ref_light_pdf_sum).  Pixels then match the reference's also where a ray grazes a box corner.  Rays that cross a tripwire (rt_exact.h
// pt_tripwire: the leaf box of a triangle whose test accepts points far away from it) never go to the walkers at all.
#pragma once
#include "rt_path_source.h" // the first ray of a sample under WF_FEAT_SOURCE; brings rt_wavefront.h
#include "rt_pt_queue.h" // the queues: pt_count, pt_ballot, pt_rank_below, pt_prefix, pt_pop, pt_push; PT_NONE

namespace rtamd {
namespace dev {

// hw8 / hw7: workgroups of FOUR waves (one per SIMD), FIVE resident per CU = five waves per SIMD.  That takes <= 96 VGPRs per wave (no
// scratch), 24-entry stack columns (4 x 24 x 256 B = 24 KB per workgroup) and 1.4 bytes of LDS per path for bitmaps and group tables: 31.7 KB per
// workgroup, five of which fill the CU's 160 KB (handed out in 1,280-byte granules: 25 granules each).
#define P8_WAVES 4
#define P8_THREADS (64 * P8_WAVES)
#define P8_PER_CU 5
#define PT_MAX_PATHS 5120             // paths per workgroup (bitmap capacity in LDS): x 1,280 workgroups = 6.5 M (a 3840x2160 frame on one GPU: two passes)
#define PT_MIN_GROUP 16               // smallest group of the deal (group_shift 4): the LDS tables are sized for it
#define PT_NW (PT_MAX_PATHS / 32)
#define PT_BIT_T 1u                   // pending: closest-hit walk outstanding
#define PT_BIT_L 2u                   // pending: light-pdf sum outstanding
// indices into PtShared::need / PtShared::cnt
#define PT_Q_TRACE 0
#define PT_Q_LIGHT 1
#define PT_Q_SHADE 2
#define PT_Q_XLIGHT 3                 // light sums for the exact walk (more than WF_MAX_LIGHT_HITS hits, or a hit at a box boundary)
#define PT_Q_XTRACE 4                 // closest hits for the exact walk
#define PT_N_LIVE 5                   // cnt only: pixels of this workgroup not finished yet
#define PT_W_TRACE 6                  // cnt only: waves currently walking closest hits / light sums
#define PT_W_LIGHT 7
#define PT_GSHIFT 15                  // cnt only: PtParams::group_shift (constant during the launch)
// What a sub-tile costs its workgroup, in units of one closest-hit node step (wave time by role over steps by role on the benchmark
// scene): the measure the frame is re-dealt by after its first phase.  Counting shaded hits alone misses the rays that hit nothing.
#define PT_COST_TRACE_NODE 1u     // a node visit of a closest-hit walk
#define PT_COST_TRACE_TRI 1u      // a triangle test of a closest-hit walk
#define PT_COST_LIGHT_NODE 2u     // a node visit of a light-sum walk
#define PT_COST_LIGHT_TEST 2u     // a light test of a light-sum walk
#define PT_COST_SHADE 14u
#define PT_DEBUG_BLOCKS 2048           // RTAMD_DEBUG_COUNTERS: workgroups whose start / exit times are recorded (>= 256 CUs x 5)
#define PT_DRAINED 0xFFFFFFFEu        // `cur` of a lane whose stack is empty and whose last leaf is still to be tested (reads as a leaf: the lane waits)
// `cur` of a lane that walks nothing: just below the leaf bit and above every node index (an array of 64-byte nodes below 4 GiB has fewer than
// 2^26), so that one compare tells an inner node from all the rest and the leaf bit alone tells who waits for a leaf phase.
#define PT_IDLE 0x7FFFFFFDu           // no walk
#define PT_FULL 0x7FFFFFFEu           // the walk is over, its stack column could not take a node's children: full() and end() are due
#define PT_ENDED 0x7FFFFFFFu          // the walk is over: its end() is due
RT_DEV bool pt_is_inner(uint32_t cur) { return cur < PT_IDLE; }
RT_DEV bool pt_is_ending(uint32_t cur) { return (int32_t)cur > (int32_t)PT_IDLE; } // PT_FULL or PT_ENDED (leaves are negative)
#define PT_T_OVERFLOW (-1.f)          // t of a closest-hit record whose walk ran out of stack: the exact role redoes the query
// ---- one step of a walk over the four-wide grid nodes (rt_types.h GpuNode4Q), shared with rt_persistent_hw6.h ------------------------
// A step yields the lane's next `cur`: the child to visit (the others wait in the lane's stack column), or, when no child is entered, what
// pt_pop_or_end gives, or PT_FULL when the column cannot take the children that would wait (nothing is pushed then).
//
// pt_pop_or_end: what a lane with nothing at hand visits next — the top of its column; with an empty column the walk is over (PT_ENDED),
// unless leaves are parked (`parked`): those are tested first (PT_DRAINED).
RT_DEV uint32_t pt_pop_or_end(uint32_t (*stack)[64], int lane, int &sp, bool parked) {
    if (sp != 0) return stack[--sp][lane];
    return parked ? PT_DRAINED : PT_ENDED;
}
// sort key of a child: its entry distance's (rt_device.h slab_enter_q), or the last of all for one that is not entered
RT_DEV uint32_t pt_near_key(bool entered, uint32_t key) { return entered ? key : 0xFFFFFFFFu; }
// compare-exchange of (key, child word) pairs: the smaller key first
RT_DEV void pt_order(uint32_t &ka, uint32_t &ca, uint32_t &kb, uint32_t &cb) {
    const bool s = kb < ka;
    const uint32_t k = s ? kb : ka, c = s ? cb : ca;
    kb = s ? ka : kb; cb = s ? ca : cb;
    ka = k; ca = c;
}
// The four records of wide node `cur`.  NODES: the node array as the kernel holds it, a plain pointer (rt_persistent_hw6.h) or a GlobalBytes
// (this file's walkers: one 64-byte node at byte cur << 6 of an array below 4 GiB).
RT_DEV void pt_node_records(const GpuNode4Q *nodes, uint32_t cur, uint4 &b0, uint4 &b1, uint4 &b2, uint4 &b3) {
    const uint4 *q = reinterpret_cast<const uint4 *>(nodes + cur);
    b0 = q[0]; b1 = q[1]; b2 = q[2]; b3 = q[3];
}
RT_DEV void pt_node_records(const GlobalBytes nodes, uint32_t cur, uint4 &b0, uint4 &b1, uint4 &b2, uint4 &b3) {
    const uint32_t ofs = cur << 6;
    b0 = nodes.u4(ofs, 0u); b1 = nodes.u4(ofs, 1u); b2 = nodes.u4(ofs, 2u); b3 = nodes.u4(ofs, 3u);
}
// Closest-hit walks: the entered children nearest first — the nearest becomes `cur`, the others are pushed farthest first.
// `cap`: entries the column may hold.
template <class NODES>
RT_DEV uint32_t pt_wide_step_nearest(const NODES nodes, const RayGrid &ray, float cull_t, uint32_t (*stack)[64], int lane, int &sp, int cap, uint32_t cur, bool parked) {
    uint4 b0, b1, b2, b3;
    pt_node_records(nodes, cur, b0, b1, b2, b3);
    uint32_t k0, k1, k2, k3;
    const bool h0 = slab_enter_q(b0, ray, cull_t, k0), h1 = slab_enter_q(b1, ray, cull_t, k1);
    const bool h2 = slab_enter_q(b2, ray, cull_t, k2), h3 = slab_enter_q(b3, ray, cull_t, k3);
    k0 = pt_near_key(h0, k0); k1 = pt_near_key(h1, k1); k2 = pt_near_key(h2, k2); k3 = pt_near_key(h3, k3);
    uint32_t c0 = b0.w, c1 = b1.w, c2 = b2.w, c3 = b3.w;
    pt_order(k0, c0, k1, c1); pt_order(k2, c2, k3, c3); pt_order(k0, c0, k2, c2); pt_order(k1, c1, k3, c3); pt_order(k1, c1, k2, c2);
    const int nh = (int)h0 + (int)h1 + (int)h2 + (int)h3;
    if (nh == 0) return pt_pop_or_end(stack, lane, sp, parked);
    if (sp + nh - 1 > cap) return PT_FULL;
    if (nh > 3) stack[sp++][lane] = c3;
    if (nh > 2) stack[sp++][lane] = c2;
    if (nh > 1) stack[sp++][lane] = c1;
    return c0;
}
// Which records of wide node `cur` a light sum enters: the one decision of the light walker (pt_wide_step_all) and of the shader's
// settling of light sums (pt_light_reach), so that both take it with the same code.
template <class NODES>
RT_DEV void pt_wide_enter_all(const NODES nodes, uint32_t cur, const RayGrid &ray, uint4 &b0, uint4 &b1, uint4 &b2, uint4 &b3,
                              bool &h0, bool &h1, bool &h2, bool &h3) {
    pt_node_records(nodes, cur, b0, b1, b2, b3);
    h0 = slab_test_q(b0, ray); h1 = slab_test_q(b1, ray); h2 = slab_test_q(b2, ray); h3 = slab_test_q(b3, ray); // no entry distance: every entered child is walked
}
// The root of a tree is the same 64 bytes for every lane: read through the constant address space, i.e. by scalar loads, once for the wave.
struct PtRootNode { const GpuNode4Q *nodes; };
RT_DEV void pt_node_records(const PtRootNode root, uint32_t, uint4 &b0, uint4 &b1, uint4 &b2, uint4 &b3) {
    typedef const __attribute__((address_space(4))) GlobalBytes::Word4 *Q;
    const Q q = (Q)root.nodes;
    const GlobalBytes::Word4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    b0 = make_uint4(w0.x, w0.y, w0.z, w0.w); b1 = make_uint4(w1.x, w1.y, w1.z, w1.w); b2 = make_uint4(w2.x, w2.y, w2.z, w2.w); b3 = make_uint4(w3.x, w3.y, w3.z, w3.w);
}
// Light sums: every entered child is walked, in any order (the callers keep their hits sorted): the first one now, the others wait.
template <class NODES>
RT_DEV uint32_t pt_wide_step_all(const NODES nodes, const RayGrid &ray, uint32_t (*stack)[64], int lane, int &sp, int cap, uint32_t cur, bool parked) {
    uint4 b0, b1, b2, b3;
    bool h0, h1, h2, h3;
    pt_wide_enter_all(nodes, cur, ray, b0, b1, b2, b3, h0, h1, h2, h3);
    if (!(h0 || h1 || h2 || h3)) return pt_pop_or_end(stack, lane, sp, parked);
    // an entered child waits when one before it is entered too: decided on the lane masks of the four tests, no counting of hits
    const bool w3 = h3 && (h0 || h1 || h2), w2 = h2 && (h0 || h1), w1 = h1 && h0;
    if (sp + (int)w3 + (int)w2 + (int)w1 > cap) return PT_FULL;
    if (w3) stack[sp++][lane] = b3.w;
    if (w2) stack[sp++][lane] = b2.w;
    if (w1) stack[sp++][lane] = b1.w;
    return h0 ? b0.w : h1 ? b1.w : h2 ? b2.w : b3.w;
}
// The shader settles the light sums whose walk enters no record of the light tree's root (pt_light_reach < PT_LIGHT_SETTLE) instead of
// handing them to the light walker.
#define PT_LIGHT_SETTLE 1
// How far the light walker's walk of this ray would get before its first light test, taking the walker's own decisions
// (pt_wide_enter_all): 0 = it enters no record of the light tree's root; 1 = it enters inner nodes there but none of their records;
// 2 = it goes further (or LEVELS < 2 and it enters the root).  `steps`: the node steps that took.  A walk that ends at 0 or 1 tests no
// light, so its sum is exactly the walker's sum of no hits.
template <int LEVELS>
RT_DEV int pt_light_reach(const SceneView &S, const RayGrid &ray, int &steps) {
    uint4 b[4];
    bool h[4];
    const GlobalBytes nodes = global_bytes(S.light_walk_nodes4);
    pt_wide_enter_all(PtRootNode{S.light_walk_nodes4}, 0u, ray, b[0], b[1], b[2], b[3], h[0], h[1], h[2], h[3]);
    steps = 1;
    if (!(h[0] | h[1] | h[2] | h[3])) return 0;
    if (LEVELS < 2) return 2;
    for (int c = 0; c < 4; c++) {
        if (!h[c]) continue;
        if (b[c].w & RT_LEAF_BIT) return 2;                      // a leaf (or an unused record): the walker tests lights there
        uint4 g0, g1, g2, g3;
        bool e0, e1, e2, e3;
        pt_wide_enter_all(nodes, b[c].w, ray, g0, g1, g2, g3, e0, e1, e2, e3);
        steps++;
        if (e0 | e1 | e2 | e3) return 2;
    }
    return 1;
}
#define PT_EXACT_BATCH 16             // the exact role walks at most this many queries at once: their stacks (RT_STACK_SIZE entries each) share the wave's LDS stack area

struct PtShared {
    uint32_t stack[P8_WAVES][P8_STACK][64];   // per-lane traversal stack columns, one area per wave
    uint32_t need[5][PT_NW];
    uint32_t pending[PT_NW * 2];              // 2 bits per path
    uint32_t groups[PT_MAX_PATHS / PT_MIN_GROUP]; // local group -> group of the pass
    uint32_t cost[PT_MAX_PATHS / PT_MIN_GROUP];       // work done for each local group in this launch (PT_COST_*): the load measure the frame is re-dealt by
    int cnt[16];
};
static_assert(PT_EXACT_BATCH * RT_STACK_SIZE <= P8_STACK * 64, "the exact role's stacks must fit the wave's LDS stack area");
static_assert(sizeof(PtShared) <= (128 / P8_PER_CU) * 1280, "P8_PER_CU workgroups per CU: the CU's 128 LDS granules of 1,280 bytes shared evenly");

struct PtParams {
    uint32_t n_groups;                // groups of this pass: 2^group_shift consecutive path slots each
    uint32_t group_shift;             // 6: a group is an 8x8 sub-tile; 4: two rows of one (small frames: more, smaller units for the deal — a
                                      // workgroup should hold well over a dozen, and a heavy 8x8 sub-tile alone can outweigh a workgroup's fair share)
    // Which groups a workgroup owns: group_ids[group_ofs[b] .. group_ofs[b + 1]) when group_ofs is set (the host's re-deal after
    // the first phase of a frame), else b, b + n_blocks, b + 2 n_blocks, ...; `resume` = the paths carry on from their records
    // (a later phase) instead of being seeded; group_cost[g] receives the number of hits shaded for group g in this launch.
    const uint32_t *group_ofs, *group_ids;
    uint32_t *group_cost;
    uint32_t resume;
    int stack_cap;                    // counting builds only: entries a walker's stack column may hold (the kernel's own, or RTAMD_PT_STACK_CAP); the plain kernels hold it as an immediate
    int refill, leaf_batch;           // as in rt_wavefront.h (refill = closest-hit walker's | light walker's << 16; leaf_batch = batch | share << 16)
    int shade_min;                    // a wave turns shader when this many paths wait for shading (64 = a full wave of them)
    int shade_thr0, shade_thr_step;   // wave w stops refilling its walkers when need_shade holds >= thr0 + w * step paths
    int cost_t, cost_l;               // relative cost of a closest-hit / light query (walker split)
    uint32_t front_first;             // 1: the queues serve the front of the workgroup's group list first (the host sorted it by cost, most expensive first)
    int prio;                         // experiment: 1 = walker stints run at raised wave priority (s_setprio 2), 2 = shader batches do
    unsigned long long deadline_ticks; // 100 MHz ticks a wave may spend in this launch before it gives up (error)
    unsigned long long *counters;     // rt_types.h CounterSlot
    unsigned long long *debug;        // nullable: per workgroup {start time, exit time of its last wave (100 MHz ticks), paths}
    // COUNT builds, RTAMD_TRACE_PIXEL: every hit record the shader consumes for pixel trace_pixel (= y * width + x) is appended as
    // four float4 (r0..r3 of the path record: ray, hit, packed word); word 0 of trace_buf counts the entries
    float4 *trace_buf; uint32_t trace_cap; int32_t trace_pixel;
};

// COUNT builds only: where a wave's time goes (shader-clock cycles per role, the slots of CNT_ROLE_TIME: closest-hit walks, light walks, shading,
// rare roles, idle) and how full its walker iterations are ([2]: closest-hit | light walker)
struct PtProf {
    unsigned long long t_role[5] = {0, 0, 0, 0, 0};
    unsigned long long iters[2] = {0, 0}, lane_iters[2] = {0, 0}, stints = 0, shade_batches = 0, shade_items = 0;
    // where a walker's wave time goes (counting build): [0] hand-off and refill, [1] inner nodes, [2] leaves; tests / lane-tests of the leaf loops; light hits
    unsigned long long t_part[2][3] = {{0, 0, 0}, {0, 0, 0}}, leaf_iters[2] = {0, 0}, leaf_lane_iters[2] = {0, 0}, light_hits = 0, light_tests = 0; // the last two per lane
    unsigned long long t_sub[2][3] = {{0, 0, 0}, {0, 0, 0}}, refills[2] = {0, 0}; // of [0]: publish finished walks | take new ones from the bitmap | read their rays
    unsigned long long light_reach[2] = {0, 0}; // light sums whose walk ends at the light tree's root / one level below it (pt_light_reach), per lane
    PtPopStat pops[3];                          // what pt_pop handed out, by queue (PT_Q_TRACE, PT_Q_LIGHT, PT_Q_SHADE); flushed by the hw8 kernel only (CNT_P8_POPS)
    // the hw8 shader's wave time by section (PtShadeLap: [0] record load, gate and pending bounce, [1] attributes and textures, [2] Mix::sample,
    // [3] BRDF and pdf, [4] path end), the lanes that ran each section, and the hits at the deepest level among them (CNT_P8_SHADE_*)
    unsigned long long t_shade[5] = {0, 0, 0, 0, 0}, shade_lanes[5] = {0, 0, 0, 0, 0}, shade_last = 0;
};
template <bool COUNT> struct PtLap { // s_memtime laps of the counting build
    unsigned long long t;
    RT_DEV PtLap() : t(COUNT ? __builtin_amdgcn_s_memtime() : 0ull) {}
    RT_DEV void lap(unsigned long long &acc) { if (COUNT) { const unsigned long long n = __builtin_amdgcn_s_memtime(); acc += n - t; t = n; } }
};

// The shader's laps (counting build): a lane carries the cycles of the sections it ran through one batch; the sections are divergent, so
// the clock is read where a section ends for its lanes (s_memtime is scalar: all lanes of a section take the same two readings), and
// PtRoles::shade books each section once per batch with the number of lanes that hold a time for it.
template <bool COUNT> struct PtShadeLap {
    unsigned long long t;
    uint32_t d[5] = {0, 0, 0, 0, 0};
    bool last = false;                // the lane shades a hit at the deepest level
    RT_DEV PtShadeLap() : t(__builtin_amdgcn_s_memtime()) {}
    RT_DEV void start() { t = __builtin_amdgcn_s_memtime(); } // a section that begins where lanes of different sections meet again
    RT_DEV void lap(int k) { const unsigned long long n = __builtin_amdgcn_s_memtime(); d[k] += (uint32_t)(n - t); t = n; }
    RT_DEV void at_last_level() { last = true; }
};
template <> struct PtShadeLap<false> { // the plain kernels carry nothing
    RT_DEV void start() {}
    RT_DEV void lap(int) {}
    RT_DEV void at_last_level() {}
};

// wave-uniform state
struct PtWave {
    uint32_t nw, n_local, n_blocks, block;
    bool front_first;                 // pt_pop's from_start for the trace / light / shade queues (PtParams::front_first)
    uint32_t cur[5];
};

// A workgroup's paths come in groups of 2^shift consecutive slots (PtParams::group_shift: 6 = an 8x8 sub-tile, 4 = two rows of one): the unit of the deal.
template <class SH> RT_DEV uint32_t pt_gshift(const SH &sh) { return (uint32_t)__builtin_amdgcn_readfirstlane(__hip_atomic_load(&sh.cnt[PT_GSHIFT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }
template <class SH> RT_DEV uint32_t pt_slot(const SH &sh, uint32_t l) { const uint32_t g = pt_gshift(sh); return (sh.groups[l >> g] << g) | (l & ((1u << g) - 1u)); }
// One of the two walks of path l is done (its results are in HBM, ordered before this call by the caller's release fence):
// clear its pending bit; whoever clears the last one hands the path to the shaders.  Wave-uniform call.
template <class SH> RT_DEV void pt_complete(SH &sh, uint32_t l, uint32_t bit, bool doit) {
    bool ready = false;
    if (doit) {
        const uint32_t shift = (l & 15u) * 2u;
        const uint32_t old = atomicAnd(&sh.pending[l >> 4], ~(bit << shift));
        ready = ((old >> shift) & 3u) == bit;
    }
    pt_push(sh, PT_Q_SHADE, l, ready);
}

// ---- the walker loop -----------------------------------------------------------------------------------------------------------
// The walker loop of rt_wavefront.h (wf_walk_loop, while-while) with its lanes refilled from a `need` bitmap: the one loop of the closest-hit and
// the light-sum walkers of this file and of rt_persistent_hw6.h.  A walker is a policy WK, a struct that holds the per-walk state of a
// lane and says what differs between the four:
//   Queue                           which queue it serves and how a finished lane is published (PtTraceQueue, PtLightQueue)
//   COST_NODE, COST_TEST            what a node step / a leaf test adds to the walk's `steps`, the cost measure of the re-deal (PT_COST_*)
//   begin(slot)                     read the ray from the path's record, reset the walk's state
//   step<COUNT>(cur, sp, parked)    one wide step: the lane's next `cur` (pt_wide_step_*); full(): what a full stack column means for the walk's result
// The walk's place is `cur` and `sp` alone: a node or a leaf to visit, PT_DRAINED, or one of the marks PT_IDLE, PT_ENDED, PT_FULL.  The node loop
// writes nothing but `cur`, `sp`, `steps` and the parked leaves; a walk that ends there, by an empty column or a full one, only leaves its mark in
// `cur`, and full() and end() run outside the loop (DEFER) or right where the mark appears (immediate endings), through one `finish`.
//   Leaf, test(i, sp, lf)           the state of one leaf phase and its per-triangle body: tests record i, returns whether it was its leaf's last
//   leaves_done(lf, sp)             after a lane's leaf loop; returns whether the walk is over whatever its stack holds
//   end(l, slot, steps)             the end of a walk: writes its result, returns the lane's `fin` word (path l, bit 31 for the queue's use)
// Two measured tuning choices are parameters (DESIGN.md, section 3 "leaf phases"); nothing else depends on who is served:
//   SLOTS  leaves a lane may park for the next leaf phase: 3 for hw8 (one slot 380, two 396 -> 414 Msamples/s, the third +0.6 %), 2 for hw6
//   DEFER  the end of a walk runs once per pass for all lanes that ended in it (hw8: +1.2 %), or at once where the walk ends (the hw6
//          kernel lost 3 % with the deferred form and keeps the immediate one)
struct PtTraceQueue {
    static constexpr int ID = PT_Q_TRACE;
    static RT_DEV int refill_at(const PtParams &P) { return P.refill & 0xFFFF; }
    template <class SH> static RT_DEV void publish(SH &sh, uint32_t fin) { pt_complete(sh, fin, PT_BIT_T, fin != PT_NONE); }
};
// bit 31 of `fin`: the sum is left to a rare role (queue RARE: PT_Q_XLIGHT, P6_Q_SLOW), which completes the path's light bit in its turn
template <int RARE> struct PtLightQueue {
    static constexpr int ID = PT_Q_LIGHT;
    static RT_DEV int refill_at(const PtParams &P) { return P.refill >> 16; }
    template <class SH> static RT_DEV void publish(SH &sh, uint32_t fin) {
        const bool slow = (fin >> 31) != 0u && fin != PT_NONE;
        pt_complete(sh, fin, PT_BIT_L, fin != PT_NONE && !slow);
        pt_push(sh, RARE, fin & 0x7FFFFFFFu, slow);
    }
};
// the work of a finished walk, booked to its path's group (PtShared::cost)
template <class SH> RT_DEV void pt_book_cost(SH &sh, const PtParams &P, uint32_t l, uint32_t steps) {
    if (P.group_cost) atomicAdd(&sh.cost[l >> pt_gshift(sh)], steps);
}

template <int SLOTS, bool DEFER, bool COUNT, class WK, class SH>
RT_DEV void pt_walk_stint(WK &w, SH &sh, const PtParams &P, PtWave &wv, uint32_t (*stack)[64], const int shade_thr,
                          uint32_t &n_queries, unsigned long long &n_nodes, unsigned long long &n_tris, PtProf &prof) {
    static_assert(SLOTS == 2 || SLOTS == 3, "a lane parks two or three leaves");
    typedef typename WK::Queue Q;
    constexpr int K = Q::ID; // PtProf's index of the walker
    const int lane = threadIdx.x & 63;
    bool refill_ok = true;
    uint32_t l = 0, slot = 0, cur = PT_IDLE, fin = PT_NONE; // fin: the lane's finished, unpublished path
    int sp = 0;
    uint32_t pend = RT_EMPTY_LEAF, pend2 = RT_EMPTY_LEAF, pend3 = RT_EMPTY_LEAF; // the leaves this lane has met and not yet tested (pend first)
    uint32_t steps = 0;   // node steps + leaf tests of the lane's current walk, weighted
    auto finish = [&]() { // of a lane whose `cur` is PT_ENDED or PT_FULL
        if (cur == PT_FULL) { // the parked leaves stay untested: a rare role redoes the query
            w.full();
            pend = RT_EMPTY_LEAF; pend2 = RT_EMPTY_LEAF; pend3 = RT_EMPTY_LEAF;
        }
        fin = w.end(l, slot, steps);
        cur = PT_IDLE;
    };
    PtLap<COUNT> clk;
    for (;;) {
        // Walks that ended since the last pass write their results here, together: in the loops below a lane only marks itself, so the
        // code of an ending (gap code or sum, record store, cost counter) runs once per pass and not in every step in which some lane ends.
        if (DEFER && pt_ballot(pt_is_ending(cur))) {
            if (pt_is_ending(cur)) finish();
        }
        const unsigned long long idle = pt_ballot(cur == PT_IDLE);
        if (idle && (__popcll(idle) >= Q::refill_at(P) || idle == ~0ull)) {
            // Hand-off point.  Finished lanes are published here and not the moment they finish: the release (a wait for the
            // wave's outstanding record stores) is paid once per refill, when the stores have long landed, not once per walk.
            PtLap<COUNT> sub;
            if (COUNT) prof.refills[K]++;
            if (pt_ballot(fin != PT_NONE)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                Q::publish(sh, fin);
                fin = PT_NONE;
            }
            sub.lap(prof.t_sub[K][0]);
            if (!refill_ok) {}
            else if (pt_count(&sh.cnt[PT_Q_SHADE]) >= shade_thr) refill_ok = false;      // shaders are behind: drain, then help them
            else if (pt_count(&sh.cnt[Q::ID]) > 0) {
                const uint32_t got = pt_pop(sh.need[Q::ID], &sh.cnt[Q::ID], wv.nw, wv.cur[Q::ID], cur == PT_IDLE, wv.front_first, COUNT ? &prof.pops[K] : nullptr);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                sub.lap(prof.t_sub[K][1]);
                n_queries += __popcll(pt_ballot(got != PT_NONE));
                if (got != PT_NONE) {
                    l = got; slot = pt_slot(sh, l);
                    w.begin(slot);
                    steps = 0;
                    cur = 0; sp = 0; pend = RT_EMPTY_LEAF; pend2 = RT_EMPTY_LEAF; pend3 = RT_EMPTY_LEAF;
                }
                sub.lap(prof.t_sub[K][2]);
            }
        }
        const unsigned long long m_active = pt_ballot(cur != PT_IDLE);
        clk.lap(prof.t_part[K][0]);
        if (!m_active) break;
        const int lb = pt_leaf_batch(P.leaf_batch, m_active);
        for (;;) { // phase 1: inner nodes
            // A lane that meets a leaf keeps it for the next leaf phase and walks on with what its stack holds (a leaf beyond its slots stops
            // it): more lanes stay in the node loop, and more of them bring a leaf to each leaf phase.
            if ((cur & RT_LEAF_BIT) && (SLOTS == 3 ? pend3 : pend2) == RT_EMPTY_LEAF && cur != PT_DRAINED) {
                if (pend == RT_EMPTY_LEAF) pend = cur; else if (SLOTS == 2 || pend2 == RT_EMPTY_LEAF) pend2 = cur; else pend3 = cur; // (an empty leaf leaves the slot as it was)
                cur = pt_pop_or_end(stack, lane, sp, pend != RT_EMPTY_LEAF); // (PT_ENDED: an empty leaf was all that was left)
                if (!DEFER && cur == PT_ENDED) finish();
            }
            // The two ballots that end the phase: no lane is at an inner node, or at least `lb` lanes wait at a leaf (the marks are neither).
            // One flag, not `||`: both conditions are wave-uniform, and two exits would be two branch targets at the loop's top.
            const bool inner = pt_is_inner(cur);
            const bool stop = (pt_ballot(inner) == 0ull) | (__popcll(pt_ballot((cur & RT_LEAF_BIT) != 0u)) >= lb);
            if (stop) break;
            if (COUNT) { prof.iters[K]++; prof.lane_iters[K] += __popcll(pt_ballot(inner)); }
            if (inner) {
                if (COUNT) n_nodes++;
                steps += WK::COST_NODE;
                cur = w.template step<COUNT>(cur, sp, pend != RT_EMPTY_LEAF);
                if (!DEFER && pt_is_ending(cur)) finish();
            }
        }
        clk.lap(prof.t_part[K][1]);
        const bool at_leaf = pend != RT_EMPTY_LEAF && (!DEFER || cur != PT_FULL); // (idle lanes have nothing parked)
        if (COUNT) { prof.leaf_iters[K]++; prof.leaf_lane_iters[K] += __popcll(pt_ballot(at_leaf)); }
        if (at_leaf) { // phase 2: the lane's parked leaves, in the order it met them
            uint32_t i = pend & ~RT_LEAF_BIT, more = pend2, more2 = pend3;
            typename WK::Leaf lf;
            for (;;) { // ONE loop over all of them: a lane goes on to its next leaf while its neighbours are still in their first
                const bool last = w.test(i, sp, lf);
                if (COUNT) n_tris++;
                steps += WK::COST_TEST;
                if (!last) i++;
                else if (more == RT_EMPTY_LEAF) break;
                else { i = more & ~RT_LEAF_BIT; more = more2; more2 = RT_EMPTY_LEAF; } // the lane's next leaf
            }
            const bool over = w.leaves_done(lf, sp);
            pend = RT_EMPTY_LEAF; pend2 = RT_EMPTY_LEAF; pend3 = RT_EMPTY_LEAF;
            if (cur == PT_DRAINED || over) { // a lane that stopped at a leaf beyond its slots keeps that for the next round
                cur = PT_ENDED;
                if (!DEFER) finish();
            }
        }
        clk.lap(prof.t_part[K][2]);
    }
}

// What a walker reads in its innermost loops it reads through a GlobalBytes of its own (rt_device.h global_bytes_own): a scalar base, 32-bit offsets.
// ---- closest-hit walker: near-first, tie -> lowest figure index ---------------------------------------------------------------------
struct PtTraceWalk {
    typedef PtTraceQueue Queue;
    static constexpr uint32_t COST_NODE = PT_COST_TRACE_NODE, COST_TEST = PT_COST_TRACE_TRI;
    const SceneView &S; const WfView &W; PtShared &sh; const PtParams &P; uint32_t (*stack)[64];
    const GlobalBytes nodes = global_bytes_own(S.nodes4), tris = global_bytes(S.tri_walk);
    const int lane = threadIdx.x & 63;
    F3 o = f3(0.f, 0.f, 0.f), d = f3(0.f, 0.f, 1.f);
    RayGrid ray = RT_GRID_RAY_IDLE; // idle lanes: never used
    uint32_t hit = WF_MISS;
    float best_t = RT_T_MAX, best_u = 0.f, best_v = 0.f;
    // Boxes are pruned, and farther hits dropped, only beyond cull_t = best_t + the look-behind of rt_exact.h: the runner-up of the
    // best hit must be SEEN, whatever tree the walk uses, to decide at the end of the walk whether the exact walk is needed.
    float cull_t = RT_T_MAX, t2 = 2.f * RT_T_MAX, h_ray = 0.f; // h_ray: absolute part of the look-behind (pt_look_behind)
    struct Leaf {};
    RT_DEV void begin(uint32_t slot) {
        const float4 *r = wf_rec(W, slot);
        float4 q0 = r[0], q1 = r[1];
        o = f3(q0.x, q0.y, q0.z); d = f3(q0.w, q1.x, q1.y);
        ray = make_ray_grid(S.grid, o, d);
        h_ray = S.exact_boxes ? pt_look_behind_abs(d, S.box_c2x) : 0.f;
        hit = WF_MISS; best_t = RT_T_MAX; cull_t = RT_T_MAX; t2 = 2.f * RT_T_MAX; best_u = 0.f; best_v = 0.f;
    }
    // (the cap of the column is an immediate but in the counting build, where RTAMD_PT_STACK_CAP may lower it)
    template <bool COUNT> RT_DEV uint32_t step(uint32_t cur, int &sp, bool parked) {
        return pt_wide_step_nearest(nodes, ray, cull_t, stack, lane, sp, COUNT ? P.stack_cap : P8_STACK, cur, parked);
    }
    // The column is full (a walk holds up to three entries per level of a tree of up to P8_STACK / 2 levels; this takes a ray that
    // grazes many boxes: triangle soups).  The walk says so — no hit has a negative t — and the exact role walks the query with a
    // stack of its own (pt_exact_batch).
    RT_DEV void full() { best_t = PT_T_OVERFLOW; best_u = 0.f; best_v = 0.f; hit = 0u; t2 = PT_T_OVERFLOW; }
    RT_DEV bool test(uint32_t i, int, Leaf &) {
        TriIsect T = load_isect(tris, record_ofs(i, (uint32_t)sizeof(TriIsect)));
        float t, u, v; bool inside;
        const uint32_t fi = T.pad >> 1; // index in the figure order
        if (tri_test_closer(T, o, d, cull_t, t, u, v, inside)) {
            const uint32_t best_i = hit & WF_INDEX_MASK;
            if (t < best_t || (t == best_t && fi < best_i)) { // reference tie rule: smallest t, equal t -> lowest figure index
                t2 = fminf(t2, best_t);
                best_t = t; best_u = u; best_v = v; hit = fi | (inside ? WF_INSIDE_BIT : 0u);
                cull_t = t + fmaxf(S.cull_k * t, h_ray);
            } else t2 = fminf(t2, t);
        }
        return (T.pad & 1u) != 0u;
    }
    RT_DEV bool leaves_done(Leaf &, int) { return false; }
    RT_DEV uint32_t end(uint32_t l, uint32_t slot, uint32_t steps) { // the gate (pt_shade_item) decides with the runner-up's t whether this hit needs the exact walk
        wf_rec(W, slot)[2] = make_float4(best_t, best_u, best_v, __uint_as_float(S.exact_boxes && hit != WF_MISS ? hit | pt_gap_code(best_t, t2) : hit));
        pt_book_cost(sh, P, l, steps);
        return l;
    }
};

// ---- light-sum walker (WfLightWalk of rt_wavefront.h): every light on the ray, the hits kept sorted at the top of the lane's column --
template <bool COUNT> struct PtLightWalk {
    typedef PtLightQueue<PT_Q_XLIGHT> Queue;
    static constexpr uint32_t COST_NODE = PT_COST_LIGHT_NODE, COST_TEST = PT_COST_LIGHT_TEST;
    const SceneView &S; const WfView &W; PtShared &sh; const PtParams &P; uint32_t (*stack)[64]; PtProf &prof;
    const GlobalBytes nodes = global_bytes_own(S.light_walk_nodes4), tests = global_bytes_own(S.lights_walk_test), rests = global_bytes(S.lights_walk_rest);
    const int lane = threadIdx.x & 63;
    bool overflow = false; // the exact role sums this query
    int k = 0;             // hits so far
    F3 o = f3(0.f, 0.f, 0.f), d = f3(0.f, 0.f, 1.f);
    RayGrid ray = RT_GRID_RAY_IDLE; // idle lanes: never used
    // The leaf loop only tests; what a hit needs beyond the test (the rest of the light's record, the pdf term, the robustness test, the
    // sorted insertion) waits until after the loop — a lane rarely hits twice in one leaf phase, and the long hit code then runs once
    // per phase instead of once per tested light.
    struct Leaf { bool held = false; uint32_t h_i = 0u, h_li = 0u; float h_t = 0.f, h_u = 0.f, h_v = 0.f; bool h_in = false; };
    RT_DEV void begin(uint32_t slot) {
        const float4 *r = wf_rec(W, slot);
        float4 q0 = r[0], q1 = r[1];
        o = f3(q0.x, q0.y, q0.z); d = f3(q0.w, q1.x, q1.y);
        ray = make_ray_grid(S.grid, o, d);
        k = 0; overflow = false;
    }
    template <bool> RT_DEV uint32_t step(uint32_t cur, int &sp, bool parked) { // the hits sit at the column's top
        return pt_wide_step_all(nodes, ray, stack, lane, sp, (COUNT ? P.stack_cap : P8_STACK) - 2 * k - 1, cur, parked);
    }
    RT_DEV void full() { overflow = true; } // no room beside the hits
    RT_DEV void take(Leaf &lf, int sp) { // the held hit joins the lane's hits
        bool robust;
        const float term = pt_light_pdf_hit(S, tests, rests, lf.h_i, o, d, lf.h_t, lf.h_u, lf.h_v, lf.h_in, robust);
        if (COUNT && term != 0.f) prof.light_hits++;
        if (term != 0.f) { // (a hit whose term is exactly 0 adds nothing, like a miss)
            if (!robust || k >= WF_MAX_LIGHT_HITS || sp + 2 * k + 2 >= P8_STACK) overflow = true;
            else { // kept sorted by light index (this tree's leaf order is not the light order): hit j at words P8_STACK-1-2j (index), -2-2j (term)
                int j = k;
                while (j > 0 && stack[P8_STACK - 1 - 2 * (j - 1)][lane] > lf.h_li) {
                    stack[P8_STACK - 1 - 2 * j][lane] = stack[P8_STACK - 1 - 2 * (j - 1)][lane];
                    stack[P8_STACK - 2 - 2 * j][lane] = stack[P8_STACK - 2 - 2 * (j - 1)][lane];
                    j--;
                }
                stack[P8_STACK - 1 - 2 * j][lane] = lf.h_li; stack[P8_STACK - 2 - 2 * j][lane] = __float_as_uint(term); k++;
            }
        }
        lf.held = false;
    }
    RT_DEV bool test(uint32_t i, int sp, Leaf &lf) {
        bool last, inside; uint32_t li; float t, u, v;
        if (COUNT) prof.light_tests++;
        if (pt_light_test(tests, i, o, d, last, li, t, u, v, inside)) {
            if (lf.held) take(lf, sp); // a second hit in this phase
            lf.held = true; lf.h_i = i; lf.h_li = li; lf.h_t = t; lf.h_u = u; lf.h_v = v; lf.h_in = inside;
        }
        return last;
    }
    RT_DEV bool leaves_done(Leaf &lf, int sp) { if (lf.held) take(lf, sp); return false; }
    RT_DEV uint32_t end(uint32_t l, uint32_t slot, uint32_t steps) {
        pt_book_cost(sh, P, l, steps);
        if (overflow) return l | 0x80000000u;
        float v = 0.f;
        if (k == 1) v = __uint_as_float(stack[P8_STACK - 2][lane]);
        else if (k == 2) v = __uint_as_float(stack[P8_STACK - 2][lane]) + __uint_as_float(stack[P8_STACK - 4][lane]);
        else if (k > 2) { // the reference's association of the additions: wf_merge_light_hits of rt_wavefront.h, for this kernel's columns
            const uint32_t nl = S.n_lights;
            for (int j = 1; j < k; j++) {
                uint32_t a0 = stack[P8_STACK - 1 - 2 * (j - 1)][lane], b0 = stack[P8_STACK - 1 - 2 * j][lane];
                uint32_t len = b0 - a0;
                uint32_t lv = 31u - (uint32_t)__clz((int)len);
                uint16_t m0 = S.light_sep[(size_t)lv * nl + a0], m1 = S.light_sep[(size_t)lv * nl + (b0 - (1u << lv))];
                stack[j - 1][lane] = m0 < m1 ? m0 : m1;
            }
            for (int n = k; n > 1; n--) {
                int best = 1;
                uint32_t bd = stack[0][lane];
                for (int i = 2; i < n; i++) { uint32_t di = stack[i - 1][lane]; if (di > bd) { bd = di; best = i; } }
                float merged = __uint_as_float(stack[P8_STACK - 2 - 2 * (best - 1)][lane]) + __uint_as_float(stack[P8_STACK - 2 - 2 * best][lane]);
                stack[P8_STACK - 2 - 2 * (best - 1)][lane] = __float_as_uint(merged);
                for (int i = best; i < n - 1; i++) {
                    stack[P8_STACK - 2 - 2 * i][lane] = stack[P8_STACK - 2 - 2 * (i + 1)][lane];
                    stack[i - 1][lane] = stack[i][lane];
                }
            }
            v = __uint_as_float(stack[P8_STACK - 2][lane]);
        }
        int depth = (int)(__float_as_uint(reinterpret_cast<const float *>(wf_rec(W, slot) + 3)[3]) & 15u);
        float *pdf = reinterpret_cast<float *>(wf_entry(W, slot, depth)) + 3;
        *pdf = *pdf + v / S.n_lights_f;                                  // distributions.h:123,273
        return l;
    }
};

// ---- the shader role: wf_shade_item / pt_shade_item of rt_wavefront.h laid out for a 96-VGPR budget -----------------------------------
// Same arithmetic, same order of random draws, same record writes.  What differs is where values wait: the shading code is a chain of
// sections (finish the pending bounce | hit attributes and textures | Mix::sample | BRDF | Mix::pdf terms | path epilogue), each of
// which needs 50-75 VGPRs on its own, and only what the *current* section works on stays in registers.  Everything else that a later
// section needs — the incoming direction, the random engine, base colour x texture colour, the metallic product, a path's tail —
// is parked in this lane's column of the wave's LDS stack area (idle while the wave shades; volatile accesses, so the compiler neither
// forwards a parked value through a register nor moves other memory operations across a park / unpark).
// Each section runs once per batch.  A batch mixes depths, so a hit at the deepest level, of which getColor keeps only the emission, has no
// branch of its own (the round pipeline's wf_shade_item has one: its launches are of one depth): it takes the common sections and ends
// with the lanes whose BRDF is black, untraced.  The three normal draws of the cosine sampler are one call (rng_n01x3: two polar loops
// for the wave, not three), and the VNDF frame that its sampler and its pdf both need is formed once, before the components part, and parked.
#define PK_TAIL 0                     // 3 words: value the innermost call returns (paths that end)
#define PK_LEVELS 3                   // bounces below which it returns
#define PK_RNG 4                      // engine state, saved normal (has_saved travels in the packed word)
#define PK_D 6                        // incoming direction (3)
#define PK_BC 9                       // base_color * texture colour (3), metallic * baseMetallic
#define PK_Q 13                       // the VNDF frame of the hit, shared by vndf_sample and vndf_pdf: the rotation vndf_getq(sn) (4) ...
#define PK_VT 17                      // ... and the outgoing direction in it, qtransform(q, -d) (3)
#define PK_WORDS 20
static_assert(PK_WORDS <= P8_STACK, "the shader parks its values in the lane's stack column");
typedef __attribute__((address_space(3))) volatile uint32_t *PtLdsWord; // an LDS pointer that stays one (32-bit base + immediate offsets)
struct PtPark {
    PtLdsWord p;                      // this lane's column: word i at p[64 * i]
    RT_DEV void put(int i, float v) const { p[64 * i] = __float_as_uint(v); }
    RT_DEV void putu(int i, uint32_t v) const { p[64 * i] = v; }
    RT_DEV float get(int i) const { return __uint_as_float(p[64 * i]); }
    RT_DEV uint32_t getu(int i) const { return p[64 * i]; }
    RT_DEV void put3(int i, F3 v) const { put(i, v.x); put(i + 1, v.y); put(i + 2, v.z); }
    RT_DEV F3 get3(int i) const { const float x = get(i), y = get(i + 1), z = get(i + 2); return f3(x, y, z); }
    RT_DEV Rng rng(uint32_t packed) const { Rng g; g.x = getu(PK_RNG); g.saved = get(PK_RNG + 1); g.has_saved = (packed & 16u) != 0; return g; }
    RT_DEV void keep(const Rng &g, uint32_t &packed) const { putu(PK_RNG, g.x); put(PK_RNG + 1, g.saved); packed = g.has_saved ? (packed | 16u) : (packed & ~16u); }
    RT_DEV void end(F3 tail, int levels) const { put3(PK_TAIL, tail); putu(PK_LEVELS, (uint32_t)levels); }
    RT_DEV void frame(Quat q, F3 vT) const { put3(PK_Q, q.v); put(PK_Q + 3, q.w); put3(PK_VT, vT); }
    RT_DEV Quat q() const { Quat g; g.v = get3(PK_Q); g.w = get(PK_Q + 3); return g; }
};

template <int FEAT, bool COUNT>
RT_DEV int pt_shade_lean(const SceneView &S, const RenderView &R, const WfView &W, const uint32_t slot, const PtPark pk, bool &discarded, PtShadeLap<COUNT> &lp) {
    float4 *r = wf_rec(W, slot);
    uint32_t packed = __float_as_uint(reinterpret_cast<const float *>(r + 3)[3]);
    int depth = (int)(packed & 15u);
    const float4 q0 = r[0], q1 = r[1], q2 = r[2];
    const uint32_t hit = __float_as_uint(q2.w);
    // Everything whose address is known once the record is in goes out together — the figure's box (the gate), its plane normal, the head of
    // its TriShade record (texture coordinates, material), the pending bounce's entry — so that ONE memory latency covers what would otherwise
    // be four dependent round trips (gate -> entry -> normal -> attributes).  Lanes without a hit read figure 0, lanes without a pending
    // bounce read their level's entry anyway: the values are simply not used.
    const uint32_t fig = hit != WF_MISS ? (hit & WF_INDEX_MASK) : 0u;
    float4 blo = make_float4(0.f, 0.f, 0.f, 0.f), bhi = blo;
    if (S.exact_boxes) { const float4 *bx = reinterpret_cast<const float4 *>(S.tri_box) + 2 * (size_t)fig; blo = bx[0]; bhi = bx[1]; }
    const F3 tri_n = load_tri_normal(S, fig);
    const TriShadeHead head = load_shade_head(S, fig);
    float4 pe0, pe1;
    { const float4 *e = wf_entry(W, slot, depth); pe0 = e[0]; pe1 = e[1]; }
    // the exactness gate (pt_shade_item): a hit that does not stand as the reference's answer goes to the exact walk first, untouched
    if (q2.x == PT_T_OVERFLOW && !(packed & WF_VERIFIED_BIT)) return PT_SHADE_EXACT; // the walk ran out of stack (PtTraceWalk::full)
    if (S.exact_boxes == 1u && hit != WF_MISS && !(packed & WF_VERIFIED_BIT) &&
        !pt_hit_stands(f3(blo.x, blo.y, blo.z), f3(bhi.x, bhi.y, bhi.z), f3(q0.x, q0.y, q0.z), f3(q0.w, q1.x, q1.y), q2.x, pt_gap_floor(hit, q2.x), S.box_c2, S.box_c2x, S.cull_k))
        return PT_SHADE_EXACT;
    pk.put(PK_D, q0.w); pk.put(PK_D + 1, q1.x); pk.put(PK_D + 2, q1.y);
    pk.putu(PK_RNG, __float_as_uint(q1.z)); pk.put(PK_RNG + 1, q1.w);
    bool ended = false;
    if (packed & WF_PENDING_BIT) {
        // The bounce at `depth` sampled the ray that was just traced; its pdf is complete now (Mix::pdf, distributions.h:268-278).
        float4 *e = wf_entry(W, slot, depth);
        const float4 e0 = pe0, e1 = pe1;
        const float pdf = e0.w / S.n_components_f;                                  // :278
        const float k = (float)(1. / (double)pdf * fabs((double)e1.w));             // scene.cpp:159
        F3 mult = k * f3(e1.x, e1.y, e1.z);
        const bool clamp = mult.x > 6.f || mult.y > 6.f || mult.z > 6.f || mult.x != mult.x || mult.y != mult.y || mult.z != mult.z;
        if (clamp || depth + 1 >= R.ray_depth) {
            // clamp hack (scene.cpp:161-163): the path returns the emission and the speculative hit is dropped; at the
            // last level the inner call returns 0, i.e. emission + mult * 0 evaluated literally.
            discarded = true; ended = true;
            if (clamp) pk.end(f3(e0.x, e0.y, e0.z), depth);
            else { e[1] = make_float4(mult.x, mult.y, mult.z, e1.w); pk.end(f3(0.f, 0.f, 0.f), depth + 1); }
        } else {
            bool survives = true;
            if (R.rr_depth > 0 && depth + 1 >= R.rr_depth) { // Russian roulette (throughput mode only), see wf_shade_item
                Rng rng = pk.rng(packed);
                const float q = wf_roulette_q(W, slot, depth, mult);
                survives = rng_u01(rng) < q;
                mult = (1.f / q) * mult;
                pk.keep(rng, packed);
            }
            e[1] = make_float4(mult.x, mult.y, mult.z, e1.w);
            if (survives) depth++;
            else { discarded = true; ended = true; pk.end(f3(0.f, 0.f, 0.f), depth + 1); }
        }
    }
    lp.lap(0);
    if (!ended) {
        HitRec h;
        h.idx = (int)(hit & WF_INDEX_MASK); h.inside = (hit & WF_INSIDE_BIT) != 0; h.t = q2.x; h.u = q2.y; h.v = q2.z;
        if (hit == WF_MISS) { ended = true; pk.end(miss_color<(FEAT & WF_FEAT_ENV) != 0>(S, pk.get3(PK_D)), depth); }
        else {
            // A hit at the deepest level (SceneView::last_level_emission_only: getColor returns its emission whatever Mix::sample / brdf /
            // pdf produce) takes the same sections as every other hit, so that a batch of mixed depths runs each of them once: its draws are
            // Mix::sample's, in order, and it leaves where a black BRDF leaves, with the level's emission and no new ray to trace.
            const bool last = S.last_level_emission_only && depth + 1 >= R.ray_depth;
            if (last) lp.at_last_level();
            const bool hw7 = (FEAT & WF_FEAT_HW7) && S.hw7;
            float4 *e = wf_entry(W, slot, depth);
            {   // the next ray's origin goes to the path's record at once (its final place): x + eps * geomNorma, scene.cpp:104
                const F3 ng = geom_normal(tri_n, h.inside);
                const F3 x = f3(q0.x, q0.y, q0.z) + h.t * pk.get3(PK_D);
                const F3 xo = x + 9.99999974737875163555e-05f * ng;
                r[0] = make_float4(xo.x, xo.y, xo.z, 0.f);                           // the next ray doubles as the light query
            }
            float alpha; F3 sn;
            {
                // hit attributes, material, textures (scene.cpp:99-149).  The emission goes to the level's entry at once; colour and
                // metallic shrink to the products the BRDF uses and wait in the park.
                F3 base_color; float base_metallic; Shaded sh;
                shade_fetch_attr(S, h, head, sh, base_color, base_metallic, hw7);
                e[0] = make_float4(sh.emission.x, sh.emission.y, sh.emission.z, 0.f);
                pk.put3(PK_BC, base_color * sh.color);
                pk.put(PK_BC + 3, sh.metallic * base_metallic);
                alpha = sh.alpha; sn = sh.sn;
            }
            lp.lap(1);
            F3 nd;
            {   // Mix::sample (distributions.h:256-265)
                // the VNDF frame once per hit, for the sampler (component 1) and for the pdf (every lane): both would build it from sn and d
                { const Quat q = vndf_getq(sn); pk.frame(q, qtransform(q, neg(pk.get3(PK_D)))); }
                Rng rng = pk.rng(packed);
                const int comp = (int)(rng_u01(rng) * S.n_components_f);         // :257
                if (comp == 0) nd = cosine_sample(rng, sn);
                else if (comp == 2) { const float4 xq = r[0]; nd = light_sample(S, rng, f3(xq.x, xq.y, xq.z)); }
                else nd = vndf_sample(rng, pk.q(), pk.get3(PK_VT), alpha);
                pk.keep(rng, packed);
            }
            lp.lap(2);
            // the record and entry addresses are formed again from the slot number after the sampling code (an opaque copy, so that the
            // two 64-bit pointers do not sit in registers across it)
            uint32_t slot_again = slot;
            int depth_again = depth;
            asm volatile("" : "+v"(slot_again), "+v"(depth_again));
            r = wf_rec(W, slot_again);
            e = wf_entry(W, slot_again, depth_again);
            F3 brdf;
            {
                const F3 d = pk.get3(PK_D), bc = pk.get3(PK_BC);
                const float metallic_eff = pk.get(PK_BC + 3);
                brdf = hw7 ? material_brdf_hw7(bc, metallic_eff, nd, neg(d), sn, alpha * alpha)
                           : material_brdf_pre(bc, metallic_eff, nd, neg(d), sn, alpha);
            }
            const float epsf = 9.99999974737875163555e-05f;
            if (last || (brdf.x <= epsf && brdf.y <= epsf && brdf.z <= epsf)) {       // scene.cpp:154-156
                const float4 e0 = e[0];
                ended = true; pk.end(f3(e0.x, e0.y, e0.z), depth);
                lp.lap(3);
            } else {
                e[1] = make_float4(brdf.x, brdf.y, brdf.z, dot(nd, sn));
                float pdf = 0.f;                                                       // distributions.h:268-276, first two terms
                pdf += cosine_pdf(sn, nd);
                pdf += vndf_pdf(pk.q(), pk.get3(PK_VT), nd, alpha);
                reinterpret_cast<float *>(e)[3] = pdf;
                reinterpret_cast<float *>(r)[3] = nd.x;
                r[1] = make_float4(nd.y, nd.z, __uint_as_float(pk.getu(PK_RNG)), pk.get(PK_RNG + 1));
                const uint32_t sample = (packed >> 6) & WF_SAMPLE_MASK;
                reinterpret_cast<float *>(r + 3)[3] = __uint_as_float(wf_pack(depth, (packed & 16u) != 0, sample, true));
                lp.lap(3);
                return WF_NEXT_TRACE | (S.n_lights ? WF_NEXT_LIGHT : 0);               // traced speculatively beside its own light-pdf sum
            }
        }
    }
    lp.start();
    Rng rng = pk.rng(packed);
    const int todo = wf_finish_path<PtSource<FEAT>>(S, R, W, slot, (int)pk.getu(PK_LEVELS), pk.get3(PK_TAIL), rng, (packed >> 6) & WF_SAMPLE_MASK);
    lp.lap(4);
    return todo;
}

// ---- the exact role: one lane per query, the reference's own box arithmetic over the reference trees (rt_exact.h) -------------------
// At most PT_EXACT_BATCH queries of each kind per call; their node stacks live in the wave's (otherwise idle) LDS stack area, entry e of
// lane i at word e * PT_EXACT_BATCH + i — no scratch.  Rare (3e-5 of the queries), so the partly filled wave does not matter.
template <class SH>
RT_DEV void pt_exact_batch(const SceneView &S, const WfView &W, SH &sh, PtWave &wv, uint32_t *area, uint32_t &n_xlight, uint32_t &n_xtrace) {
    const uint32_t lane = threadIdx.x & 63u;
    const StridedStack<PT_EXACT_BATCH> xview = {area + (lane & (PT_EXACT_BATCH - 1u))};
    uint32_t got = pt_pop(sh.need[PT_Q_XLIGHT], &sh.cnt[PT_Q_XLIGHT], wv.nw, wv.cur[PT_Q_XLIGHT], lane < PT_EXACT_BATCH);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (got != PT_NONE) {
        const uint32_t slot = pt_slot(sh, got);
        const float4 *r = wf_rec(W, slot);
        float4 q0 = r[0], q1 = r[1];
        const F3 x = f3(q0.x, q0.y, q0.z), d = f3(q0.w, q1.x, q1.y);
        float v;
        if (S.exact_boxes) v = ref_light_pdf_sum(S, x, d, xview);
        else { Counters c; c.closest = c.lightq = c.nodes = c.tris = 0; v = light_pdf_sum<false>(S, x, d, xview, c); }
        wf_add_light_pdf(S, W, slot, v);
    }
    n_xlight += __popcll(pt_ballot(got != PT_NONE));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    pt_complete(sh, got, PT_BIT_L, got != PT_NONE);
    got = pt_pop(sh.need[PT_Q_XTRACE], &sh.cnt[PT_Q_XTRACE], wv.nw, wv.cur[PT_Q_XTRACE], lane < PT_EXACT_BATCH);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (got != PT_NONE) {
        const uint32_t slot = pt_slot(sh, got);
        float4 *r = wf_rec(W, slot);
        float4 q0 = r[0], q1 = r[1];
        float bt, bu, bv; uint32_t hit;
        if (S.exact_boxes == 1u) ref_closest_hit(S, f3(q0.x, q0.y, q0.z), f3(q0.w, q1.x, q1.y), xview, bt, bu, bv, hit);
        else { // no reference boxes to be exact about (a walk that ran out of stack): the padded float boxes of the two-box tree decide, as for every other hit
            Counters c; c.closest = c.lightq = c.nodes = c.tris = 0;
            const HitRec h = closest_hit<false, PT_EXACT_BATCH>(S, f3(q0.x, q0.y, q0.z), f3(q0.w, q1.x, q1.y), xview.p, c);
            bt = h.t; bu = h.u; bv = h.v; hit = h.idx < 0 ? WF_MISS : ((uint32_t)h.idx | (h.inside ? WF_INSIDE_BIT : 0u));
        }
        r[2] = make_float4(bt, bu, bv, __uint_as_float(hit));
        float *pk = reinterpret_cast<float *>(r + 3) + 3;
        *pk = __uint_as_float(__float_as_uint(*pk) | WF_VERIFIED_BIT);
    }
    n_xtrace += __popcll(pt_ballot(got != PT_NONE));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    // A hit the gate sent here has both walks behind it: it goes back to the shaders.  A ray that came here instead of to the walkers (a
    // tripwire, pt_tripwire) still has its closest-hit bit pending, and its light sum may be under way: the last of the two hands it on.
    bool ready = false;
    if (got != PT_NONE) {
        const uint32_t shift = (got & 15u) * 2u;
        const uint32_t old = (atomicAnd(&sh.pending[got >> 4], ~(PT_BIT_T << shift)) >> shift) & 3u;
        ready = old == 0u || old == PT_BIT_T;
    }
    pt_push(sh, PT_Q_SHADE, got, ready);
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------
// What a workgroup of THREADS threads does first, in this kernel and in rt_persistent_hw6.h's: its share of the pass's groups, the wave's
// state, cleared queues and tables in LDS (SH: PtShared, P6Shared), the debug stamp.  False: the workgroup owns no path and leaves.
template <int THREADS, class SH>
RT_DEV bool pt_enter(SH &sh, const PtParams &P, PtWave &wv) {
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    wv.n_blocks = gridDim.x; wv.block = blockIdx.x;
    wv.front_first = P.front_first != 0u;
    const uint32_t first_group = P.group_ofs ? P.group_ofs[wv.block] : 0u;
    const uint32_t n_local_groups = P.group_ofs ? P.group_ofs[wv.block + 1u] - first_group
                                                : (P.n_groups > wv.block ? (P.n_groups - wv.block + wv.n_blocks - 1u) / wv.n_blocks : 0u);
    wv.n_local = n_local_groups << P.group_shift;
    wv.nw = (wv.n_local + 31u) >> 5;
    if (wv.n_local == 0u) return false;
    if (P.debug && tid == 0) { P.debug[3 * blockIdx.x] = __builtin_amdgcn_s_memrealtime(); P.debug[3 * blockIdx.x + 2] = wv.n_local; }
    for (int q = 0; q < 5; q++) wv.cur[q] = (wave * 64u) % wv.nw;
    for (uint32_t i = tid; i < wv.nw; i += THREADS) { sh.need[0][i] = 0; sh.need[1][i] = 0; sh.need[2][i] = 0; sh.need[3][i] = 0; sh.need[4][i] = 0; }
    for (uint32_t i = tid; i < 2u * wv.nw; i += THREADS) sh.pending[i] = 0;
    for (uint32_t i = tid; i < n_local_groups; i += THREADS) { sh.groups[i] = P.group_ofs ? P.group_ids[first_group + i] : i * wv.n_blocks + wv.block; sh.cost[i] = 0; }
    if (tid < 16u) sh.cnt[tid] = tid == PT_GSHIFT ? (int)P.group_shift : 0;
    __syncthreads();
    return true;
}
// ... and last: the work booked for each of its groups goes back to the host (every wave leaves the scheduler loop once the workgroup's
// pixels are done, or at the deadline)
template <int THREADS, class SH>
RT_DEV void pt_leave(SH &sh, const PtParams &P, const PtWave &wv) {
    if (!P.group_cost) return;
    __syncthreads();
    const uint32_t n_local_groups = wv.n_local >> P.group_shift;
    for (uint32_t i = threadIdx.x; i < n_local_groups; i += THREADS) P.group_cost[sh.groups[i]] = sh.cost[i];
}

// A wave-uniform kernel argument compared where it is used: hoisted out of the scheduler loop, each compare of PtParams::prio holds a register pair across
// every role of the loop, and the walkers need them more (profiles/r09_scheduler_refactor.txt: reloads in the hw6 kernel's largest inner loop 106 -> 74).
RT_DEV int pt_here(int v) { asm volatile("" : "+s"(v)); return v; }
// ---- the kernel body: seeding, the scheduler loop and the epilogue, once for this file's kernel and rt_persistent_hw6.h's -----------------
// What the shader role decided for the path of one lane (all false / 0 for a lane without a path).
struct PtShaded {
    bool trace = false;   // the record holds a new ray that wants its closest hit: PT_BIT_T is outstanding ...
    bool light = false;   // ... and its light-pdf sum is walked beside it: PT_BIT_L
    bool xtrace = false;  // the closest hit is the exact role's (PT_Q_XTRACE): the hit the gate refused, or, with `trace`, the new ray's instead of PT_Q_TRACE
    bool done = false;    // the path is finished, or parked for the next phase of the frame
    uint32_t cost = 0;    // what the step adds to the work booked for the path's group (PtShared::cost); 0 for a refused hit
};
// What differs between the two kernels is a policy RL, the kernel's roles (PtRoles below, P6Roles of rt_persistent_hw6.h): a struct that
// holds the kernel's arguments (S, R, W, P), its LDS block `sh`, the wave's stack area `stack`, its own query counts, and says
//   THREADS, COUNT, SLOTS, DEFER    the workgroup's size; the counting build; the two measured choices of pt_walk_stint
//   trace_walk(), light_walk(prof)  the kernel's two walker policies
//   seed(slot, gslot, x, y, rng, sum)  writes r0..r3 of a fresh path: its first camera ray, drawn from `rng`, and the pixel sum; false: the slot starts no
//                                   path (a path source without a record for it, rt_path_source.h; the camera always has one)
//   resumed_sample(slot)            the sample count in the packed word of a record that carries on (PtParams::resume)
//   seed_wire(slot)                 whether the record's camera ray belongs to the exact role from the start (a tripwire)
//   rare(wv)                        runs one batch of the kernel's rare roles if any is queued, and says whether it did
//   shade(got, n_light, n_nodes, prof)  one shader step of path `got` (PT_NONE: none), between the loop's acquire and release: all that is the integrator's
//   flush(lane, prof)               the kernel's own counters at the exit
template <class RL>
RT_DEV void pt_run(RL &rl) {
    constexpr bool COUNT = RL::COUNT;
    auto &sh = rl.sh;
    const RenderView &R = rl.R;
    const PtParams &P = rl.P;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    PtWave wv;
    if (!pt_enter<RL::THREADS>(sh, P, wv)) return;

    // ---- init: seed every pixel of this workgroup, first camera ray (wf_init_kernel of rt_wavefront.h) -----------------------
    for (uint32_t base = 0; base < wv.n_local; base += RL::THREADS) {
        const uint32_t l = base + tid;
        bool started = false, wire = false;
        if (l < wv.n_local) {
            const uint32_t slot = pt_slot(sh, l), gslot = slot + rl.W.slot_base;
            int x, y; Rng rng; F3 sum;
            if (wf_seed_record(R, gslot, !P.resume, x, y, rng, sum)) {
                // a later phase of the frame: the record holds the pixel sum, the random stream and the parked camera ray
                if (P.resume) started = rl.resumed_sample(slot) < (uint32_t)R.samples;
                else started = rl.seed(slot, gslot, x, y, rng, sum);
                if (started) {
                    atomicOr(&sh.pending[l >> 4], PT_BIT_T << ((l & 15u) * 2u));
                    wire = rl.seed_wire(slot);
                }
            }
        }
        const unsigned long long m = pt_ballot(started);
        if (m && lane == 0) atomicAdd(&sh.cnt[PT_N_LIVE], (int)__popcll(m));
        pt_push(sh, PT_Q_TRACE, l, started && !wire);
        pt_push(sh, PT_Q_XTRACE, l, wire);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // ---- scheduler: every wave picks a role whenever it is idle ----------------------------------------------------------------
    uint32_t(*stack)[64] = rl.stack;
    const int shade_thr = P.shade_thr0 + (int)wave * P.shade_thr_step;
    uint32_t n_closest = 0, n_light = 0; // per wave and launch: well below 2^32
    unsigned long long n_nodes = 0, n_tris = 0;
    uint32_t idle_spins = 0;
    int gave_up = 0; // 1: the launch ran into its deadline; 2: the workgroup waited in vain for a path to come back (a lost path: a bug)
    PtProf prof;
    PtLap<COUNT> clk; // the role clock of the counting build (prof.t_role)
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime(); // the deadline's clock: deadline_ticks are 100 MHz ticks
    for (;;) {
        if (__builtin_amdgcn_s_memrealtime() - t_start > P.deadline_ticks) { gave_up = 1; break; } // safety net: never hang the GPU; the host reports the error
        const int ns = pt_count(&sh.cnt[PT_Q_SHADE]), nt = pt_count(&sh.cnt[PT_Q_TRACE]), nl = pt_count(&sh.cnt[PT_Q_LIGHT]);
        if (rl.rare(wv)) {
            idle_spins = 0;
            clk.lap(prof.t_role[3]);
            continue;
        }
        // shaders first when a full wave of paths waits (or when it is all there is to do)
        if (ns >= P.shade_min || (ns > 0 && nt + nl == 0)) {
            const uint32_t got = pt_pop(sh.need[PT_Q_SHADE], &sh.cnt[PT_Q_SHADE], wv.nw, wv.cur[PT_Q_SHADE], true, wv.front_first, COUNT ? &prof.pops[PT_Q_SHADE] : nullptr);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (pt_here(P.prio) == 2) __builtin_amdgcn_s_setprio(2);
            const PtShaded s = rl.shade(got, n_light, n_nodes, prof);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (s.trace || s.light) atomicOr(&sh.pending[got >> 4], ((s.trace ? PT_BIT_T : 0u) | (s.light ? PT_BIT_L : 0u)) << ((got & 15u) * 2u));
            pt_push(sh, PT_Q_TRACE, got, s.trace && !s.xtrace); // (a refused hit sets no pending bit and takes no other push: where its push stands does not matter)
            pt_push(sh, PT_Q_LIGHT, got, s.light);
            pt_push(sh, PT_Q_XTRACE, got, s.xtrace);
            if (s.cost) atomicAdd(&sh.cost[got >> pt_gshift(sh)], s.cost);
            const unsigned long long done = pt_ballot(s.done);
            if (done && lane == 0) atomicSub(&sh.cnt[PT_N_LIVE], (int)__popcll(done));
            idle_spins = 0;
            if (pt_here(P.prio) == 2) __builtin_amdgcn_s_setprio(0);
            if (COUNT) { prof.shade_batches++; prof.shade_items += __popcll(pt_ballot(got != PT_NONE)); } // reported by hw8's flush only (CNT_P8_*)
            clk.lap(prof.t_role[2]);
            continue;
        }
        if (nt + nl > 0) {
            // walkers: the kind whose backlog per walking wave (weighted by the cost of a query) is larger
            const long long wt = (long long)nt * P.cost_t * (pt_count(&sh.cnt[PT_W_LIGHT]) + 1), wl = (long long)nl * P.cost_l * (pt_count(&sh.cnt[PT_W_TRACE]) + 1);
            if (pt_here(P.prio) == 1) __builtin_amdgcn_s_setprio(2);
            if (nl == 0 || (nt > 0 && wt >= wl)) {
                if (lane == 0) atomicAdd(&sh.cnt[PT_W_TRACE], 1);
                auto walk = rl.trace_walk();
                pt_walk_stint<RL::SLOTS, RL::DEFER, COUNT>(walk, sh, P, wv, stack, shade_thr, n_closest, n_nodes, n_tris, prof);
                if (lane == 0) atomicSub(&sh.cnt[PT_W_TRACE], 1);
                clk.lap(prof.t_role[0]);
            } else {
                if (lane == 0) atomicAdd(&sh.cnt[PT_W_LIGHT], 1);
                auto walk = rl.light_walk(prof);
                pt_walk_stint<RL::SLOTS, RL::DEFER, COUNT>(walk, sh, P, wv, stack, shade_thr, n_light, n_nodes, n_tris, prof);
                if (lane == 0) atomicSub(&sh.cnt[PT_W_LIGHT], 1);
                clk.lap(prof.t_role[1]);
            }
            if (pt_here(P.prio) == 1) __builtin_amdgcn_s_setprio(0);
            idle_spins = 0;
            if (COUNT) prof.stints++;
            continue;
        }
        if (pt_count(&sh.cnt[PT_N_LIVE]) <= 0) break;
        // paths are in flight in other waves' registers: wait for them
        __builtin_amdgcn_s_sleep(8);
        clk.lap(prof.t_role[4]);
        if (++idle_spins > (1u << 24)) { gave_up = 2; break; } // safety net (seconds): never hang the GPU on a lost path; the host reports it
    }
    if (gave_up && lane == 0 && P.counters) atomicAdd(&P.counters[gave_up == 1 ? CNT_DEADLINE : CNT_LOST_PATH], 1ull);
    pt_leave<RL::THREADS>(sh, P, wv);
    if (P.counters) {
        if (lane == 0 && n_closest) atomicAdd(&P.counters[CNT_CLOSEST], (unsigned long long)n_closest);
        if (lane == 0 && n_light) atomicAdd(&P.counters[CNT_LIGHT], (unsigned long long)n_light);
        if (COUNT) { // node visits and tests are counted per lane, the role times per wave
            atomicAdd(&P.counters[CNT_NODE_VISITS], n_nodes); atomicAdd(&P.counters[CNT_TRI_TESTS], n_tris);
            if (lane == 0) for (int i = 0; i < 5; i++) atomicAdd(&P.counters[CNT_ROLE_TIME + i], prof.t_role[i]);
        }
        rl.flush(lane, prof);
    }
    if (P.debug && lane == 0) atomicMax(&P.debug[3 * blockIdx.x + 1], __builtin_amdgcn_s_memrealtime());
}

// The roles of the hw8 / hw7 kernel.  Its rare role is the exact role (pt_exact_batch); its shader also keeps rays that cross a tripwire
// away from the walkers and settles the light sums whose walk would test no light (PT_LIGHT_SETTLE).
template <bool COUNT_, int FEAT>
struct PtRoles {
    static constexpr bool COUNT = COUNT_;
    static constexpr int THREADS = P8_THREADS;
    static constexpr int SLOTS = 3;      // three parked leaves, deferred endings (pt_walk_stint)
    static constexpr bool DEFER = true;
    const SceneView &S; const RenderView &R; const WfView &W; PtShared &sh; const PtParams &P;
    uint32_t (*stack)[64] = sh.stack[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
    uint32_t n_xtrace = 0, n_xlight = 0, n_discarded = 0; // per wave and launch: well below 2^32
    RT_DEV PtTraceWalk trace_walk() { return PtTraceWalk{S, W, sh, P, stack}; }
    RT_DEV PtLightWalk<COUNT> light_walk(PtProf &prof) { return PtLightWalk<COUNT>{S, W, sh, P, stack, prof}; }
    RT_DEV bool seed(uint32_t slot, uint32_t gslot, int x, int y, Rng &rng, F3 sum) {
        F3 o, d;
        float4 *r = wf_rec(W, slot);
        if constexpr ((FEAT & WF_FEAT_SOURCE) != 0) {
            if (!PtSource<FEAT>::first(S, R, gslot, rng, o, d)) {
                // no path: the state stays as it is, and the record says "every sample is in" to a later phase of the launch (resumed_sample)
                r[3] = make_float4(0.f, 0.f, 0.f, __uint_as_float(wf_pack(0, false, (uint32_t)R.samples)));
                if (P.counters && pt_source_counts<FEAT>(R, gslot)) atomicAdd(&P.counters[CNT_SRC_NO_PATH], 1ull);
                return false;
            }
        } else {
            if (R.sample_seeds) wf_sample_seed(R, rng, gslot, x, y, 0u);
            wf_camera_ray(S, R, rng, x, y, o, d);
        }
        r[0] = make_float4(o.x, o.y, o.z, d.x);
        r[1] = make_float4(d.y, d.z, __uint_as_float(rng.x), rng.saved);
        r[2] = make_float4(0.f, 0.f, 0.f, 0.f);
        r[3] = make_float4(sum.x, sum.y, sum.z, __uint_as_float(wf_pack(0, rng.has_saved, R.accum ? (uint32_t)R.sample_first : 0u)));
        return true;
    }
    RT_DEV uint32_t resumed_sample(uint32_t slot) { return (__float_as_uint(reinterpret_cast<const float *>(wf_rec(W, slot) + 3)[3]) >> 6) & WF_SAMPLE_MASK; }
    RT_DEV bool seed_wire(uint32_t slot) { // the record's ray pierces a tripwire (rt_exact.h): its closest hit is the exact role's
        // (a pixel source's ray is a camera ray, which the walkers were derived for: tripwires only, as the camera kernels)
        if constexpr ((FEAT & WF_FEAT_SOURCE) != 0 && (FEAT & WF_FEAT_PIXELS) == 0) { // ... or it is a first ray the walkers were not derived for (pt_source_exact, which looks at the tripwires too)
            const float4 *nr = wf_rec(W, slot);
            const float4 n0 = nr[0], n1 = nr[1];
            return pt_source_exact(S, f3(n0.x, n0.y, n0.z), f3(n0.w, n1.x, n1.y));
        }
        if (!S.n_tripwire_groups) return false;
        const float4 *nr = wf_rec(W, slot);
        const float4 n0 = nr[0], n1 = nr[1];
        return pt_tripwire(S, f3(n0.x, n0.y, n0.z), f3(n0.w, n1.x, n1.y));
    }
    RT_DEV bool rare(PtWave &wv) {
        const bool queued = pt_count(&sh.cnt[PT_Q_XLIGHT]) + pt_count(&sh.cnt[PT_Q_XTRACE]) > 0;
        if (queued) pt_exact_batch(S, W, sh, wv, &stack[0][0], n_xlight, n_xtrace);
        return queued; // decided before the batch's divergent code: the loop's branch on it stays a scalar one
    }
    RT_DEV PtShaded shade(uint32_t got, uint32_t &n_light, unsigned long long &n_nodes, PtProf &prof) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t slot = got != PT_NONE ? pt_slot(sh, got) : 0u; // once: an LDS read and a readfirstlane each time
        int todo = 0;
        bool discarded = false;
        if (COUNT && P.trace_buf && got != PT_NONE) {
            const uint32_t tslot = slot;
            int tx, ty; bool tin; size_t toi;
            wf_slot_to_pixel(R, tslot + W.slot_base, tx, ty, tin, toi);
            if (tin && ty * R.width + tx == P.trace_pixel) {
                const float4 *tr = wf_rec(W, tslot);
                const uint32_t k = atomicAdd(reinterpret_cast<uint32_t *>(P.trace_buf), 1u);
                if (4u * k + 5u <= P.trace_cap) for (int q = 0; q < 4; q++) P.trace_buf[1 + 4 * k + q] = tr[q];
            }
        }
        PtShadeLap<COUNT> lp;
        if (got != PT_NONE) { PtPark pk; pk.p = (PtLdsWord)&stack[0][lane]; todo = pt_shade_lean<FEAT>(S, R, W, slot, pk, discarded, lp); }
        if constexpr (COUNT) { // each section once per batch: its lanes all hold the same time
            for (int k = 0; k < 5; k++) {
                const unsigned long long m = pt_ballot(lp.d[k] != 0u);
                if (m) { prof.t_shade[k] += (uint32_t)__builtin_amdgcn_readlane((int)lp.d[k], __builtin_ctzll(m)); prof.shade_lanes[k] += __popcll(m); }
            }
            prof.shade_last += __popcll(pt_ballot(lp.last));
        }
        n_discarded += __popcll(pt_ballot(discarded));
        const bool next = got != PT_NONE && todo != PT_SHADE_EXACT && (todo & WF_NEXT_TRACE), with_light = next && (todo & WF_NEXT_LIGHT);
        bool wire = false;    // the new ray pierces a tripwire (rt_exact.h): its closest hit is the exact role's
        bool settled = false; // its light sum is settled here (PT_LIGHT_SETTLE): the walk would test no light
        int settle_steps = 0; // the node steps that decision took (the cost the light walker would have booked)
        if (next && (S.n_tripwire_groups || ((COUNT || PT_LIGHT_SETTLE) && with_light))) {
            const float4 *nr = wf_rec(W, slot);
            const float4 n0 = nr[0], n1 = nr[1];
            const F3 o = f3(n0.x, n0.y, n0.z), d = f3(n0.w, n1.x, n1.y);
            if (S.n_tripwire_groups) wire = pt_tripwire(S, o, d);
            if ((COUNT || PT_LIGHT_SETTLE) && with_light) { // the counting build classifies every sum, whatever it settles
                const int reach = pt_light_reach<COUNT ? 2 : PT_LIGHT_SETTLE>(S, make_ray_grid(S.grid, o, d), settle_steps);
                if (COUNT) { prof.light_reach[0] += reach == 0; prof.light_reach[1] += reach == 1; }
                settled = reach < PT_LIGHT_SETTLE;
                if (settled) { // what the walker's end() does with no hit, before the loop's release publishes the path
                    const int depth = (int)(__float_as_uint(reinterpret_cast<const float *>(nr + 3)[3]) & 15u);
                    float *pdf = reinterpret_cast<float *>(wf_entry(W, slot, depth)) + 3;
                    *pdf = *pdf + 0.f / S.n_lights_f;                      // distributions.h:123,273 (+0.f: a -0 sum becomes +0)
                }
            }
        }
        if constexpr ((FEAT & WF_FEAT_SOURCE) != 0 && (FEAT & WF_FEAT_PIXELS) == 0) { // the next sample's first ray (depth 0, no bounce pending) gets the treatment of the slot's first
            if (next && !wire) {
                const float4 *nr = wf_rec(W, slot);
                if ((__float_as_uint(reinterpret_cast<const float *>(nr + 3)[3]) & (15u | WF_PENDING_BIT)) == 0u) {
                    const float4 n0 = nr[0], n1 = nr[1];
                    wire = pt_source_exact(S, f3(n0.x, n0.y, n0.z), f3(n0.w, n1.x, n1.y));
                }
            }
        }
        n_light += __popcll(pt_ballot(settled)); // a settled sum is still a light-pdf query of the algorithm
        if (COUNT && settled) n_nodes += (unsigned long long)settle_steps;
        PtShaded s;
        s.trace = next;
        s.light = with_light && !settled;
        s.xtrace = (got != PT_NONE && todo == PT_SHADE_EXACT) || wire;
        s.done = got != PT_NONE && (todo == 0 || todo == WF_PARKED); // finished, or parked for the next phase
        if (got != PT_NONE && todo != PT_SHADE_EXACT) s.cost = (uint32_t)PT_COST_SHADE + (settled ? PT_COST_LIGHT_NODE * (uint32_t)settle_steps : 0u);
        return s;
    }
    RT_DEV void flush(uint32_t lane, const PtProf &prof) {
        if (lane == 0) {
            if (n_discarded) atomicAdd(&P.counters[CNT_DISCARDED], (unsigned long long)n_discarded);
            if (n_xtrace) atomicAdd(&P.counters[CNT_EXACT_CLOSEST], (unsigned long long)n_xtrace);
            if (n_xlight) atomicAdd(&P.counters[CNT_EXACT_LIGHT], (unsigned long long)n_xlight);
        }
        if (!COUNT) return;
        atomicAdd(&P.counters[CNT_P8_LIGHT_HITS], prof.light_hits); atomicAdd(&P.counters[CNT_P8_LIGHT_TESTS], prof.light_tests);
        atomicAdd(&P.counters[CNT_P8_LIGHT_REACH], prof.light_reach[0]); atomicAdd(&P.counters[CNT_P8_LIGHT_REACH + 1], prof.light_reach[1]);
        if (lane == 0) { // wave-level profile, words 21..27 and 48..63
            atomicAdd(&P.counters[CNT_P8_WALK_ITERS], prof.iters[0]); atomicAdd(&P.counters[CNT_P8_WALK_ITERS + 1], prof.lane_iters[0]);
            atomicAdd(&P.counters[CNT_P8_WALK_ITERS + 2], prof.iters[1]); atomicAdd(&P.counters[CNT_P8_WALK_ITERS + 3], prof.lane_iters[1]);
            atomicAdd(&P.counters[CNT_P8_STINTS], prof.stints); atomicAdd(&P.counters[CNT_P8_SHADE_BATCHES], prof.shade_batches); atomicAdd(&P.counters[CNT_P8_SHADE_ITEMS], prof.shade_items);
            for (int k = 0; k < 3; k++) atomicAdd(&P.counters[CNT_P8_HANDOFF_TIME + k], prof.t_sub[0][k]);
            atomicAdd(&P.counters[CNT_P8_HANDOFFS], prof.refills[0]);
            for (int k = 0; k < 5; k++) { atomicAdd(&P.counters[CNT_P8_SHADE_TIME + k], prof.t_shade[k]); atomicAdd(&P.counters[CNT_P8_SHADE_LANES + k], prof.shade_lanes[k]); }
            atomicAdd(&P.counters[CNT_P8_SHADE_LAST], prof.shade_last);
            for (int q = 0; q < 3; q++) {
                atomicAdd(&P.counters[CNT_P8_POPS + 3 * q], prof.pops[q].pops); atomicAdd(&P.counters[CNT_P8_POPS + 3 * q + 1], prof.pops[q].paths);
                atomicAdd(&P.counters[CNT_P8_POPS + 3 * q + 2], prof.pops[q].words);
            }
            for (int w = 0; w < 2; w++) {
                for (int k = 0; k < 3; k++) atomicAdd(&P.counters[CNT_P8_WALK_TIME + 3 * w + k], prof.t_part[w][k]);
                atomicAdd(&P.counters[CNT_P8_LEAF_ITERS + 2 * w], prof.leaf_iters[w]); atomicAdd(&P.counters[CNT_P8_LEAF_ITERS + 2 * w + 1], prof.leaf_lane_iters[w]);
            }
        }
    }
};

// __launch_bounds__(256, 5): five waves per SIMD, i.e. a budget of 96 VGPRs.  Every role fits it without scratch; the scheduler's own
// state is wave-uniform and lives in SGPRs (pt_count / readfirstlane).
template <bool COUNT, int FEAT>
__global__ __launch_bounds__(P8_THREADS, P8_PER_CU) void pt_persistent_kernel(SceneView S, RenderView R, WfView W, PtParams P) {
    __shared__ PtShared sh;
    PtRoles<COUNT, FEAT> roles{S, R, W, sh, P};
    pt_run(roles);
}

} // namespace dev
} // namespace rtamd

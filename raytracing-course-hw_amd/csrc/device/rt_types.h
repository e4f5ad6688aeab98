// Flat HBM layouts shared by the host preparation (scene_prep.cpp) and the HIP kernels.
// Everything is plain old data, 16-byte aligned records so one lane fetches a record with
// global_load_dwordx4 instructions.
#pragma once
#include <stdint.h>

namespace rtamd {

// Limits that scene creation and the frame geometry check and the kernels size their stacks by.
#define RT_MAX_DEPTH 16               // ray_depth of the hw8 / hw7 integrators
#define RT_STACK_SIZE 64              // private traversal stack of the megakernel and of the exact walks over the reference's own tree
#define P8_STACK 24                   // rt_persistent.h: LDS traversal stack entries per lane; the walkers' tree is built at most this deep (rt_bvh_build.h)

// The 80 counters of a render (8 bytes each; RenderView::counters / PtParams::counters), zeroed before every frame and read back after
// it for rt_stats, the error checks and the RTAMD_DEBUG_COUNTERS report (render_frame, report_persistent).  One name per meaning: where
// two kernels use a slot differently it has two names, and the comment says who writes it (P8 = pt_persistent_kernel, P6 =
// p6_persistent_kernel, WF = the round pipeline's kernels, mega = render_hw8_kernel / render_hw6_kernel).
enum CounterSlot {
    CNT_CLOSEST = 0,            // closest-hit queries: P8, P6, mega; WF: summed by the host from the rounds' queue lengths
    CNT_LIGHT = 1,              // light-pdf queries: likewise
    CNT_NODE_VISITS = 2,        // counting variants of P8, P6, WF, render_hw8_kernel
    CNT_TRI_TESTS = 3,
    CNT_WF_NODE_ITERS = 4,      // WF closest-hit walker (WfTraceWalk): wave node-iterations, ...
    CNT_WF_LEAF_PHASES = 5,
    CNT_WF_LEAF_LANES = 6,
    CNT_WF_REFILLS = 7,
    CNT_WF_LANE_NODES = 8,      // ... and its own share of CNT_NODE_VISITS / CNT_TRI_TESTS
    CNT_WF_LANE_TRIS = 9,
    CNT_DISCARDED = 10,         // speculative closest hits that the clamp step discarded: P8, WF wf_shade_item
    CNT_WF_SLOW_LIGHT = 11,     // WF: light sums finished by wf_light_exact_kernel (summed by the host from the rounds' counters)
    CNT_P6_EXACT_LIGHT = 11,    // P6: exact light sums
    CNT_EXACT_CLOSEST = 12,     // exact closest hits: P8, P6, WF wf_trace_exact_kernel
    CNT_EXACT_LIGHT = 13,       // exact light sums: P8; WF: the host's copy of CNT_WF_SLOW_LIGHT
    CNT_P6_SLOW_LIGHT = 13,     // P6: light sums through the slow role
    CNT_LOST_PATH = 14,         // P8, P6: waves that gave up waiting for a lost path (an error)
    CNT_WANT_HISTOGRAMS = 15,   // request, set by the host (RTAMD_DEBUG_COUNTERS): WF's counting kernels fill the two histograms
    CNT_WF_HIST_CLOSEST = 16,   // WF, 16 slots: closest-hit queries by in-flight wave iterations / 32
    CNT_ROLE_TIME = 16,         // P8, P6, 5 slots: wave time by role in shader-clock cycles (closest-hit walks, light walks, shading, rare roles — P8: exact walks, P6: slow light sums and exact walks —, idle)
    CNT_P8_WALK_ITERS = 21,     // P8, 2 slots per walker (closest hit, light): wave iterations, lane iterations
    CNT_P8_STINTS = 25,
    CNT_P8_SHADE_BATCHES = 26,
    CNT_P8_SHADE_ITEMS = 27,
    CNT_SRC_NO_PATH = 28,       // P8 with a path source (rt_path_source.h): records that started no path (rays: invalid records; bake: invalid points)
    CNT_DEADLINE = 29,          // P8, P6: waves that ran into the launch deadline (an error)
    CNT_P8_LIGHT_REACH = 30,    // P8, 2 slots: light sums whose walk ends at the light tree's root / one level below it (pt_light_reach)
    CNT_WF_HIST_LIGHT = 32,     // WF, 16 slots: light queries by in-flight wave iterations / 32
    CNT_P6_SLOW_HITS = 32,      // P6, 16 slots: light sums in the slow role by number of hits
    CNT_P8_POPS = 32,           // P8, 3 slots per queue (trace, light, shade): pt_pop calls, paths they handed out, bitmap words those came from
    CNT_P8_WALK_TIME = 48,      // P8, 3 slots per walker: hand-off and refill, inner nodes, leaves
    CNT_P8_LEAF_ITERS = 54,     // P8, 2 slots per walker: leaf passes, their lanes
    CNT_P8_LIGHT_HITS = 58,
    CNT_P8_LIGHT_TESTS = 59,
    CNT_P8_HANDOFF_TIME = 60,   // P8, 3 slots: the closest-hit walker's hand-off time by part (publish, take, read rays)
    CNT_P8_HANDOFFS = 63,       // P8: the closest-hit walker's hand-off points
    CNT_P8_SHADE_TIME = 64,     // P8, 5 slots: the shader's wave time by section (record load, gate and pending bounce; attributes and textures; Mix::sample; BRDF and pdf; path end)
    CNT_P8_SHADE_LANES = 69,    // P8, 5 slots: the lanes that ran each section, summed over the batches
    CNT_P8_SHADE_LAST = 74,     // P8: shaded hits at the deepest level (lanes, summed over the batches)
    CNT_SLOTS = 80
};
#define CNT_BYTES (CNT_SLOTS * sizeof(unsigned long long)) // the 640-byte block

// Binary BVH node with BOTH child boxes inline (one 64-byte fetch decides both children).
// child = index of an inner node, or 0x80000000|first for a leaf whose primitives run from `first`
// up to the record whose `pad` word is 1 (cnt repeats the count for diagnostics), or 0xFFFFFFFF (empty).
// Boxes are padded conservatively on the host (see scene_prep.cpp pad_box).
struct GpuNode {
    float lo0[3]; int32_t child0;
    float hi0[3]; int32_t cnt0;
    float lo1[3]; int32_t child1;
    float hi1[3]; int32_t cnt1;
};
static_assert(sizeof(GpuNode) == 64, "GpuNode must be 64 bytes");

// Walk node of the persistent pipeline: the children of a GpuNode's two children (a child that is a leaf stays as it is), each as one
// 16-byte record {x, y, z, child}: two levels of the tree per fetch of one 64-byte line — half the dependent node fetches of a walk.
// The boxes lie on a 16-bit grid over the scene (NodeGrid), rounded outwards and one more cell: x = lo | hi << 16 along x, and so on.
// The walkers move the ray into grid coordinates once per walk; a box of the grid contains the float box whatever that arithmetic
// rounds (rt_device.h slab_test_q).  Unused records: child = 0xFFFFFFFF, a point in the grid's border.
struct GpuNode4Q { uint32_t rec[4][4]; };
static_assert(sizeof(GpuNode4Q) == 64, "GpuNode4Q must be 64 bytes");
#define RT_GRID_CELLS 65000.0   // cells across the larger of: the axis' own extent, 1/64 of the largest extent
#define RT_GRID_BORDER 4        // cells in front of the lowest box
struct NodeGrid { float lo[3], step[3], istep[3]; };

// Per-triangle intersection record, in the reference's BVH (figure) order.  All derived values are
// computed on the host with the reference's float expressions (hw8/src/primitives.cpp:85-104), so
// the kernel's test is bit-identical to Figure::intersectAsTriangle while fetching only 48 bytes.
struct TriIsect {
    float ax, ay, az;   // a = data3.coords
    float nx, ny, nz;   // n = b.cross(c) (negated cross convention), b = data - a, c = data2 - a
    float a1, b1;       // magic1 . b, magic1 . c
    float a2, b2;       // magic2 . b, magic2 . c
    float den;          // b1*a2 - a1*b2
    uint32_t pad;       // triangle arrays: bit 0 = last record of its leaf, bits 1.. = the triangle's index in the figure order (what a hit
                        // reports and the tie rule compares); light arrays: 1 = last record of its leaf
};
static_assert(sizeof(TriIsect) == 48, "TriIsect must be 48 bytes");

// Per-triangle shading record (fetched once per hit): interpolation bases and deltas
// (hw8/src/primitives.cpp:110-117) plus material.
struct TriShade {
    float n3[3], dn1[3], dn2[3];   // data3.normals, data.normals-data3.normals, data2.normals-data3.normals
    float t3[3], dt1[3], dt2[3];   // same for tangents.v
    float uv3[2], duv1[2], duv2[2];
    float tanw;                    // data.tangents.w
    uint32_t material;
    uint32_t orig;                 // LOAD-order index (diagnostics)
    uint32_t pad;
};
static_assert(sizeof(TriShade) == 112, "TriShade must be 112 bytes");

// Emissive triangle in the reference's light order (hw8/src/include/distributions.h:60-115).
struct LightRec {
    TriIsect isect;                // for pdfOneFigureLight's intersection test
    float b[3], c[3];              // for TriangleLight::sample: point = a + u*b + v*c
    float point_prob;              // 1 / area
    float n3[3], dn1[3], dn2[3];   // shading-normal interpolation (pdfOne uses the shading normal in hw8)
    float box_lo[3], pad0;         // the light's own box: min / max over a, a + b, a + c in float (what the robustness test of rt_exact.h compares a hit
    float box_hi[3], pad1;         // point with; formed on the host instead of 24 instructions per light hit)
};
static_assert(sizeof(LightRec) == 48 + 64 + 32, "LightRec must be 144 bytes");
// What a LightRec holds after its TriIsect.  The persistent kernel's light walker keeps its own copy of the lights as a pair of arrays, the TriIsect
// of every light packed (what a light test reads: 48-byte records share no 64-byte line with anything a test does not read) and the LightRest of
// every light (what a hit reads): record k of the pair is LightRec k of the walker's leaf order, byte for byte.
struct LightRest {
    float b[3], c[3];
    float point_prob;
    float n3[3], dn1[3], dn2[3];
    float box_lo[3], pad0;
    float box_hi[3], pad1;
};
static_assert(sizeof(LightRest) == sizeof(LightRec) - sizeof(TriIsect) && sizeof(LightRest) == 96, "LightRest must be the 96 bytes of a LightRec after its TriIsect");

// The persistent pipeline's walkers read their arrays (nodes4, light_walk_nodes4, tri_walk, lights_walk_test / lights_walk_rest) at 32-bit byte offsets from a scalar
// base, a record's offset formed by a 24-bit multiply (rt_device.h GlobalBytes, record_ofs): at most 2^24 records each — the 24-bit figure index
// bounds the triangles, hence the lights and the nodes — and every array below 4 GiB (2^24 LightRest are 1.6 GB).  Scene creation checks it.
#define RT_WALK_MAX_RECORDS (1u << 24)
inline bool walk_arrays_fit(uint64_t n_tris, uint64_t n_lights, uint64_t n_nodes, uint64_t n_light_nodes) {
    const uint64_t lim = 1ull << 32;
    return n_tris <= RT_WALK_MAX_RECORDS && n_lights <= RT_WALK_MAX_RECORDS && n_tris * sizeof(TriIsect) < lim && n_lights * sizeof(LightRest) < lim &&
           n_nodes * sizeof(GpuNode4Q) < lim && n_light_nodes * sizeof(GpuNode4Q) < lim;
}

// Node of the reference's own tree with its UNPADDED box (hw8/src/include/bvh.h:9-16), for the reference-exact walks of
// rt_persistent.h: left == 0 marks a leaf holding the figures (lights) [first, last) of the reference order.
struct GpuRefNode {
    float mn[3]; uint32_t left;
    float mx[3]; uint32_t right;
    uint32_t first, last, pad0, pad1;
};
static_assert(sizeof(GpuRefNode) == 48, "GpuRefNode must be 48 bytes");

struct GpuMaterial {
    float base_color[3]; float metallic_factor;
    float emission[3];   float roughness_factor;
    int32_t base_color_tex, emissive_tex, metallic_roughness_tex, normal_tex; // image slot or -1
};
static_assert(sizeof(GpuMaterial) == 48, "GpuMaterial must be 48 bytes");

struct GpuImage {
    uint64_t offset; // byte offset of the RGB8 data in the texel buffer
    int32_t width, height;
};

// Device-side view of a prepared scene (pointers into HBM).
struct SceneView {
    const GpuNode *nodes;          // scene BVH, root = 0
    const TriIsect *tri_isect;     // figure order (the reference's BVH order; LOAD order under RT_BUILD_DEVICE_BVH): shading, exact walks
    float cull_k;                  // walkers prune boxes against best_t (1 + cull_k): the tie tolerance of the leaf test plus the slab test's rounding
    const TriIsect *tri_walk;      // the same records in the leaf order of `nodes` (== tri_isect when `nodes` is the reference topology)
    const TriShade *tri_shade;
    const GpuNode *light_nodes;    // light BVH in the reference's topology, root = 0
    const LightRec *lights;
    // The persistent kernel's light walker: a tree of the library's own over the lights (GPU-built over their reference leaf boxes) and the light
    // records in ITS leaf order (lights_walk_test / lights_walk_rest), pad = light index (position in `lights`) << 1 | last-of-leaf.  == light_nodes /
    // lights with pads rewritten when the scene has too few lights to bother (then the index is the position).
    const GpuNode *light_walk_nodes;
    const float *tripwires;        // host/scene_prep.h: boxes a ray must not pierce unnoticed (8 floats per record: groups, then members); rt_exact.h pt_tripwire
    uint32_t n_tripwire_groups;
    const GpuNode4Q *nodes4, *light_walk_nodes4;  // `nodes` / `light_walk_nodes` four wide on the 16-bit grid: what the persistent pipeline's walkers read
    NodeGrid grid;                 // covers both trees' root boxes and the camera (every ray origin lies inside it)
    const TriIsect *lights_walk_test;   // the walker's light records as a pair of arrays (LightRest above): what a test reads ...
    const LightRest *lights_walk_rest;  // ... and what a hit reads
    const uint16_t *light_sep;     // range-minimum table of the separation depths of neighbouring lights (scene_prep.h)
    const GpuMaterial *materials;
    const GpuImage *images;
    const uint8_t *texels;
    const float *srgb_lut;         // 256 entries: powf(float(1/255.)*b, 2.2f) evaluated by the host libm
    // reference-exact box decisions (rt_persistent.h): the reference's trees with unpadded boxes, per figure its own box
    // (min, max — primitives.cpp:130-141), and the robustness margin c2 = 2^-20 * max |coordinate| of scene and camera
    const GpuRefNode *ref_nodes, *ref_light_nodes;
    const float *tri_box;          // 8 floats per figure: min.xyz, 0, max.xyz, 0
    float box_c2;
    float box_c2x;                 // 1.25f * box_c2 (the walkers' absolute look-behind, rt_exact.h)
    uint32_t exact_boxes;          // 0 = accept every hit of the conservative walk (the round pipeline's behaviour)
    uint32_t n_tris, n_lights, n_components;
    float n_lights_f, n_components_f; // the same numbers as floats (exact): a conversion in the kernel would sit in a VGPR for the whole launch
    uint32_t n_nodes;              // inner nodes of the scene BVH (`nodes`)
    // 1 when every material has 0 <= metallicFactor <= 1 and a non-negative base colour: then the BRDF is >= 0,
    // the throughput of the deepest level is in [0, inf] or NaN, and that level returns exactly its emission
    // (emission + mult*0, or emission via the clamp) — the wavefront path then skips its BRDF/pdf work.
    uint32_t last_level_emission_only;
    // 1 = replay the hw7 snapshot on this scene (set per render): no textures / normal map / environment, alpha =
    // roughness^2 without the 0.08 floor, the ungated BRDF of hw7/src/include/material.h:44-61, and the GEOMETRIC normal in
    // the light pdf (hw7/src/include/distributions.h:140-145).
    uint32_t hw7;
    int32_t env_image;             // image slot of the environment map or -1
    float cam_pos[3], cam_right[3], cam_up[3], cam_fwd[3];
    float bg[3];
    float tan_fov_y;               // (float)tan((double)(fovY / 2)), hw8/src/scene.cpp:180
};

// The camera of one view of a view set (include/rtamd.h: rt_views_*; rt_path_source.h, src_mode 5): what wf_camera_ray takes from the
// scene and the frame, per view.  64 bytes, 16-byte aligned: a first ray reads it as four 16-byte words.
struct alignas(16) ViewCamera {
    float pos[3], right[3], up[3], fwd[3];
    float tan_fov_x, tan_fov_y;    // (float)tan((double)(fov_y / 2)) * width / height and (float)tan((double)(fov_y / 2)), hw8/src/scene.cpp:180-181
    float pad[2];
};
static_assert(sizeof(ViewCamera) == 64, "a view's camera is four 16-byte words");

struct RenderView {
    int32_t width, height, samples, ray_depth;
    int32_t sample_stop;           // a path that reaches this sample index parks (its camera ray is in its record): the persistent
                                   // pipeline renders a frame in phases and re-deals the pixels between them; = samples otherwise
    int32_t tile_w, tile_h, tiles_x, tiles_y;
    int32_t shard_index, shard_count;
    uint32_t n_shard_tiles;
    float tan_fov_x;               // tanFovY * width / height, hw8/src/scene.cpp:181
    float inv_samples;             // (float)(1.0 / samples), hw8/src/scene.cpp:176
    float *out_rgb;                // nullable
    uint8_t *out_rgb8;             // nullable
    uint32_t *work_counter;        // dynamic tile queue head
    unsigned long long *counters;  // nullable: CNT_SLOTS counters (CounterSlot)
    // Throughput mode (rt_render_params.sample_streams = K > 1, wavefront path only): K independent random streams per pixel,
    // `samples` is then the count PER STREAM, path slot = stream * n_pixslots + pixel slot, every slot leaves its unnormalised
    // sum in `partial` and wf_reduce_streams_kernel adds the K sums of a pixel in stream order.
    int32_t streams;               // 0 or 1 = replay mode (the reference's one stream per pixel)
    uint32_t n_pixslots;           // pixel slots of this shard (64 per 8x8 sub-tile)
    uint32_t seed_stride;          // stream k of pixel i is seeded with i + k * seed_stride (= width * height)
    float *partial;                // [streams][n_pixslots][3]
    uint32_t sample_seeds;         // throughput mode, RT_FLAG_SAMPLE_SEEDS: every sample seeds its own engine (hash of pixel and sample)
    uint32_t total_samples;        // samples per pixel over all its streams
    int32_t rr_depth;              // throughput mode, RT_FLAG_RUSSIAN_ROULETTE: first bounce index that plays roulette (0 = off)
    // Resumable renders (rt_accum_*, replay mode): a launch advances every pixel from sample `sample_first` to sample `samples`
    // (both absolute, as the indices in the path records are).  Paths start from the per-pixel-slot state instead of a seed
    // and a path that reaches `samples` leaves its sum and engine there instead of writing a pixel.  Layout (rt_wavefront.h
    // accum_enter / accum_leave): n_pixslots x {sum.x, sum.y, sum.z, Rng::x}, then n_pixslots x {Rng::saved, Rng::has_saved}.
    uint32_t *accum;               // nullable: null = a one-shot frame
    int32_t sample_first;
    // The path source of the persistent hw8 kernel (rt_path_source.h, kernels compiled with WF_FEAT_SOURCE): where a sample's first ray comes
    // from.  Every other launch leaves these zero.  Indexed by the record index, which is the pixel slot (frame geometry: rt_path_source.h).
    uint32_t src_mode;             // 0 = the camera, 1 = the caller's rays, 2 = bake irradiance, 3 = SH9 probes, 4 = the pixels of another frame, 5 = a batch of cameras
    uint32_t src_n;                // records (mode 2: points x streams); a slot at or beyond it starts no path
    union {                        // one pointer's room: the struct, and with it every kernel's argument block, is laid out as before mode 3
        const float *src_rays;     // mode 1: src_n x {o.xyz, d.xyz} (rt_ray), used as given
        float *src_sh;             // mode 3: src_n rounded up to 64 x {first direction xyz, 27 accumulators [m][c]}, slot-major, 8-byte aligned
        const uint32_t *src_pixels; // mode 4: src_n x (x | y << 16), the pixel of the real frame behind the strip slot (ad_gather_kernel, rt_adaptive.h)
                                   // mode 5: the same (vw_gather_kernel, rt_views.h), then src_n / 64 x the view index of each 64-slot group
    };
    union {                        // again one pointer's room, for mode 4, which has no points
        const float *src_points;   // mode 2 and 3: src_n / src_streams x {p.xyz, n.xyz} (rt_bake_point)
        int32_t src_frame[2];      // mode 4: width and height of the real frame, which wf_camera_ray takes in place of the strip's
        const ViewCamera *src_cameras; // mode 5: one record per view of the set, indexed by the group's view index
    };
    union {
        uint32_t src_streams;      // mode 2 and 3: slots per point
        float src_tan_fov_x;       // mode 4: the real frame's tan_fov_x
        uint32_t src_wh;           // mode 5: width | height << 16 of the views' frame (both at most 65,535)
    };
};

} // namespace rtamd

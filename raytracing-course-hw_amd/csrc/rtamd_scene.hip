// C-ABI of the scene (include/rtamd.h): rt_scene_create and what goes with it, and the host-side file front-end.  No kernels here:
// the renders are in rtamd_api.hip, the on-device tree builder in rtamd_build.hip.
// No CPU fallback exists: every entry point that needs the GPU fails with RT_ERR_NO_DEVICE / RT_ERR_HIP when HIP is unusable.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtamd.h"
#include "host/host_scene.h"
#include "host/png.h"
#include "host/scene_prep.h"
#include "host/shared_prep.h"
#include "host/device_build.h"
#include "host/knobs.h"
#include "host/rt_scene.h"
#include "device/rt_node_grid.h"

namespace rtamd {
static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }
}
using namespace rtamd;

namespace {

struct OwnedTree {
    DeviceTree t;
    ~OwnedTree() { free_device_tree(t); }
};

// A tree built on the device over n boxes, and the n records `d_records` gathered into its leaf order (`gathered`); the scene owns both.
// Of the returned tree only `nodes` and the numbers are left.  depth_cap: the stack column of the kernel that walks the tree;
// the record's size, mark_word, or_into_word: gather_records (device_build.h).
template <class Rec>
DeviceTree build_leaf_ordered(rt_scene *s, const float *d_boxes, const Rec *d_records, uint32_t n, float box_pad, uint32_t depth_cap,
                              int mark_word, bool or_into_word, const Rec *&gathered) {
    OwnedTree tree;
    tree.t = build_tree_on_device(d_boxes, n, box_pad, depth_cap);
    OwnedDev out;
    HIP_CHECK(hipMalloc(&out.p, (size_t)n * sizeof(Rec)));
    gather_records(d_records, out.p, tree.t, n, sizeof(Rec), mark_word, or_into_word);
    HIP_CHECK(hipDeviceSynchronize());
    s->allocations.reserve(s->allocations.size() + 2);
    s->allocations.push_back(tree.t.nodes);
    s->allocations.push_back(out.p);
    gathered = (const Rec *)out.release();
    DeviceTree t = tree.t;
    t.order = nullptr; t.last = nullptr; // these two go with the OwnedTree,
    tree.t.nodes = nullptr;              // the nodes are the scene's
    return t;
}

// The walk nodes of the persistent pipelines: both trees four wide on one 16-bit grid that also holds the camera (rt_types.h GpuNode4Q).
void make_walk_nodes(rt_scene *s, const float cam_pos[3], const GpuNode *nodes, uint32_t n_nodes, const GpuNode *light_nodes, uint32_t n_light_nodes,
                     bool join_light_root, NodeGrid &grid, const GpuNode4Q *&nodes4, const GpuNode4Q *&light_nodes4, uint64_t &bytes) {
    float glo[3], ghi[3];
    for (int k = 0; k < 3; k++) glo[k] = ghi[k] = cam_pos[k];
    join_root_box(nodes, glo, ghi);
    if (join_light_root) join_root_box(light_nodes, glo, ghi);
    grid = make_node_grid(glo, ghi);
    uint32_t n4 = 0, n4l = 0, depth4 = 0;
    s->allocations.push_back(widen_nodes(nodes, n_nodes, grid, n4, depth4));
    nodes4 = (const GpuNode4Q *)s->allocations.back();
    s->allocations.push_back(widen_nodes(light_nodes, n_light_nodes, grid, n4l, depth4));
    light_nodes4 = (const GpuNode4Q *)s->allocations.back();
    bytes += ((uint64_t)n4 + n4l) * sizeof(GpuNode4Q);
}

template <class View> void set_camera(View &V, const rt_scene_desc &desc) {
    for (int k = 0; k < 3; k++) {
        V.cam_pos[k] = desc.camera.position[k]; V.cam_right[k] = desc.camera.right[k];
        V.cam_up[k] = desc.camera.up[k]; V.cam_fwd[k] = desc.camera.forward[k];
        V.bg[k] = desc.bg_color[k];
    }
}

// What every scene ends with: the tile queue's head, the counters, the frame's events; then it is the caller's.
// t0 / t1: when the host-side preparation began and ended.
int finish_scene(std::unique_ptr<rt_scene> &s, rt_scene **out, uint64_t bytes, double t0, double t1) {
    HIP_CHECK(hipMalloc((void **)&s->d_work_counter, 64));
    s->allocations.push_back(s->d_work_counter);
    HIP_CHECK(hipMalloc((void **)&s->d_counters, CNT_BYTES));
    s->allocations.push_back(s->d_counters);
    HIP_CHECK(hipEventCreate(&s->ev_start));
    HIP_CHECK(hipEventCreate(&s->ev_stop));
    HIP_CHECK(hipDeviceSynchronize());
    s->info.device_bytes = bytes;
    s->info.prep_ms = t1 - t0; s->info.upload_ms = now_ms() - t1;
    *out = s.release();
    return RT_OK;
}

// Uploads a prepared array, hands it to the scene (which frees it) and counts its bytes.
struct Uploader {
    rt_scene *s;
    uint64_t bytes = 0;
    template <class T> const T *operator()(const std::vector<T> &v) { s->allocations.push_back((void *)upload(v, bytes)); return (const T *)s->allocations.back(); }
};
// What the three flavours upload and report alike: the reference's own two trees, for the exact walks, and the light order and
// rt_scene_info; n_nodes, bvh_depth: of the scene tree the kernels walk, the prepared one or one built on the device.
template <class View> void upload_ref_trees(View &V, const PreparedTrees &P, Uploader &up) { V.ref_nodes = up(P.ref_nodes); V.ref_light_nodes = up(P.ref_light_nodes); }
void report_trees(rt_scene *s, const rt_scene_desc *desc, const PreparedTrees &P, uint32_t n_lights, uint32_t n_nodes, uint32_t bvh_depth) {
    s->light_order = P.light_order;
    s->info.n_triangles = desc->n_triangles; s->info.n_lights = n_lights;
    s->info.n_bvh_nodes = n_nodes; s->info.n_light_bvh_nodes = (uint32_t)P.light_nodes.size();
    s->info.bvh_depth = bvh_depth; s->info.light_bvh_depth = P.light_bvh_depth;
}

// What the views of the two triangle flavours are told alike; components: of the reference's mix without lights (hw6 scene.cpp:8-16, hw8 scene.cpp:65-74).
template <class View> void set_triangle_view(View &V, const rt_scene_desc &desc, const PreparedTriangles &P, uint32_t components) {
    V.box_c2 = P.box_c2; V.box_c2x = 1.25f * P.box_c2;
    V.cull_k = (float)env_float("RTAMD_CULL_K", 0.0078125); // how far behind the best hit the walkers still look, relative to t (rt_exact.h)
    V.n_tris = desc.n_triangles;
    V.n_lights = (uint32_t)P.light_order.size();
    V.n_components = components + (V.n_lights ? 1u : 0u);
    V.n_lights_f = (float)V.n_lights; V.n_components_f = (float)V.n_components;
    set_camera(V, desc);
    V.tan_fov_y = (float)std::tan((double)(desc.camera.fov_y / 2)); // scene.cpp:180 (host libm, like the reference)
}

// Analytic primitives only: a .txt scene (hw1 .. hw5).
int create_txt(const rt_scene_desc *desc, std::unique_ptr<rt_scene> &s, rt_scene **out, double t0) {
    PreparedSceneTxt T;
    prepare_scene_txt(*desc, T);
    PreparedScene5 P5; // hw5 structures: reference figure order, BVH over the non-planes, light list + light BVH
    prepare_scene_hw5(*desc, P5);
    Uploader up{s.get()};
    s->txt_has_triangles = T.has_triangles;
    SceneViewTxt &V = s->viewt;
    V.prims = up(T.prims);
    V.n_prims = desc->n_primitives;
    set_camera(V, *desc);
    V.tan_fov_x = (float)std::tan((double)(desc->camera.fov_x / 2)); // hw3/src/scene.cpp:100
    V.tan_fov_x_f = tanf(desc->camera.fov_x / 2);                    // hw1/src/scene.cpp:23, hw2/src/scene.cpp:91 (<math.h>: float overload)
    V.n_lights = desc->n_lights;
    if (desc->n_lights) V.lights = up(T.lights);
    for (int k = 0; k < 3; k++) V.ambient[k] = desc->ambient_light[k];
    V.n_light_prims = (uint32_t)T.light_prims.size();
    if (!T.light_prims.empty()) V.light_prims = up(T.light_prims);
    SceneView5 &V5 = s->view5;
    V5.nodes = up(P5.nodes);
    V5.figs = up(P5.figs);
    V5.light_nodes = up(P5.light_nodes);
    upload_ref_trees(V5, P5, up);
    if (!P5.lights.empty()) V5.lights = up(P5.lights);
    V5.n_figs = (uint32_t)P5.figs.size(); V5.n_nonplanes = P5.n_nonplanes; V5.n_lights = (uint32_t)P5.lights.size();
    set_camera(V5, *desc);
    V5.tan_fov_x = V.tan_fov_x;
    report_trees(s.get(), desc, P5, V5.n_lights, (uint32_t)P5.nodes.size(), P5.bvh_depth);
    s->flavor = RT_INTEGRATOR_HW3;
    return finish_scene(s, out, up.bytes, t0, t0); // the preparation is no work to speak of: all of it counts as upload
}

// hw6: flat shading, no per-vertex normals (hw6/src/sceneio.cpp:186-225).
int create_hw6(const rt_scene_desc *desc, std::unique_ptr<rt_scene> &s, rt_scene **out, double t0) {
    // hw6's scene tree is the library's own (the reference's is degenerate, rt_kernels_hw6.h), so it can be built on the GPU
    // without touching the replay: the tie rule reads the reference's figure index from the record.
    const bool tree_on_device = desc->n_triangles >= 64 && !env_flag("RTAMD_HOST_BVH");
    PreparedScene6 P6;
    prepare_scene_hw6(*desc, P6, tree_on_device);
    uint32_t bvh_depth = P6.bvh_depth, n_nodes = (uint32_t)P6.nodes.size();
    double t1 = now_ms();
    Uploader up{s.get()};
    SceneView6 &V = s->view6;
    if (tree_on_device) {
        uint64_t scratch = 0;
        OwnedDev d_load(upload(P6.tris, up.bytes)); // device_bytes: stands for the gathered copy of the same size, which the scene keeps
        OwnedDev d_boxes(upload(P6.boxes8, scratch));
        const DeviceTree t = build_leaf_ordered(s.get(), (const float *)d_boxes.p, (const Tri6 *)d_load.p, desc->n_triangles, P6.box_pad, 28, // hw6 walkers: 36-entry stack columns
                                                13, false, V.tris);                                                                         // word 13 = Tri6::last
        V.nodes = t.nodes;
        up.bytes += (uint64_t)t.n_nodes * sizeof(GpuNode);
        bvh_depth = t.depth;
        n_nodes = t.n_nodes;
        s->info.bvh_build_ms = t.build_ms; s->info.bvh_on_device = 1;
    } else {
        V.nodes = up(P6.nodes);
        V.tris = up(P6.tris);
    }
    if (bvh_depth > RT6_STACK_SIZE - 2 || P6.light_bvh_depth > RT6_STACK_SIZE - 2 || P6.fast_light_bvh_depth > RT6_STACK_SIZE - 2)
        return fail(RT_ERR_LIMIT, "scene BVH deeper than the kernel's traversal stack (" + std::to_string(bvh_depth) + "/" +
                                      std::to_string(P6.light_bvh_depth) + ")");
    s->hw6_lds_stack = bvh_depth <= RT6_LDS_STACK && P6.fast_light_bvh_depth <= RT6_LDS_STACK; // both own trees fit the LDS stack columns
    s->hw6_pt_stack = bvh_depth <= P6_STACK && P6.fast_light_bvh_depth <= P6_STACK;           // ... of the persistent pipeline
    V.light_nodes = up(P6.light_nodes);
    V.lights = up(P6.lights);
    V.fast_light_nodes = up(P6.fast_light_nodes);
    V.fast_lights = up(P6.fast_lights);
    V.light_ref = up(P6.light_ref);
    upload_ref_trees(V, P6, up);
    V.ref_tris = up(P6.ref_tris);
    V.tri_box = up(P6.tri_box);
    set_triangle_view(V, *desc, P6, 1u);
    V.exact_boxes = env_flag("RTAMD_NO_EXACT_BOXES") ? 0u : 1u;
    V.light_sep = up(P6.light_sep);
    V.materials = up(P6.materials);
    s->view.tan_fov_y = V.tan_fov_y;
    s->flavor = RT_INTEGRATOR_HW6;
    make_walk_nodes(s.get(), V.cam_pos, V.nodes, n_nodes, V.fast_light_nodes, (uint32_t)P6.fast_light_nodes.size(), true,
                    V.grid, V.nodes4, V.fast_light_nodes4, up.bytes);
    report_trees(s.get(), desc, P6, V.n_lights, n_nodes, bvh_depth);
    return finish_scene(s, out, up.bytes, t0, t1);
}

// hw8 / hw7.  The host-side preparation (the replay of the reference's figure and light order: ~0.4 s for the benchmark scene) is
// optionally taken from `shared`: the first caller fills it, the others wait for it and only upload.
int create_hw8(const rt_scene_desc *desc, std::unique_ptr<rt_scene> &s, rt_scene **out, double t0, SharedPrep *shared) {
    if (desc->build_flags & ~RT_BUILD_DEVICE_BVH) return fail(RT_ERR_INVALID_ARG, "rt_scene_create: unknown build_flags");
    // Two things a scene tree is needed for.  The replay needs the reference's FIGURE ORDER (tie rule, light numbering) and, for the
    // rare hits at a box boundary, the reference's own tree (exact walks): the host replays the reference's builder for those
    // (prepare_scene) unless RT_BUILD_DEVICE_BVH gives the order up.  The walkers need a good tree of bounded depth, and a closest
    // hit does not depend on which: that one is built on the GPU (device/rt_bvh_build.h) over the records in figure order, each of
    // which carries its figure index (RTAMD_HOST_BVH=1, or a handful of triangles: the walkers use the reference topology).
    const bool fast_build = (desc->build_flags & RT_BUILD_DEVICE_BVH) && desc->n_triangles >= 64;
    const bool walk_tree_on_device = desc->n_triangles >= 64 && (fast_build || !env_flag("RTAMD_HOST_BVH"));
    PreparedScene P_local;
    if (shared) std::call_once(shared->once, [&] { try { prepare_scene(*desc, shared->P, fast_build); } catch (...) { shared->error = std::current_exception(); } });
    else prepare_scene(*desc, P_local, fast_build);
    if (shared && shared->error) std::rethrow_exception(shared->error);
    const PreparedScene &P = shared ? shared->P : P_local; // read-only from here on (several devices may be uploading from it)
    uint32_t bvh_depth = P.bvh_depth, n_nodes = (uint32_t)P.nodes.size();
    double t1 = now_ms();
    Uploader up{s.get()};
    SceneView &V = s->view;
    V.tri_isect = up(P.isect);
    V.tri_shade = up(P.shade);
    V.tri_box = up(P.tri_box);
    if (walk_tree_on_device) {
        const uint32_t n = desc->n_triangles;
        uint64_t scratch = 0;
        OwnedDev d_walk_box;
        if (!P.walk_box.empty()) d_walk_box.p = upload(P.walk_box, scratch); // reference leaf boxes (scene_prep.h)
        // The persistent kernel's walkers take two levels per step (GpuNode4Q) and hold up to three entries per step in a stack column
        // of P8_STACK entries; a walk that runs out of room is redone by the exact role with a stack of its own (rt_persistent.h).
        const DeviceTree t = build_leaf_ordered(s.get(), d_walk_box.p ? (const float *)d_walk_box.p : V.tri_box, V.tri_isect, n, P.box_pad, P8_STACK,
                                                11, true, V.tri_walk); // word 11 = TriIsect::pad: figure index << 1 | leaf mark
        V.nodes = t.nodes;
        up.bytes += (uint64_t)t.n_nodes * sizeof(GpuNode) + (uint64_t)n * sizeof(TriIsect);
        bvh_depth = t.depth;
        n_nodes = t.n_nodes;
        s->info.bvh_build_ms = t.build_ms; s->info.bvh_on_device = 1;
    } else {
        V.nodes = up(P.nodes);
        V.tri_walk = V.tri_isect;
    }
    if (P.bvh_depth > RT_STACK_SIZE - 2) // the exact walks keep a private stack over the reference's own tree
        return fail(RT_ERR_LIMIT, "the reference's scene BVH is deeper than the exact walk's stack (" + std::to_string(P.bvh_depth) + ")");
    if (bvh_depth > RT_STACK_SIZE - 2 || P.light_bvh_depth > RT_STACK_SIZE - 2)
        return fail(RT_ERR_LIMIT, "scene BVH deeper than the kernel's traversal stack (" + std::to_string(bvh_depth) + "/" +
                                      std::to_string(P.light_bvh_depth) + ")");
    V.light_nodes = up(P.light_nodes);
    V.light_sep = up(P.light_sep);
    upload_ref_trees(V, P, up);
    set_triangle_view(V, *desc, P, 2u);
    V.box_c2x *= (float)env_float("RTAMD_C2X_SCALE", 1.0); // experiment: the walkers' absolute look-behind (the gate's `seen` follows)
    V.exact_boxes = (env_flag("RTAMD_NO_EXACT_BOXES") || fast_build) ? 0u : 1u; // RT_BUILD_DEVICE_BVH: there is no reference tree to be exact about
    if (env_flag("RTAMD_DIAG_LOOKBEHIND_ONLY")) V.exact_boxes = 2u; // diagnostic (timing only, pixels NOT exact): the walkers look behind as with the gate, every hit stands
    V.n_tripwire_groups = (V.exact_boxes != 1u || env_flag("RTAMD_NO_TRIPWIRES")) ? 0u : P.n_tripwire_groups; // part of the exactness machinery
    V.tripwires = V.n_tripwire_groups ? up(P.tripwires) : nullptr;
    V.lights = up(P.lights);
    uint32_t n_light_walk_nodes = 0;
    {   // the light walker's own tree (rt_types.h: light_walk_nodes / lights_walk_test, lights_walk_rest)
        const uint32_t nl = (uint32_t)P.lights.size();
        const LightRec *ordered = nullptr;       // the records in the walker's leaf order
        std::vector<LightRec> tagged = P.lights; // pad = light index << 1 | last-of-leaf (of the REFERENCE topology for now)
        for (uint32_t i = 0; i < nl; i++) tagged[i].isect.pad = (i << 1) | (tagged[i].isect.pad ? 1u : 0u);
        if (nl >= 64 && !env_flag("RTAMD_HOST_LIGHT_BVH")) {
            uint64_t scratch = 0;
            OwnedDev d_tagged(upload(tagged, up.bytes)); // device_bytes: stands for the gathered copy of the same size, which the scene keeps
            OwnedDev d_lbox(upload(P.light_walk_box, scratch));
            const DeviceTree lt = build_leaf_ordered(s.get(), (const float *)d_lbox.p, (const LightRec *)d_tagged.p, nl, P.box_pad, 16, // the hits of a walk share its 24-entry column with the node stack
                                                     11, true, ordered);                                                        // word 11 = TriIsect::pad
            V.light_walk_nodes = lt.nodes;
            up.bytes += (uint64_t)lt.n_nodes * sizeof(GpuNode);
            s->light_walk_depth = lt.depth;
            n_light_walk_nodes = lt.n_nodes;
        } else {
            V.light_walk_nodes = V.light_nodes;
            n_light_walk_nodes = (uint32_t)P.light_nodes.size();
            ordered = up(tagged);
            s->light_walk_depth = P.light_bvh_depth;
        }
        // The walker reads the records as a pair of arrays (rt_types.h LightRest), which together are the bytes of the one: the leaf-ordered records
        // of either branch, the scene's newest allocation, make way for them.
        OwnedDev whole(s->allocations.back());
        s->allocations.pop_back();
        const size_t n_rec = nl ? nl : 1u; // (no lights: the one zeroed dummy record of the upload)
        char *pair = nullptr;
        HIP_CHECK(hipMalloc((void **)&pair, n_rec * sizeof(LightRec)));
        s->allocations.push_back(pair);
        char *rest = pair + n_rec * sizeof(TriIsect);
        HIP_CHECK(hipMemcpy2D(pair, sizeof(TriIsect), ordered, sizeof(LightRec), sizeof(TriIsect), n_rec, hipMemcpyDeviceToDevice));
        HIP_CHECK(hipMemcpy2D(rest, sizeof(LightRest), (const char *)ordered + sizeof(TriIsect), sizeof(LightRec), sizeof(LightRest), n_rec, hipMemcpyDeviceToDevice));
        V.lights_walk_test = (const TriIsect *)pair;
        V.lights_walk_rest = (const LightRest *)rest;
    }
    V.materials = up(P.materials);
    V.images = up(P.images);
    V.texels = up(P.texels);
    V.srgb_lut = up(std::vector<float>(P.srgb_lut, P.srgb_lut + 256));
    V.n_nodes = n_nodes;
    V.last_level_emission_only = 1;
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        const rt_material &m = desc->materials[i];
        if (!(m.metallic_factor >= 0 && m.metallic_factor <= 1 && m.base_color[0] >= 0 && m.base_color[1] >= 0 && m.base_color[2] >= 0))
            V.last_level_emission_only = 0;
    }
    if (env_flag("RTAMD_NO_LAST_LEVEL_SHORTCUT")) V.last_level_emission_only = 0;
    V.env_image = P.env_image;
    if (!walk_arrays_fit(desc->n_triangles, V.n_lights, n_nodes, n_light_walk_nodes)) // (a tree has no more wide nodes than two-box nodes)
        return fail(RT_ERR_LIMIT, "the scene's triangles, lights or tree nodes do not fit the walkers' 32-bit offsets (2^24 records, 4 GiB per array)");
    make_walk_nodes(s.get(), V.cam_pos, V.nodes, n_nodes, V.light_walk_nodes, n_light_walk_nodes, n_light_walk_nodes != 0,
                    V.grid, V.nodes4, V.light_walk_nodes4, up.bytes);
    report_trees(s.get(), desc, P, V.n_lights, n_nodes, bvh_depth);
    return finish_scene(s, out, up.bytes, t0, t1);
}

} // namespace

// rt_scene_create, with the host-side preparation of an hw8 / hw7 scene optionally shared (create_hw8): rt_multi_create gives all its
// devices the same one (rtamd_multi.hip); the plain C entry point passes none.
int rtamd::scene_create_shared(const rt_scene_desc *desc, rt_scene **out, rtamd::SharedPrep *shared) {
    if (!desc || !out) return fail(RT_ERR_INVALID_ARG, "rt_scene_create: null argument");
    if (desc->struct_size != sizeof(rt_scene_desc)) return fail(RT_ERR_INVALID_ARG, "rt_scene_create: struct_size mismatch (ABI skew)");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(RT_ERR_NO_DEVICE, "rt_scene_create: no HIP device available (this library has no CPU fallback)");
    return guarded("", [&]() -> int { // the preparation's refusals and HIP's failures name themselves
        std::unique_ptr<rt_scene> s(new rt_scene());
        HIP_CHECK(hipGetDevice(&s->device));
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, s->device));
        s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        const double t0 = now_ms();
        // (A scene without any figure counts as a .txt scene when its camera carries only CAMERA_FOV_X, as the .txt loader leaves it.)
        if (desc->n_triangles == 0 && (desc->n_primitives > 0 || (desc->camera.fov_x != 0.f && desc->camera.fov_y == 0.f))) return create_txt(desc, s, out, t0);
        // A scene without per-vertex normals can only be an hw6 scene.
        if (desc->n_triangles && !desc->normals) return create_hw6(desc, s, out, t0);
        return create_hw8(desc, s, out, t0, shared);
    });
}

extern "C" {

const char *rt_last_error(void) { return g_last_error.c_str(); }

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out) { return rtamd::scene_create_shared(desc, out, nullptr); }

void rt_scene_destroy(rt_scene *scene) { delete scene; }

int rt_scene_get_info(const rt_scene *scene, rt_scene_info *info) {
    if (!scene || !info) return fail(RT_ERR_INVALID_ARG, "rt_scene_get_info: null argument");
    *info = scene->info;
    return RT_OK;
}

int rt_scene_get_light_order(const rt_scene *scene, uint32_t *out, uint32_t capacity) {
    if (!scene || (!out && capacity)) return fail(RT_ERR_INVALID_ARG, "rt_scene_get_light_order: null argument");
    if (capacity < scene->light_order.size()) return fail(RT_ERR_INVALID_ARG, "rt_scene_get_light_order: buffer too small");
    memcpy(out, scene->light_order.data(), scene->light_order.size() * sizeof(uint32_t));
    return (int)scene->light_order.size();
}

int rt_host_prepare_orders(const rt_scene_desc *desc, int integrator, uint32_t *figure_order, uint32_t figure_capacity,
                           uint32_t *light_order, uint32_t light_capacity) {
    if (!desc || desc->struct_size != sizeof(rt_scene_desc)) return fail(RT_ERR_INVALID_ARG, "rt_host_prepare_orders: bad desc");
    return guarded("rt_host_prepare_orders: ", [&]() -> int {
        auto answer = [&](const PreparedTrees &P) -> int {
            if ((figure_order && figure_capacity < P.figure_order.size()) || (light_order && light_capacity < P.light_order.size())) return fail(RT_ERR_INVALID_ARG, "rt_host_prepare_orders: buffer too small");
            if (figure_order) memcpy(figure_order, P.figure_order.data(), P.figure_order.size() * sizeof(uint32_t));
            if (light_order) memcpy(light_order, P.light_order.data(), P.light_order.size() * sizeof(uint32_t));
            return (int)P.light_order.size();
        };
        if (integrator == RT_INTEGRATOR_HW8 || integrator == RT_INTEGRATOR_HW7) { PreparedScene P; prepare_scene(*desc, P); return answer(P); }
        if (integrator == RT_INTEGRATOR_HW6) { PreparedScene6 P; prepare_scene_hw6(*desc, P); return answer(P); }
        if (integrator == RT_INTEGRATOR_HW5) { PreparedScene5 P; prepare_scene_hw5(*desc, P); return answer(P); }
        return fail(RT_ERR_UNSUPPORTED, "rt_host_prepare_orders: integrator must be HW5, HW6, HW7 or HW8");
    });
}

int rt_unshard(const rt_render_params *p, const void *shard_buf, size_t elem_size, void *full_image) {
    if (!p || !shard_buf || !full_image || (elem_size != 1 && elem_size != 4)) return fail(RT_ERR_INVALID_ARG, "rt_unshard: bad argument");
    return guarded("rt_unshard: ", [&]() -> int {
    RenderView R{};
    std::string err;
    if (!resolve_tiles(p, R, err)) return fail(RT_ERR_INVALID_ARG, "rt_unshard: " + err);
    const uint8_t *src = (const uint8_t *)shard_buf;
    uint8_t *dst = (uint8_t *)full_image;
    size_t px = 3 * elem_size;
    if (R.shard_count <= 1) { memcpy(dst, src, (size_t)R.width * R.height * px); return RT_OK; }
    for (uint32_t st = 0; st < R.n_shard_tiles; st++) {
        int tx0, ty0, w, h;
        shard_tile_rect(R, st, tx0, ty0, w, h);
        for (int ly = 0; ly < h; ly++)
            memcpy(dst + ((size_t)(ty0 + ly) * R.width + tx0) * px, src + (((size_t)st * R.tile_h + ly) * R.tile_w) * px, (size_t)w * px);
    }
    return RT_OK;
    });
}

// ---- host-side front-end ---------------------------------------------------------------------------
int rt_load_gltf(const char *path, int flavor, rt_host_scene **out) {
    if (!path || !out) return fail(RT_ERR_INVALID_ARG, "rt_load_gltf: null argument");
    *out = nullptr;
    return guarded(std::string("rt_load_gltf(") + path + "): ", [&]() -> int { *out = load_gltf(path, flavor); return RT_OK; }, RT_ERR_PARSE);
}
int rt_load_txt(const char *path, int flavor, rt_host_scene **out, int32_t *w, int32_t *h, int32_t *samples, int32_t *depth) {
    if (!path || !out) return fail(RT_ERR_INVALID_ARG, "rt_load_txt: null argument");
    *out = nullptr;
    return guarded(std::string("rt_load_txt(") + path + "): ", [&]() -> int { *out = load_txt(path, flavor, w, h, samples, depth); return RT_OK; }, RT_ERR_PARSE);
}
int rt_host_scene_set_environment(rt_host_scene *hs, const char *image_path) {
    if (!hs || !image_path) return fail(RT_ERR_INVALID_ARG, "rt_host_scene_set_environment: null argument");
    return guarded("", [&]() -> int {
        int w, h;
        load_image_rgb8(image_path, w, h, hs->env_data);
        hs->env = rt_image{w, h, nullptr};
        hs->has_env = true;
        hs->finalize();
        return RT_OK;
    }, RT_ERR_IO);
}
const rt_scene_desc *rt_host_scene_desc(const rt_host_scene *hs) { return hs ? &hs->desc : nullptr; }
void rt_host_scene_free(rt_host_scene *hs) { delete hs; }

int rt_write_ppm(const char *path, int32_t width, int32_t height, const uint8_t *rgb8) { // sceneio.cpp:383-385,397-401
    if (!path || !rgb8 || width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARG, "rt_write_ppm: bad argument");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(RT_ERR_IO, std::string("rt_write_ppm: cannot open ") + path);
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    size_t n = (size_t)width * height * 3;
    bool ok = fwrite(rgb8, 1, n, f) == n;
    ok = (fclose(f) == 0) && ok;
    return ok ? RT_OK : fail(RT_ERR_IO, std::string("rt_write_ppm: short write to ") + path);
}
int rt_decode_png(const char *path, int32_t *width, int32_t *height, uint8_t **rgb) {
    if (!path || !width || !height || !rgb) return fail(RT_ERR_INVALID_ARG, "rt_decode_png: null argument");
    return guarded("", [&]() -> int {
        std::vector<uint8_t> px;
        int w, h;
        load_image_rgb8(path, w, h, px);
        *rgb = (uint8_t *)malloc(px.size());
        if (!*rgb) return fail(RT_ERR_IO, "rt_decode_png: out of memory");
        memcpy(*rgb, px.data(), px.size());
        *width = w; *height = h;
        return RT_OK;
    }, RT_ERR_IO);
}
void rt_free(void *p) { free(p); }

} // extern "C"

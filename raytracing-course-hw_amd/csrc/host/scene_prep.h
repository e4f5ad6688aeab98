// What every device array of a scene holds (scene_prep.cpp decides it, without HIP; rtamd_scene.hip uploads it).
#pragma once
#include "../../../include/rtamd.h"
#include "../device/rt_types.h"
#include "../device/rt_types_hw6.h"
#include "../device/rt_types_hw5.h"
#include "../device/rt_types_txt.h"
#include <cstdint>
#include <vector>

namespace rtamd {

// What the three flavours with a BVH have in common: the scene tree and the light tree, each as padded two-box nodes for the culling
// walks and as the reference's own tree with its unpadded boxes for the reference-exact walks, the two orders and the two depths.
struct PreparedTrees {
    std::vector<GpuNode> nodes, light_nodes;
    std::vector<GpuRefNode> ref_nodes, ref_light_nodes;
    std::vector<uint32_t> figure_order; // BVH order -> LOAD index
    std::vector<uint32_t> light_order;  // light order -> LOAD index
    uint32_t bvh_depth = 0, light_bvh_depth = 0;
};

// ... and the two flavours of triangles (hw8 / hw7 and hw6):
struct PreparedTriangles : PreparedTrees {
    // Every figure's own box (reference figure order, 8 floats each), read with the reference's trees by the reference-exact walks of
    // the persistent pipelines (device/rt_persistent.h); box_c2 = 2^-20 * the largest |coordinate| of scene and camera.
    std::vector<float> tri_box;
    float box_c2 = 0.f;
    float box_pad = 0.f;   // absolute part of the walkers' box padding (scene_prep.cpp pad_box): 2^-18 x the largest |coordinate|
    // Order of the light-pdf additions without walking the reference tree: light_sep[j * n_lights + i] = the shallowest
    // separation depth among the boundaries i .. i + 2^j - 1 (boundary b lies between lights b and b+1 of the reference order;
    // its depth is that of the reference-tree node whose children hold the two lights, or, inside one leaf, a pseudo depth
    // that grows towards the leaf's first light).  A range minimum over it gives the depth at which two hit lights separate.
    std::vector<uint16_t> light_sep;
    uint32_t light_sep_levels = 0;
};

struct PreparedScene : PreparedTriangles {
    // Per figure the box of its LEAF in the reference's tree (a few leaves hold several triangles): what the GPU builder makes the
    // walkers' tree from, so that whatever the reference can reach through its leaf box is inside a box of ours.  Empty when the
    // reference's tree is not replayed.
    std::vector<float> walk_box;
    // The same for the lights (light order): the box of each light's leaf in the reference's light tree.  The persistent kernel's light
    // walker uses a tree of its own over these (built on the GPU): the reference's light tree also holds the far-apart ceiling quads and
    // the lamp near its root, so its upper boxes span the room and most rays descend into them in vain.
    std::vector<float> light_walk_box;
    // Tripwires (device/rt_exact.h pt_tripwire): the reference's triangle test solves the hit's barycentrics in a fixed projection
    // (primitives.cpp:85-104); for a triangle whose plane (nearly) contains that projection's kernel direction the system is (nearly)
    // singular and the test accepts points anywhere on the plane — a "hit" metres away from the triangle, which the reference finds or not
    // depending on whether its walk enters the triangle's leaf box before a closer hit prunes it.  No culling walk can know that, so a ray
    // that pierces the leaf box of such a triangle anywhere AND passes that triangle's test (the reference would test it if its walk got there) goes
    // to the exact walk at once.  Layout: n_tripwire_groups records of two
    // float4 {lo.xyz, first member | hi.xyz, member count} (indices as raw bits), then the members' boxes {lo.xyz, figure index | hi.xyz, -}; empty when
    // the reference's tree is not replayed.
    std::vector<float> tripwires;
    uint32_t n_tripwire_groups = 0;
    std::vector<TriIsect> isect;
    std::vector<TriShade> shade;
    std::vector<LightRec> lights;
    std::vector<GpuMaterial> materials;
    std::vector<GpuImage> images;
    std::vector<uint8_t> texels;
    float srgb_lut[256];
    int32_t env_image = -1;
};

// Throws std::runtime_error on invalid input.
// tree_on_device (rt_scene_desc.build_flags & RT_BUILD_DEVICE_BVH): the reference's scene-tree build is not replayed; figure order =
// LOAD order, `nodes` stays empty, `isect` / `shade` / `tri_box` stay in LOAD order without leaf marks, for device/rt_bvh_build.h.
void prepare_scene(const rt_scene_desc &desc, PreparedScene &out, bool tree_on_device = false);

// hw6 flavour (flat-shaded triangles, hw6/src/scene.cpp): own scene tree (`nodes`, bvh_depth) + reference-topology light tree;
// ref_nodes / ref_light_nodes are the reference's own trees, figure_order / light_order its orders.
struct PreparedScene6 : PreparedTriangles {
    std::vector<GpuNode> fast_light_nodes;
    std::vector<Tri6> tris, lights, fast_lights;
    uint32_t fast_light_bvh_depth = 0;
    std::vector<uint32_t> light_ref; // 4 words per reference light-tree node: left, right, first, last
    std::vector<Tri6> ref_tris;      // figure records in the reference's figure order (ref_index = position)
    std::vector<float> boxes8;       // tree_on_device only: per triangle (LOAD order) the box of its reference leaf
    std::vector<GpuMaterial6> materials;
};
// tree_on_device: skip the own scene tree; `tris` stay in LOAD order (ref_index set, no leaf marks) and `boxes8` (lo.xyz, -, hi.xyz, -
// per triangle) is filled for device/rt_bvh_build.h.
void prepare_scene_hw6(const rt_scene_desc &desc, PreparedScene6 &out, bool tree_on_device = false);

// hw5 flavour (.txt scene with TRIANGLE figures): the reference's figure order, BVH and light list / light BVH
// (hw5/src/scene.cpp:8-23, hw5/src/include/distributions.h:180-198), both trees in the reference's topology; the hw5 kernel walks
// the ref_* trees (reference-exact box decisions).
struct PreparedScene5 : PreparedTrees {
    std::vector<GpuFig5> figs, lights;
    uint32_t n_nonplanes = 0;
};
void prepare_scene_hw5(const rt_scene_desc &desc, PreparedScene5 &out);

// What hw1 .. hw4 read of a .txt scene: the primitives and the hw2 lights in LOAD order, and hw4's list of emissive BOX / ELLIPSOID
// primitives (hw4/src/scene.cpp:12-21).  Its two refusals carry rt_scene_create's name: no other entry point prepares these.
struct PreparedSceneTxt {
    std::vector<GpuPrim> prims;
    std::vector<GpuLight> lights;
    std::vector<uint32_t> light_prims;
    bool has_triangles = false; // TRIANGLE figures: the hw5 grammar only
};
void prepare_scene_txt(const rt_scene_desc &desc, PreparedSceneTxt &out);

// Two steps of the preparation on their own, for the test hooks: the intersection record of one triangle (data, data2, data3 as nine
// floats; make_isect) and a box as the walkers' two-box nodes hold it (pad_box with scene_abs_pad of the scene's largest |coordinate|).
// Also the records of one .txt figure as prepare_scene_txt and prepare_scene_hw5 pack them (material and leaf mark aside).
TriIsect isect_of_positions(const float *positions9);
GpuPrim pack_prim(const rt_primitive &p);
GpuFig5 pack_fig5(const rt_primitive &p);
void walk_box_of(const float lo[3], const float hi[3], float max_coord, float out_lo[3], float out_hi[3]);

} // namespace rtamd

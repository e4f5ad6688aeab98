// The four host-side preparations (csrc/host/scene_prep.cpp) under a host sanitizer, stand-alone: a soup beyond the 16,384-triangle
// fork of the threaded tree build and a .txt scene, both made in memory.  From the repository root:
//   hipcc -x c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/diagnostics/prep_sanitize.cpp raytracing-course-hw_amd/csrc/host/scene_prep.cpp -lpthread -o /tmp/prep_asan && /tmp/prep_asan
// and once more with -fsanitize=thread for the threads of the subtree build.  Prints one line per preparation; no GPU, no Python.
#include "../../raytracing-course-hw_amd/csrc/host/scene_prep.h"
#include <cstdio>

int main() {
    const uint32_t n = 40000;
    uint32_t x = 12345u;
    auto rnd = [&] { x = x * 1664525u + 1013904223u; return (float)(x >> 8) * (1.f / 16777216.f); };
    std::vector<float> pos(9 * (size_t)n), nrm(9 * (size_t)n);
    std::vector<uint32_t> mat(n);
    for (uint32_t i = 0; i < n; i++) {
        const float c[3] = {4 * rnd() - 2, 4 * rnd() - 2, 4 * rnd() - 2};
        for (int k = 0; k < 9; k++) { pos[9 * (size_t)i + k] = c[k % 3] + 0.7f * rnd() - 0.35f; nrm[9 * (size_t)i + k] = rnd(); }
        mat[i] = x % 3u;
    }
    for (int k = 0; k < 9 * 20; k++) pos[9 * (size_t)(n / 2) + k] = pos[k]; // exact duplicates: ties
    rt_material mats[3] = {};
    for (rt_material &m : mats) m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = m.normal_texture = -1;
    mats[0].emission[1] = 2.f;
    rt_scene_desc d = {};
    d.struct_size = sizeof d;
    d.n_triangles = n; d.positions = pos.data(); d.normals = nrm.data(); d.material_index = mat.data();
    d.n_materials = 3; d.materials = mats;
    d.camera.position[2] = 6.f;
    for (int on_device = 0; on_device < 2; on_device++) {
        rtamd::PreparedScene P8;
        rtamd::prepare_scene(d, P8, on_device != 0);
        printf("hw8 tree_on_device=%d: %zu nodes, %zu lights, %u tripwire groups\n", on_device, P8.nodes.size(), P8.lights.size(), P8.n_tripwire_groups);
        rtamd::PreparedScene6 P6;
        rtamd::prepare_scene_hw6(d, P6, on_device != 0);
        printf("hw6 tree_on_device=%d: %zu nodes, %zu lights, %zu reference nodes\n", on_device, P6.nodes.size(), P6.lights.size(), P6.ref_nodes.size());
    }
    rt_primitive prims[5] = {};
    const int types[5] = {RT_PRIM_PLANE, RT_PRIM_BOX, RT_PRIM_ELLIPSOID, RT_PRIM_TRIANGLE, RT_PRIM_BOX};
    for (int i = 0; i < 5; i++) {
        prims[i].type = types[i];
        for (int k = 0; k < 3; k++) { prims[i].data[k] = 0.5f + rnd(); prims[i].data2[k] = rnd(); prims[i].data3[k] = rnd(); prims[i].position[k] = 3 * rnd(); }
        prims[i].rotation[3] = 1.f;
        prims[i].emission[0] = i & 1 ? 1.f : 0.f;
    }
    rt_light light = {};
    light.type = RT_LIGHT_POINT;
    rt_scene_desc t = {};
    t.struct_size = sizeof t;
    t.n_primitives = 5; t.primitives = prims; t.n_lights = 1; t.lights = &light;
    rtamd::PreparedScene5 P5;
    rtamd::prepare_scene_hw5(t, P5);
    rtamd::PreparedSceneTxt PT;
    rtamd::prepare_scene_txt(t, PT);
    printf("hw5: %zu figures, %zu lights; txt: %zu primitives, %zu lights, %zu light primitives\n", P5.figs.size(), P5.lights.size(), PT.prims.size(), PT.lights.size(), PT.light_prims.size());
    return 0;
}

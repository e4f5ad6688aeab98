// POD layouts of the .txt scenes' paths (hw1 .. hw4: a flat list of analytic primitives) shared by scene creation and kernels.
#pragma once
#include <stdint.h>

namespace rtamd {

struct GpuPrim {              // 80 bytes
    float data[3]; int32_t type;
    float position[3]; int32_t kind;
    float rotation[4];
    float color[3]; float ior;
    float emission[3]; float pad;
};
static_assert(sizeof(GpuPrim) == 80, "GpuPrim must be 80 bytes");

struct GpuLight {             // 64 bytes, hw2 only
    float intensity[3]; int32_t type;
    float position[3]; float pad0;
    float attenuation[3]; float pad1;
    float direction[3]; float pad2;
};
static_assert(sizeof(GpuLight) == 64, "GpuLight must be 64 bytes");

struct SceneViewTxt {
    const GpuPrim *prims;
    uint32_t n_prims;
    float cam_pos[3], cam_right[3], cam_up[3], cam_fwd[3];
    float bg[3];
    float tan_fov_x;          // (float)tan((double)(fovX / 2)), hw3/src/scene.cpp:100
    float tan_fov_x_f;        // tanf(fovX / 2): hw1/hw2 compile against <math.h>, where tan(float) is the float overload
    const GpuLight *lights;   // hw2
    uint32_t n_lights;
    float ambient[3];         // hw2 AMBIENT_LIGHT
    const uint32_t *light_prims; // hw4: emissive BOX / ELLIPSOID primitives in figure order (hw4/src/scene.cpp:12-21)
    uint32_t n_light_prims;
};

} // namespace rtamd

// The cameras of a view set (include/rtamd.h: rt_views_create, rt_views_set_cameras, and the same two of rt_view_adaptive_*): the check
// and the record the kernel reads.  Host functions with no GPU call in them, shared by rtamd_views.hip, rtamd_view_adaptive.hip and the
// test hook rtt_views_camera_check (test_hooks.hip).
#pragma once
#include <cmath>
#include <string>
#include "../../../include/rtamd.h"
#include "../device/rt_types.h" // ViewCamera

namespace rtamd {

#define VIEWS_CAMERA_MAX 1099511627776.0f // 2^40: with it no float expression of the camera ray overflows at a frame of 65,535 pixels a side
#define VIEWS_FOV_Y_MAX 3.0f
#define VIEWS_MIN_DET 1e-6                // |det(right, up, forward)| over the product of the three lengths; an orthonormal basis has 1

// Empty when the camera is usable, else the field and what is wrong with it.  fov_x is not looked at.
inline std::string views_camera_check(const rt_camera &c) {
    const struct { const char *name; const float *v; } fields[4] = {{"position", c.position}, {"right", c.right}, {"up", c.up}, {"forward", c.forward}};
    for (const auto &f : fields)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(f.v[k]) || std::fabs(f.v[k]) > VIEWS_CAMERA_MAX)
                return std::string(f.name) + "[" + std::to_string(k) + "] must be finite and at most 2^40 in magnitude";
    if (!(c.fov_y > 0.f && c.fov_y <= VIEWS_FOV_Y_MAX)) return "fov_y must lie in (0, 3] radians";
    const double r[3] = {c.right[0], c.right[1], c.right[2]}, u[3] = {c.up[0], c.up[1], c.up[2]}, f[3] = {c.forward[0], c.forward[1], c.forward[2]};
    const double det = r[0] * (u[1] * f[2] - u[2] * f[1]) - r[1] * (u[0] * f[2] - u[2] * f[0]) + r[2] * (u[0] * f[1] - u[1] * f[0]);
    const double len = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) *
                       std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(std::fabs(det) > VIEWS_MIN_DET * len)) return "right, up and forward must be linearly independent (their determinant is 0 against their lengths)";
    return std::string();
}

// The refusal of a camera array, before anything is touched; `first`: the view of cameras[0].  Empty when every camera is usable.
inline std::string views_cameras_check(const rt_camera *cameras, int32_t first, int32_t n) {
    for (int32_t i = 0; i < n; i++) {
        const std::string why = views_camera_check(cameras[i]);
        if (!why.empty()) return "cameras: view " + std::to_string(first + i) + ": " + why;
    }
    return std::string();
}

// The record the kernel reads: the camera's vectors as given, the two tangents by the expressions of the scene's own camera
// (set_triangle_view: host libm in double; frame_tan_fov_x).
inline ViewCamera views_camera_record(const rt_camera &c, int32_t width, int32_t height) {
    ViewCamera r{};
    for (int k = 0; k < 3; k++) { r.pos[k] = c.position[k]; r.right[k] = c.right[k]; r.up[k] = c.up[k]; r.fwd[k] = c.forward[k]; }
    r.tan_fov_y = (float)std::tan((double)(c.fov_y / 2)); // scene.cpp:180
    r.tan_fov_x = r.tan_fov_y * width / height;           // scene.cpp:181
    return r;
}

} // namespace rtamd

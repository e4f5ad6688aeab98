"""ctypes binding of librtamd.so — the C-ABI in include/rtamd.h.

This Python layer is plumbing for tests and bench.py only: it marshals numpy arrays into
``rt_scene_desc`` and calls the library.  There is no Python or CPU implementation of the render
path here; if the HIP extension has not been built the import fails loudly.

The package directory name contains a hyphen, so import it with
``importlib.import_module("raytracing-course-hw_amd")``.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTAMD_LIB") or os.path.join(_HERE, "librtamd.so")  # RTAMD_LIB: an experimental build of the same library (tools/tuning)

RT_INTEGRATOR_HW1, RT_INTEGRATOR_HW2, RT_INTEGRATOR_HW3, RT_INTEGRATOR_HW4, RT_INTEGRATOR_HW5 = 1, 2, 3, 4, 5
RT_INTEGRATOR_HW6, RT_INTEGRATOR_HW7, RT_INTEGRATOR_HW8 = 6, 7, 8
RT_FLAG_OUT_DEVICE, RT_FLAG_COUNTERS, RT_FLAG_SAMPLE_SEEDS, RT_FLAG_RUSSIAN_ROULETTE = 1, 2, 4, 8
RT_BUILD_DEVICE_BVH = 1
RT_QUERY_DEVICE_POINTERS, RT_QUERY_REFERENCE_WALK = 1, 2
RT_HIT_INSIDE, RT_HIT_EXACT_WALK, RT_HIT_INVALID_RAY = 1, 2, 4
RT_HIT_MISS = 0xFFFFFFFF
RT_OCCLUSION_OCCLUDED, RT_OCCLUSION_EXACT_WALK, RT_OCCLUSION_INVALID_RAY = 1, 2, 4
RT_SCATTER_END_BRDF, RT_SCATTER_END_CLAMP, RT_SCATTER_NO_SURFACE, RT_SCATTER_INVALID = 1, 2, 4, 8
RT_DENOISE_DEVICE_POINTERS, RT_DENOISE_ALBEDO = 1, 2
RT_ADAPTIVE_DILATE = 1
RT_ADAPTIVE_ACTIVE, RT_ADAPTIVE_CONVERGED, RT_ADAPTIVE_CAPPED, RT_ADAPTIVE_NO_ESTIMATE = 1, 2, 4, 8
RT_PIPELINE_SINGLE, RT_PIPELINE_ROUNDS, RT_PIPELINE_PERSISTENT = 0, 1, 2
RT_OK = 0
RT_ERR_INVALID_ARG, RT_ERR_NO_DEVICE, RT_ERR_HIP, RT_ERR_UNSUPPORTED, RT_ERR_LIMIT = -1, -2, -3, -4, -7


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rtamd error {code}: {msg}")
        self.code = code


class rt_material(C.Structure):
    _fields_ = [("base_color", C.c_float * 3), ("emission", C.c_float * 3), ("metallic_factor", C.c_float),
                ("roughness_factor", C.c_float), ("base_color_texture", C.c_int32), ("emissive_texture", C.c_int32),
                ("metallic_roughness_texture", C.c_int32), ("normal_texture", C.c_int32), ("kind", C.c_int32),
                ("ior", C.c_float)]


class rt_image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_uint8))]


class rt_primitive(C.Structure):
    _fields_ = [("type", C.c_int32), ("data", C.c_float * 3), ("position", C.c_float * 3), ("rotation", C.c_float * 4),
                ("color", C.c_float * 3), ("emission", C.c_float * 3), ("kind", C.c_int32), ("ior", C.c_float),
                ("data2", C.c_float * 3), ("data3", C.c_float * 3)]


class rt_light(C.Structure):
    _fields_ = [("type", C.c_int32), ("intensity", C.c_float * 3), ("position", C.c_float * 3),
                ("attenuation", C.c_float * 3), ("direction", C.c_float * 3)]


class rt_camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3),
                ("fov_y", C.c_float), ("fov_x", C.c_float)]


class rt_scene_desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_triangles", C.c_uint32),
                ("positions", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("normals", C.POINTER(C.c_float)), ("tangents", C.POINTER(C.c_float)),
                ("material_index", C.POINTER(C.c_uint32)),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(rt_material)),
                ("n_textures", C.c_uint32), ("texture_source", C.POINTER(C.c_uint32)),
                ("n_images", C.c_uint32), ("images", C.POINTER(rt_image)),
                ("environment_map", C.POINTER(rt_image)),
                ("n_primitives", C.c_uint32), ("primitives", C.POINTER(rt_primitive)),
                ("camera", rt_camera), ("bg_color", C.c_float * 3),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(rt_light)), ("ambient_light", C.c_float * 3),
                ("build_flags", C.c_uint32), ("reserved", C.c_uint32)]


class rt_render_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32),
                ("ray_depth", C.c_int32), ("integrator", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("flags", C.c_uint32), ("stream", C.c_void_p),
                ("sample_streams", C.c_int32), ("reserved", C.c_int32)]


class rt_stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("samples", C.c_uint64),
                ("closest_hit_queries", C.c_uint64), ("light_pdf_queries", C.c_uint64), ("node_visits", C.c_uint64),
                ("triangle_tests", C.c_uint64), ("launches", C.c_uint32), ("dominant_kernel_launches", C.c_uint32),
                ("dominant_kernel_ms", C.c_double), ("pipeline", C.c_uint32), ("reference_exact", C.c_uint32),
                ("exact_closest_hits", C.c_uint64), ("exact_light_sums", C.c_uint64)]


class rt_scene_info(C.Structure):
    _fields_ = [("n_triangles", C.c_uint32), ("n_lights", C.c_uint32), ("n_bvh_nodes", C.c_uint32),
                ("n_light_bvh_nodes", C.c_uint32), ("bvh_depth", C.c_uint32), ("light_bvh_depth", C.c_uint32),
                ("device_bytes", C.c_uint64), ("prep_ms", C.c_double), ("upload_ms", C.c_double),
                ("bvh_build_ms", C.c_double), ("bvh_on_device", C.c_uint32), ("reserved", C.c_uint32)]


class rt_noise_summary(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("batches", C.c_int32), ("samples_observed", C.c_int32), ("samples_total", C.c_int32),
                ("pixels", C.c_uint64), ("nonfinite_pixels", C.c_uint64), ("mean_luminance", C.c_double), ("rms_error", C.c_double),
                ("noise", C.c_double), ("worst_tile_noise", C.c_double)]


class rt_ray(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("d", C.c_float * 3)]


class rt_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("triangle", C.c_uint32), ("ng", C.c_float * 3), ("texcoord", C.c_float * 2), ("ns", C.c_float * 3),
                ("tangent", C.c_float * 4), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class rt_query_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reference_exact", C.c_uint32), ("rays", C.c_uint64), ("exact_walks", C.c_uint64),
                ("invalid_rays", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("launches", C.c_uint32),
                ("reserved", C.c_uint32)]


class rt_rng(C.Structure):
    _fields_ = [("x", C.c_uint32), ("saved", C.c_float), ("has_saved", C.c_uint32), ("reserved", C.c_uint32)]


class rt_scatter(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("pdf", C.c_float), ("d", C.c_float * 3), ("flags", C.c_uint32), ("weight", C.c_float * 3),
                ("component", C.c_uint32), ("brdf", C.c_float * 3), ("reserved", C.c_uint32)]


class rt_bake_point(C.Structure):
    _fields_ = [("p", C.c_float * 3), ("n", C.c_float * 3)]


class rt_bake_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("samples", C.c_int32), ("streams", C.c_int32), ("ray_depth", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class rt_bake_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reference_exact", C.c_uint32), ("points", C.c_uint64), ("invalid_points", C.c_uint64),
                ("paths", C.c_uint64), ("exact_walks", C.c_uint64), ("rounds", C.c_uint64), ("ray_slots", C.c_uint64),
                ("live_ray_slots", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("launches", C.c_uint32),
                ("reserved", C.c_uint32)]


class rt_denoise_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("sigma_depth", C.c_float), ("sigma_luminance", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class rt_denoise_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_uint32), ("fixed_pixels", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double)]


class rt_adaptive_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("target_noise", C.c_float), ("min_batches", C.c_int32), ("max_samples", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_int32)]


class rt_adaptive_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("active_tiles", C.c_uint32), ("converged_tiles", C.c_uint32), ("capped_tiles", C.c_uint32),
                ("samples", C.c_uint64), ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("kernel_ms", C.c_double),
                ("gather_ms", C.c_double), ("scatter_ms", C.c_double), ("total_ms", C.c_double), ("launches", C.c_uint32),
                ("reference_exact", C.c_uint32), ("exact_walks", C.c_uint64)]


class rt_views_params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("ray_depth", C.c_int32), ("n_views", C.c_int32),
                ("flags", C.c_uint32), ("stream", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class rt_views_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("active_views", C.c_uint32), ("samples", C.c_uint64), ("min_samples", C.c_int32),
                ("max_samples", C.c_int32), ("kernel_ms", C.c_double), ("gather_ms", C.c_double), ("scatter_ms", C.c_double),
                ("total_ms", C.c_double), ("launches", C.c_uint32), ("reference_exact", C.c_uint32), ("exact_walks", C.c_uint64)]


class rt_view_adaptive_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("active_views", C.c_uint32), ("active_tiles", C.c_uint32), ("converged_tiles", C.c_uint32),
                ("capped_tiles", C.c_uint32), ("launches", C.c_uint32), ("samples", C.c_uint64), ("min_samples", C.c_int32),
                ("max_samples", C.c_int32), ("kernel_ms", C.c_double), ("gather_ms", C.c_double), ("scatter_ms", C.c_double),
                ("noise_ms", C.c_double), ("total_ms", C.c_double), ("reference_exact", C.c_uint32), ("reserved", C.c_uint32),
                ("exact_walks", C.c_uint64)]


# rt_adaptive_tile as a numpy record: what AdaptiveRender.tiles() returns, one per 8x8 sub-tile
ADAPTIVE_TILE_DTYPE = np.dtype([("samples", np.int32), ("batches", np.int32), ("pixels", np.uint32), ("nonfinite", np.uint32),
                                ("sum_se2", np.float32), ("sum_luminance", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])

# rt_ray / rt_hit as numpy records: what Scene.query_* take and return
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3)])
HIT_DTYPE = np.dtype([("t", np.float32), ("triangle", np.uint32), ("ng", np.float32, 3), ("texcoord", np.float32, 2), ("ns", np.float32, 3),
                      ("tangent", np.float32, 4), ("flags", np.uint32), ("reserved", np.uint32)])
SURFACE_DTYPE = np.dtype([("color", np.float32, 3), ("alpha", np.float32), ("emission", np.float32, 3), ("metallic", np.float32),
                          ("sn", np.float32, 3), ("material", np.uint32), ("base_color", np.float32, 3), ("base_metallic", np.float32)])
RNG_DTYPE = np.dtype([("x", np.uint32), ("saved", np.float32), ("has_saved", np.uint32), ("reserved", np.uint32)])
SCATTER_DTYPE = np.dtype([("o", np.float32, 3), ("pdf", np.float32), ("d", np.float32, 3), ("flags", np.uint32), ("weight", np.float32, 3),
                          ("component", np.uint32), ("brdf", np.float32, 3), ("reserved", np.uint32)])
BAKE_POINT_DTYPE = np.dtype([("p", np.float32, 3), ("n", np.float32, 3)])
RT_BAKE_IRRADIANCE, RT_BAKE_SH9 = 0, 1
RT_BAKE_LOCKSTEP = 4
BAKE_FLOATS = {RT_BAKE_IRRADIANCE: 3, RT_BAKE_SH9: 27}

# Every symbol include/rtamd.h declares; tests/test_abi.py checks the library exports them all.
ABI_SYMBOLS = ["rt_abi_version", "rt_last_error", "rt_scene_create", "rt_scene_destroy", "rt_output_elems", "rt_render",
               "rt_unshard", "rt_scene_get_info", "rt_scene_get_light_order", "rt_load_gltf", "rt_load_txt",
               "rt_host_scene_set_environment", "rt_host_scene_desc", "rt_host_scene_free", "rt_write_ppm",
               "rt_decode_png", "rt_free", "rt_host_prepare_orders", "rt_device_count", "rt_multi_create", "rt_multi_render",
               "rt_multi_destroy", "rt_accum_create", "rt_accum_render", "rt_accum_samples", "rt_accum_resolve",
               "rt_accum_state_bytes", "rt_accum_save", "rt_accum_load", "rt_accum_destroy", "rt_multi_accum_create",
               "rt_multi_accum_render", "rt_multi_accum_samples", "rt_multi_accum_resolve", "rt_multi_accum_save",
               "rt_multi_accum_load", "rt_multi_accum_destroy", "rt_noise_create", "rt_noise_update", "rt_noise_reset",
               "rt_noise_batches", "rt_noise_estimate", "rt_noise_destroy", "rt_multi_noise_create", "rt_multi_noise_update",
               "rt_multi_noise_reset", "rt_multi_noise_batches", "rt_multi_noise_estimate", "rt_multi_noise_destroy", "rt_query_closest",
               "rt_query_light_pdf", "rt_query_surface", "rt_query_environment", "rt_camera_rays", "rt_render_guides",
               "rt_query_occluded", "rt_rng_seed", "rt_query_scatter", "rt_query_bsdf", "rt_trace_paths", "rt_bake_rays", "rt_bake",
               "rt_render_paths", "rt_render_bake", "rt_render_probes", "rt_adaptive_create", "rt_adaptive_render",
               "rt_adaptive_render_tiles", "rt_adaptive_tiles", "rt_adaptive_resolve", "rt_adaptive_noise", "rt_adaptive_sample_map",
               "rt_adaptive_destroy", "rt_views_create", "rt_views_set_cameras", "rt_views_render", "rt_views_samples", "rt_views_resolve",
               "rt_views_destroy", "rt_view_adaptive_create", "rt_view_adaptive_set_cameras", "rt_view_adaptive_render",
               "rt_view_adaptive_render_tiles", "rt_view_adaptive_tiles", "rt_view_adaptive_resolve", "rt_view_adaptive_noise",
               "rt_view_adaptive_sample_map", "rt_view_adaptive_destroy"]
# The preview filter's two, which the header declares `extern int`: the list above and the family lists of the tests are closed sets
# of the header's plain prototypes (tests/test_abi_and_host.py, tests/test_accum_host.py), and rt_accum_denoise is no rt_accum_* of theirs.
DENOISE_SYMBOLS = ["rt_denoise", "rt_accum_denoise"]
# Likewise the one function of the header that returns a float (`extern float`): the closed set above is of its int / void / pointer prototypes.
RNG_SYMBOLS = ["rt_rng_uniform"]

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no fallback implementation")
lib = C.CDLL(LIB_PATH)
lib.rt_last_error.restype = C.c_char_p
lib.rt_scene_create.argtypes = [C.POINTER(rt_scene_desc), C.POINTER(C.c_void_p)]
lib.rt_scene_destroy.argtypes = [C.c_void_p]
lib.rt_scene_destroy.restype = None
lib.rt_output_elems.argtypes = [C.POINTER(rt_render_params)]
lib.rt_output_elems.restype = C.c_size_t
lib.rt_render.argtypes = [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]
lib.rt_unshard.argtypes = [C.POINTER(rt_render_params), C.c_void_p, C.c_size_t, C.c_void_p]
lib.rt_scene_get_info.argtypes = [C.c_void_p, C.POINTER(rt_scene_info)]
lib.rt_scene_get_light_order.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
lib.rt_host_prepare_orders.argtypes = [C.POINTER(rt_scene_desc), C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
lib.rt_load_gltf.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
lib.rt_load_txt.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)] + [C.POINTER(C.c_int32)] * 4
lib.rt_host_scene_set_environment.argtypes = [C.c_void_p, C.c_char_p]
lib.rt_host_scene_desc.argtypes = [C.c_void_p]
lib.rt_host_scene_desc.restype = C.POINTER(rt_scene_desc)
lib.rt_host_scene_free.argtypes = [C.c_void_p]
lib.rt_host_scene_free.restype = None
lib.rt_write_ppm.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
lib.rt_decode_png.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_uint8))]
lib.rt_free.argtypes = [C.c_void_p]
lib.rt_free.restype = None
lib.rt_multi_create.argtypes = [C.POINTER(rt_scene_desc), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
lib.rt_multi_render.argtypes = [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]
lib.rt_multi_destroy.argtypes = [C.c_void_p]
lib.rt_multi_destroy.restype = None
lib.rt_accum_create.argtypes = [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(C.c_void_p)]
lib.rt_accum_render.argtypes = [C.c_void_p, C.c_int32, C.POINTER(rt_stats)]
lib.rt_accum_samples.argtypes = [C.c_void_p]
lib.rt_accum_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.rt_accum_state_bytes.argtypes = [C.POINTER(rt_render_params)]
lib.rt_accum_state_bytes.restype = C.c_size_t
lib.rt_accum_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.rt_accum_load.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
lib.rt_accum_destroy.argtypes = [C.c_void_p]
lib.rt_accum_destroy.restype = None
lib.rt_multi_accum_create.argtypes = [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(C.c_void_p)]
lib.rt_multi_accum_render.argtypes = [C.c_void_p, C.c_int32, C.POINTER(rt_stats)]
lib.rt_multi_accum_samples.argtypes = [C.c_void_p]
lib.rt_multi_accum_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.rt_multi_accum_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.rt_multi_accum_load.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
lib.rt_multi_accum_destroy.argtypes = [C.c_void_p]
lib.rt_multi_accum_destroy.restype = None
for _family in ("rt_noise", "rt_multi_noise"):
    getattr(lib, _family + "_create").argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    for _name in ("_update", "_reset", "_batches", "_destroy"):
        getattr(lib, _family + _name).argtypes = [C.c_void_p]
    getattr(lib, _family + "_estimate").argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(rt_noise_summary)]
    getattr(lib, _family + "_destroy").restype = None
for _name in ("rt_query_closest", "rt_query_light_pdf", "rt_query_surface", "rt_query_environment"):
    getattr(lib, _name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_query_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_camera_rays.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
lib.rt_render_guides.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32] + [C.c_void_p] * 4 + [C.POINTER(rt_query_stats)]
lib.rt_rng_seed.argtypes = [C.c_void_p, C.c_uint32]
lib.rt_rng_seed.restype = None
lib.rt_rng_uniform.argtypes = [C.c_void_p]
lib.rt_rng_uniform.restype = C.c_float
lib.rt_query_scatter.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_query_bsdf.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_trace_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_bake_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_void_p, C.POINTER(rt_query_stats)]
lib.rt_bake.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(rt_bake_params), C.c_void_p, C.c_void_p, C.POINTER(rt_bake_stats)]
lib.rt_render_paths.argtypes = lib.rt_trace_paths.argtypes
lib.rt_render_bake.argtypes = lib.rt_bake.argtypes
lib.rt_render_probes.argtypes = lib.rt_bake.argtypes
lib.rt_adaptive_create.argtypes = [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(rt_adaptive_params), C.POINTER(C.c_void_p)]
lib.rt_adaptive_render.argtypes = [C.c_void_p, C.c_int32, C.POINTER(rt_adaptive_stats)]
lib.rt_adaptive_render_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(rt_adaptive_stats)]
lib.rt_adaptive_tiles.argtypes = [C.c_void_p, C.c_void_p]
lib.rt_adaptive_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.rt_adaptive_noise.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(rt_noise_summary)]
lib.rt_adaptive_sample_map.argtypes = [C.c_void_p, C.c_void_p]
lib.rt_adaptive_destroy.argtypes = [C.c_void_p]
lib.rt_adaptive_destroy.restype = None
lib.rt_views_create.argtypes = [C.c_void_p, C.POINTER(rt_views_params), C.c_void_p, C.POINTER(C.c_void_p)]
lib.rt_views_set_cameras.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
lib.rt_views_render.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(rt_views_stats)]
lib.rt_views_samples.argtypes = [C.c_void_p, C.c_void_p]
lib.rt_views_resolve.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.rt_views_destroy.argtypes = [C.c_void_p]
lib.rt_views_destroy.restype = None
lib.rt_view_adaptive_create.argtypes = [C.c_void_p, C.POINTER(rt_views_params), C.POINTER(rt_adaptive_params), C.c_void_p, C.POINTER(C.c_void_p)]
lib.rt_view_adaptive_set_cameras.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
lib.rt_view_adaptive_render.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(rt_view_adaptive_stats)]
lib.rt_view_adaptive_render_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(rt_view_adaptive_stats)]
lib.rt_view_adaptive_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
lib.rt_view_adaptive_resolve.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.rt_view_adaptive_noise.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.POINTER(rt_noise_summary)]
lib.rt_view_adaptive_sample_map.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
lib.rt_view_adaptive_destroy.argtypes = [C.c_void_p]
lib.rt_view_adaptive_destroy.restype = None
lib.rt_denoise.argtypes = [C.c_void_p, C.POINTER(rt_denoise_params)] + [C.c_void_p] * 8 + [C.POINTER(rt_denoise_stats)]
lib.rt_accum_denoise.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(rt_denoise_params), C.c_void_p, C.c_void_p, C.POINTER(rt_denoise_stats)]


def _check(code):
    if code < 0:
        raise RtError(code, lib.rt_last_error().decode("utf-8", "replace"))
    return code


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None and a.size else None


class SceneData:
    """Scene arrays in LOAD order as numpy (owns its memory) + an rt_scene_desc pointing at them."""

    def __init__(self, positions, texcoords, normals, tangents, material_index, materials, texture_source=(), images=(),
                 camera=None, bg=(0, 0, 0), environment=None, primitives=None, lights=None, ambient=(0, 0, 0)):
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self.positions = f32(positions if positions is not None else np.zeros(0, np.float32)).reshape(-1, 9)
        n = self.positions.shape[0]
        self.texcoords = None if texcoords is None else f32(texcoords).reshape(n, 6)
        self.normals = None if normals is None else f32(normals).reshape(n, 9)
        self.tangents = None if tangents is None else f32(tangents).reshape(n, 12)
        self.material_index = np.ascontiguousarray(material_index, dtype=np.uint32).reshape(n)
        self.materials = (rt_material * max(1, len(materials)))(*materials)
        self.n_materials = len(materials)
        self.texture_source = np.ascontiguousarray(texture_source, dtype=np.uint32)
        self.images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]  # each (h, w, 3)
        self.camera = camera if camera is not None else rt_camera()
        self.bg = tuple(float(x) for x in bg)
        self.environment = None if environment is None else np.ascontiguousarray(environment, dtype=np.uint8)
        self.primitives = primitives
        self.lights = lights
        self.ambient = tuple(float(x) for x in ambient)
        self._build_desc()

    def _build_desc(self):
        d = rt_scene_desc()
        d.struct_size = C.sizeof(rt_scene_desc)
        d.n_triangles = self.positions.shape[0]
        d.positions = _fptr(self.positions)
        d.texcoords = _fptr(self.texcoords)
        d.normals = _fptr(self.normals)
        d.tangents = _fptr(self.tangents)
        d.material_index = self.material_index.ctypes.data_as(C.POINTER(C.c_uint32))
        d.n_materials = self.n_materials
        d.materials = self.materials
        d.n_textures = self.texture_source.size
        d.texture_source = self.texture_source.ctypes.data_as(C.POINTER(C.c_uint32))
        self._images = (rt_image * max(1, len(self.images)))()
        for i, im in enumerate(self.images):
            self._images[i] = rt_image(im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8)))
        d.n_images = len(self.images)
        d.images = self._images
        if self.environment is not None:
            self._env = rt_image(self.environment.shape[1], self.environment.shape[0],
                                 self.environment.ctypes.data_as(C.POINTER(C.c_uint8)))
            d.environment_map = C.pointer(self._env)
        if self.primitives is not None and len(self.primitives):
            self._prims = (rt_primitive * len(self.primitives))(*self.primitives)
            d.n_primitives = len(self.primitives)
            d.primitives = self._prims
        d.camera = self.camera
        d.bg_color = (C.c_float * 3)(*self.bg)
        if self.lights is not None and len(self.lights):
            self._lights = (rt_light * len(self.lights))(*self.lights)
            d.n_lights = len(self.lights)
            d.lights = self._lights
        d.ambient_light = (C.c_float * 3)(*self.ambient)
        self.desc = d

    @staticmethod
    def from_desc(desc):
        """Deep-copy an rt_scene_desc (e.g. the loader's) into numpy-owned memory."""
        n = desc.n_triangles
        arr = lambda p, k: None if not p else np.ctypeslib.as_array(p, shape=(n * k,)).copy()
        mats = [rt_material.from_buffer_copy(desc.materials[i]) for i in range(desc.n_materials)]
        images = []
        for i in range(desc.n_images):
            im = desc.images[i]
            images.append(np.ctypeslib.as_array(im.rgb, shape=(im.height, im.width, 3)).copy())
        env = None
        if desc.environment_map:
            im = desc.environment_map.contents
            env = np.ctypeslib.as_array(im.rgb, shape=(im.height, im.width, 3)).copy()
        tsrc = np.ctypeslib.as_array(desc.texture_source, shape=(desc.n_textures,)).copy() if desc.n_textures else ()
        prims = [rt_primitive.from_buffer_copy(desc.primitives[i]) for i in range(desc.n_primitives)]
        lights = [rt_light.from_buffer_copy(desc.lights[i]) for i in range(desc.n_lights)]
        return SceneData(arr(desc.positions, 9), arr(desc.texcoords, 6), arr(desc.normals, 9), arr(desc.tangents, 12),
                         np.ctypeslib.as_array(desc.material_index, shape=(n,)).copy() if n else np.zeros(0, np.uint32),
                         mats, tsrc, images, rt_camera.from_buffer_copy(desc.camera), tuple(desc.bg_color), env, prims, lights,
                         tuple(desc.ambient_light))


def load_gltf(path, flavor=RT_INTEGRATOR_HW8, environment=None):
    """Load a glTF scene with the product's C++ loader and return it as SceneData."""
    hs = C.c_void_p()
    _check(lib.rt_load_gltf(os.fsencode(path), flavor, C.byref(hs)))
    try:
        if environment is not None:
            _check(lib.rt_host_scene_set_environment(hs, os.fsencode(environment)))
        return SceneData.from_desc(lib.rt_host_scene_desc(hs).contents)
    finally:
        lib.rt_host_scene_free(hs)


def load_txt(path, flavor=RT_INTEGRATOR_HW3):
    """Load a .txt scene (grammar of snapshot hw1..hw5 by flavor). Returns (SceneData, width, height, samples, ray_depth)."""
    hs = C.c_void_p()
    w, h, s, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib.rt_load_txt(os.fsencode(path), flavor, C.byref(hs), C.byref(w), C.byref(h), C.byref(s), C.byref(d)))
    try:
        return SceneData.from_desc(lib.rt_host_scene_desc(hs).contents), w.value, h.value, s.value, d.value
    finally:
        lib.rt_host_scene_free(hs)


def host_prepare_orders(data, integrator):
    """(figure order, light order) of the host-side scene preparation, without a GPU."""
    n = max(1, data.positions.shape[0], len(data.primitives or ()))
    fo, lo = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    k = _check(lib.rt_host_prepare_orders(C.byref(data.desc), integrator, fo.ctypes.data, n, lo.ctypes.data, n))
    nf = data.positions.shape[0] if data.positions.shape[0] else len(data.primitives or ())
    return fo[:nf], lo[:k]


def decode_png(path):
    w, h, p = C.c_int32(), C.c_int32(), C.POINTER(C.c_uint8)()
    _check(lib.rt_decode_png(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        lib.rt_free(p)


def write_ppm(path, rgb8):
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    _check(lib.rt_write_ppm(os.fsencode(path), rgb8.shape[1], rgb8.shape[0], rgb8.ctypes.data))


def dominant_kernel_name(st):
    """Name of the kernel rt_stats.dominant_kernel_ms / _launches refer to (for the hw8 / hw7 integrators)."""
    return {RT_PIPELINE_ROUNDS: "wf_traverse_kernel", RT_PIPELINE_PERSISTENT: "pt_persistent_kernel"}.get(st.pipeline, "render_hw8_kernel")


def pack_rays(o, d):
    """Origins and directions, (n, 3) each (or one (3,) vector), as one contiguous array of rt_ray records.  Refuses anything else
    before the library is called: the C side only sees a pointer and a count."""
    o, d = np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)
    if o.ndim == 1 and d.ndim == 1:
        o, d = o[None, :], d[None, :]
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"ray origins and directions must both be (n, 3), got {o.shape} and {d.shape}")
    rays = np.zeros(o.shape[0], dtype=RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    return rays


def rng_seed(seeds):
    """Engines seeded as std::minstd_rand::seed does (rt_rng_seed): an array of RNG_DTYPE records, one per seed.  No GPU needed."""
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint32))
    rng = np.zeros(seeds.shape, dtype=RNG_DTYPE)
    flat = rng.reshape(-1)
    for i, s in enumerate(seeds.reshape(-1)):
        lib.rt_rng_seed(flat.ctypes.data + i * RNG_DTYPE.itemsize, int(s))
    return rng


def rng_uniform(rng):
    """One uniform draw in [0, 1) from every engine of the RNG_DTYPE array, which advances in place (rt_rng_uniform): float32 array."""
    if not isinstance(rng, np.ndarray) or rng.dtype != RNG_DTYPE or not rng.flags.c_contiguous or not rng.flags.writeable:
        raise ValueError("rng must be a writeable C-contiguous array of RNG_DTYPE records")
    flat = rng.reshape(-1)
    out = np.zeros(flat.shape[0], dtype=np.float32)
    for i in range(flat.shape[0]):
        out[i] = lib.rt_rng_uniform(flat.ctypes.data + i * RNG_DTYPE.itemsize)
    return out.reshape(rng.shape)


def _records(a, dtype, n, name):
    """`a` as a contiguous array of n records of `dtype`; anything else is refused before the library is called."""
    a = np.ascontiguousarray(a)
    if a.dtype != dtype or a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError(f"{name} must be {'(n,)' if n is None else (n,)} records of {dtype.names}, got {a.dtype} {a.shape}")
    return a


def _engines(rng, n):
    if not isinstance(rng, np.ndarray) or not rng.flags.c_contiguous or not rng.flags.writeable:
        raise ValueError("rng must be a writeable C-contiguous array of RNG_DTYPE records: the engines advance in place")
    return _records(rng, RNG_DTYPE, n, "rng")


def make_params(width, height, samples, integrator=RT_INTEGRATOR_HW8, ray_depth=0, shard_index=0, shard_count=1,
                tile=32, flags=0, stream=None, sample_streams=0):
    p = rt_render_params()
    p.struct_size = C.sizeof(rt_render_params)
    p.width, p.height, p.samples, p.ray_depth, p.integrator = width, height, samples, ray_depth, integrator
    p.tile_w = p.tile_h = tile
    p.shard_index, p.shard_count, p.flags = shard_index, shard_count, flags
    p.stream = stream
    p.sample_streams = sample_streams  # 0/1 = replay mode (reference pixels); K > 1 = throughput mode, statistical parity only
    return p


def pack_bake_points(p, n=None):
    """Points (n, 3) and their normals (n, 3; None: zeros, which RT_BAKE_SH9 does not read) as one contiguous array of rt_bake_point
    records.  Refuses anything else before the library is called."""
    p = np.asarray(p, dtype=np.float32)
    n = np.zeros_like(p) if n is None else np.asarray(n, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or n.shape != p.shape:
        raise ValueError(f"points and normals must both be (n, 3), got {p.shape} and {n.shape}")
    points = np.zeros(p.shape[0], dtype=BAKE_POINT_DTYPE)
    points["p"], points["n"] = p, n
    return points


def make_bake_params(samples, streams=1, mode=RT_BAKE_IRRADIANCE, ray_depth=0, flags=0):
    params = rt_bake_params()
    params.struct_size = C.sizeof(rt_bake_params)
    params.mode, params.samples, params.streams, params.ray_depth, params.flags = mode, samples, streams, ray_depth, flags
    return params


def make_adaptive_params(target_noise, min_batches=0, max_samples=0, flags=0):
    """rt_adaptive_params; 0 selects the default of min_batches (4) and of max_samples (the sample-index limit)."""
    p = rt_adaptive_params()
    p.struct_size = C.sizeof(rt_adaptive_params)
    p.target_noise, p.min_batches, p.max_samples, p.flags = target_noise, min_batches, max_samples, flags
    return p


def _adaptive_stats():
    st = rt_adaptive_stats()
    st.struct_size = C.sizeof(rt_adaptive_stats)
    return st


def make_views_params(width, height, n_views, ray_depth=0, stream=None):
    """rt_views_params; ray_depth 0 selects the default (6)."""
    p = rt_views_params()
    p.struct_size = C.sizeof(rt_views_params)
    p.width, p.height, p.n_views, p.ray_depth, p.stream = width, height, n_views, ray_depth, stream
    return p


def _camera_array(cameras):
    """A contiguous array of rt_camera from a sequence of them (one rt_camera alone counts as a sequence of one)."""
    cameras = [cameras] if isinstance(cameras, rt_camera) else list(cameras)
    arr = (rt_camera * max(1, len(cameras)))()
    for i, c in enumerate(cameras):
        arr[i] = c
    return arr, len(cameras)


def make_denoise_params(width, height, iterations=0, sigma_depth=0.0, sigma_luminance=0.0, flags=0):
    """rt_denoise_params; 0 selects the default of iterations and of either sigma."""
    p = rt_denoise_params()
    p.struct_size = C.sizeof(rt_denoise_params)
    p.width, p.height, p.iterations = width, height, iterations
    p.sigma_depth, p.sigma_luminance, p.flags = sigma_depth, sigma_luminance, flags
    return p


def _denoise_stats():
    st = rt_denoise_stats()
    st.struct_size = C.sizeof(rt_denoise_stats)
    return st


def _query_stats():
    st = rt_query_stats()
    st.struct_size = C.sizeof(rt_query_stats)
    return st


def _bake_stats():
    st = rt_bake_stats()
    st.struct_size = C.sizeof(rt_bake_stats)
    return st


def _host_arrays_only(name, flags):
    """The host-array wrappers refuse RT_QUERY_DEVICE_POINTERS: their arrays are numpy's."""
    if flags & RT_QUERY_DEVICE_POINTERS:
        raise ValueError(f"{name} takes host arrays; device memory goes through {name}_device")


def unshard(params, buf):
    buf = np.ascontiguousarray(buf)
    full = np.zeros((params.height, params.width, 3), dtype=buf.dtype)
    _check(lib.rt_unshard(C.byref(params), buf.ctypes.data, buf.dtype.itemsize, full.ctypes.data))
    return full


class _Handle:
    """One object of the library: `_h` is its handle, `_destroy` names the C function that frees it.  close() closes the children
    first -- an rt_noise goes before its rt_accum, an rt_accum before its scene, and the same for the rt_multi_* family."""
    _destroy = None

    def _open(self, parent=None):
        self._h = C.c_void_p()
        self._children = weakref.WeakSet()
        if parent is not None:
            parent._children.add(self)

    def close(self):
        for child in list(self._children):
            child.close()
        if self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiScene(_Handle):
    """One scene replica per listed HIP device (rt_multi); render() shards the frame over them and returns the whole frame."""
    _destroy = "rt_multi_destroy"

    def __init__(self, data, devices):
        self.data = data
        self._open()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib.rt_multi_create(C.byref(data.desc), arr, len(devices), C.byref(self._h)))

    def render(self, width, height, samples, want_float=True, want_rgb8=True, **kw):
        p = make_params(width, height, samples, **kw)
        p.shard_count, p.shard_index = 0, 0
        rgb = np.zeros((height, width, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((height, width, 3), dtype=np.uint8) if want_rgb8 else None
        st = rt_stats()
        _check(lib.rt_multi_render(self._h, C.byref(p), rgb.ctypes.data if want_float else None,
                                   rgb8.ctypes.data if want_rgb8 else None, C.byref(st)))
        return rgb, rgb8, st

    def accumulator(self, width, height, **kw):
        """A resumable render of the frame on all the devices (MultiAccumulator); keywords as make_params."""
        return MultiAccumulator(self, width, height, **kw)


class NoiseMonitor(_Handle):
    """Noise of a frame in progress (rt_noise on an Accumulator): update() after every render(n) makes those n samples one batch;
    estimate() gives the per-pixel standard error of the picture's luminance and the figures of the frame.  It only reads the
    accumulator; close it before the accumulator (Accumulator.close() does)."""
    _family = "rt_noise"
    _destroy = "rt_noise_destroy"

    def __init__(self, accumulator):
        self.accumulator = accumulator  # keeps it alive: a monitor is destroyed before its accumulator
        self._open(accumulator)
        _check(getattr(lib, self._family + "_create")(accumulator._h, C.byref(self._h)))

    def update(self):
        _check(getattr(lib, self._family + "_update")(self._h))

    def reset(self):
        _check(getattr(lib, self._family + "_reset")(self._h))

    @property
    def batches(self):
        return _check(getattr(lib, self._family + "_batches")(self._h))

    def _map(self):
        p = rt_render_params.from_buffer_copy(self.accumulator.params)
        p.samples = 1
        if p.shard_count <= 1:
            return np.zeros((p.height, p.width), dtype=np.float32)
        return np.zeros(lib.rt_output_elems(C.byref(p)) // 3, dtype=np.float32)

    def estimate(self, want_map=True):
        """(standard error per pixel as float32 or None, rt_noise_summary): the map is (H, W), or the compact shard tiles."""
        se = self._map() if want_map else None
        summary = rt_noise_summary()
        summary.struct_size = C.sizeof(rt_noise_summary)
        _check(getattr(lib, self._family + "_estimate")(self._h, 0, se.ctypes.data if want_map else None, C.byref(summary)))
        return se, summary

    def estimate_device(self, out_se_ptr):
        """The map into device memory on the scene's GPU (a raw pointer, e.g. a torch tensor's data_ptr()); returns the summary."""
        summary = rt_noise_summary()
        summary.struct_size = C.sizeof(rt_noise_summary)
        _check(getattr(lib, self._family + "_estimate")(self._h, RT_FLAG_OUT_DEVICE, out_se_ptr, C.byref(summary)))
        return summary


class MultiNoiseMonitor(NoiseMonitor):
    """The same on a MultiAccumulator (rt_multi_noise): the map is the whole (H, W) frame, and the summary equals the unsharded
    single-device monitor's of the same slicing in every field."""
    _family = "rt_multi_noise"
    _destroy = "rt_multi_noise_destroy"

    def _map(self):
        return np.zeros((self.accumulator.params.height, self.accumulator.params.width), dtype=np.float32)

    def estimate_device(self, out_se_ptr):
        raise RtError(RT_ERR_INVALID_ARG, "rt_multi_noise_estimate writes host memory only")


class _AccumulatorBase(_Handle):
    """What Accumulator (`_family` rt_accum, on a Scene) and MultiAccumulator (rt_multi_accum, on a MultiScene) share: the handle on
    its parent, samples, render(n), load(blob) and the monitor."""
    _family = None
    _monitor = None

    def _create(self, parent, params):
        self.params = params
        self._open(parent)
        _check(getattr(lib, self._family + "_create")(parent._h, C.byref(self.params), C.byref(self._h)))

    @property
    def samples(self):
        return _check(getattr(lib, self._family + "_samples")(self._h))

    def render(self, n_samples):
        st = rt_stats()
        _check(getattr(lib, self._family + "_render")(self._h, n_samples, C.byref(st)))
        return st

    def _save(self, params):
        buf = C.create_string_buffer(lib.rt_accum_state_bytes(C.byref(params)))
        _check(getattr(lib, self._family + "_save")(self._h, buf, len(buf)))
        return buf.raw

    def load(self, blob):
        _check(getattr(lib, self._family + "_load")(self._h, blob, len(blob)))

    def noise_monitor(self):
        """A monitor of this frame: NoiseMonitor, or MultiNoiseMonitor on a MultiAccumulator."""
        return self._monitor(self)


class MultiAccumulator(_AccumulatorBase):
    """A frame in progress on every device of a MultiScene (rt_multi_accum), the counterpart of Accumulator: render(n) draws n more
    samples per pixel on all devices, resolve() is the whole picture so far, bit for bit Scene.render(width, height, samples);
    save() / load() exchange the portable checkpoint, byte for byte the blob of an unsharded Accumulator of the same frame."""
    _family = "rt_multi_accum"
    _destroy = "rt_multi_accum_destroy"
    _monitor = MultiNoiseMonitor

    def __init__(self, multi, width, height, **kw):
        self.multi = multi  # keeps the rt_multi alive: an rt_multi_accum is destroyed before it
        params = make_params(width, height, 0, **kw)
        if "shard_count" not in kw:
            params.shard_count, params.shard_index = 0, 0
        self._create(multi, params)

    def resolve(self, want_float=True, want_rgb8=True):
        """(rgb float32, rgb8) of the whole frame, (H, W, 3) each."""
        h, w = self.params.height, self.params.width
        rgb = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        _check(lib.rt_multi_accum_resolve(self._h, 0, rgb.ctypes.data if want_float else None, rgb8.ctypes.data if want_rgb8 else None))
        return rgb, rgb8

    def save(self):
        p = rt_render_params.from_buffer_copy(self.params)
        p.shard_count, p.shard_index = 0, 0   # the checkpoint is the unsharded frame's
        return self._save(p)


class Accumulator(_AccumulatorBase):
    """A frame in progress on a Scene (rt_accum): render(n) draws n more samples per pixel, resolve() is the picture so far,
    bit for bit Scene.render(width, height, samples); save() / load() move the state through host memory."""
    _family = "rt_accum"
    _destroy = "rt_accum_destroy"
    _monitor = NoiseMonitor

    def __init__(self, scene, width, height, **kw):
        self.scene = scene  # keeps the scene alive: an rt_accum is destroyed before its scene
        self._create(scene, make_params(width, height, 0, **kw))

    def resolve(self, want_float=True, want_rgb8=True):
        """(rgb float32, rgb8) in Scene.render's layout: (H, W, 3), or the compact shard buffers."""
        p = rt_render_params.from_buffer_copy(self.params)
        p.samples = 1
        n = lib.rt_output_elems(C.byref(p))
        rgb = np.zeros(n, dtype=np.float32) if want_float else None
        rgb8 = np.zeros(n, dtype=np.uint8) if want_rgb8 else None
        _check(lib.rt_accum_resolve(self._h, 0, rgb.ctypes.data if want_float else None, rgb8.ctypes.data if want_rgb8 else None))
        if p.shard_count <= 1:
            rgb = None if rgb is None else rgb.reshape(p.height, p.width, 3)
            rgb8 = None if rgb8 is None else rgb8.reshape(p.height, p.width, 3)
        return rgb, rgb8

    def save(self):
        return self._save(self.params)

    def denoise(self, monitor=None, albedo=False, want_float=True, want_rgb8=True, **kw):
        """The filtered preview of the picture so far (rt_accum_denoise): (rgb float32 (H, W, 3), rgb8, rt_denoise_stats).  monitor: a
        NoiseMonitor of this accumulator with two batches, whose error map steers the filter; albedo=True demodulates by the albedo
        plane; keywords as make_denoise_params."""
        h, w = self.params.height, self.params.width
        p = make_denoise_params(0, 0, **kw)
        p.flags |= RT_DENOISE_ALBEDO if albedo else 0
        rgb = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        st = _denoise_stats()
        _check(lib.rt_accum_denoise(self._h, monitor._h if monitor is not None else None, C.byref(p), rgb.ctypes.data if want_float else None,
                                    rgb8.ctypes.data if want_rgb8 else None, C.byref(st)))
        return rgb, rgb8, st


class AdaptiveRender(_Handle):
    """A frame in progress whose converged 8x8 sub-tiles stop drawing samples (rt_adaptive on a Scene): render(n) is one slice of the
    policy, render_tiles(n, mask) one of the caller's own mask; a sub-tile that has drawn d samples holds Scene.render(samples = d)'s
    pixels.  Keywords: target_noise, min_batches, max_samples, dilate, then make_params'."""
    _destroy = "rt_adaptive_destroy"

    def __init__(self, scene, width, height, target_noise, min_batches=0, max_samples=0, dilate=False, **kw):
        self.scene = scene  # keeps the scene alive: an rt_adaptive is destroyed before its scene
        self.params = make_params(width, height, 0, **kw)
        self.adaptive = make_adaptive_params(target_noise, min_batches, max_samples, RT_ADAPTIVE_DILATE if dilate else 0)
        self._open(scene)
        _check(lib.rt_adaptive_create(scene._h, C.byref(self.params), C.byref(self.adaptive), C.byref(self._h)))

    @property
    def grid(self):
        """(rows, columns) of the frame's 8x8 sub-tiles."""
        return (self.params.height + 7) // 8, (self.params.width + 7) // 8

    def render(self, n_samples):
        st = _adaptive_stats()
        _check(lib.rt_adaptive_render(self._h, n_samples, C.byref(st)))
        return st

    def render_tiles(self, n_samples, mask):
        """One slice for the sub-tiles whose byte of `mask` (rows x columns, or flat) is not 0."""
        mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
        if mask.size != self.grid[0] * self.grid[1]:
            raise ValueError(f"mask must hold one byte per sub-tile ({self.grid[0]} x {self.grid[1]}), got {mask.size}")
        st = _adaptive_stats()
        _check(lib.rt_adaptive_render_tiles(self._h, n_samples, mask.ctypes.data, C.byref(st)))
        return st

    def tiles(self):
        """The sub-tiles' entries, ADAPTIVE_TILE_DTYPE records of shape (rows, columns)."""
        out = np.zeros(self.grid, dtype=ADAPTIVE_TILE_DTYPE)
        _check(lib.rt_adaptive_tiles(self._h, out.ctypes.data))
        return out

    def resolve(self, want_float=True, want_rgb8=True):
        """(rgb float32, rgb8), (H, W, 3) each: every sub-tile's pixels are Scene.render's at that sub-tile's sample count."""
        h, w = self.params.height, self.params.width
        rgb = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        _check(lib.rt_adaptive_resolve(self._h, 0, rgb.ctypes.data if want_float else None, rgb8.ctypes.data if want_rgb8 else None))
        return rgb, rgb8

    def noise(self, want_map=True):
        """(standard error per pixel (H, W) or None, rt_noise_summary), the sample count read per sub-tile."""
        se = np.zeros((self.params.height, self.params.width), dtype=np.float32) if want_map else None
        summary = rt_noise_summary()
        summary.struct_size = C.sizeof(rt_noise_summary)
        _check(lib.rt_adaptive_noise(self._h, 0, se.ctypes.data if want_map else None, C.byref(summary)))
        return se, summary

    def sample_map(self):
        """Samples drawn per pixel, int32 (H, W)."""
        out = np.zeros((self.params.height, self.params.width), dtype=np.int32)
        _check(lib.rt_adaptive_sample_map(self._h, out.ctypes.data))
        return out


class ViewSet(_Handle):
    """A batch of cameras over one Scene (rt_views): render(n, mask) draws n more samples for the views whose byte of `mask` is not 0
    (None: all); view v after d samples holds what a Scene created with cameras[v] renders with samples = d.  The scene is only read.
    Keywords: ray_depth, stream."""
    _destroy = "rt_views_destroy"

    def __init__(self, scene, width, height, cameras, **kw):
        self.scene = scene  # keeps the scene alive: an rt_views is destroyed before its scene
        arr, n = _camera_array(cameras)
        self.params = make_views_params(width, height, n, **kw)
        self._open(scene)
        _check(lib.rt_views_create(scene._h, C.byref(self.params), C.cast(arr, C.c_void_p), C.byref(self._h)))

    def render(self, n_samples, mask=None):
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
            if mask.size != self.params.n_views:
                raise ValueError(f"mask must hold one byte per view ({self.params.n_views}), got {mask.size}")
        st = rt_views_stats()
        st.struct_size = C.sizeof(rt_views_stats)
        _check(lib.rt_views_render(self._h, n_samples, mask.ctypes.data if mask is not None else None, C.byref(st)))
        return st

    def samples(self):
        """Samples drawn per view, int32 (n_views,)."""
        out = np.zeros(self.params.n_views, dtype=np.int32)
        _check(lib.rt_views_samples(self._h, out.ctypes.data))
        return out

    def resolve(self, view, want_float=True, want_rgb8=True):
        """(rgb float32, rgb8) of one view, (H, W, 3) each."""
        h, w = self.params.height, self.params.width
        rgb = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        _check(lib.rt_views_resolve(self._h, view, 0, rgb.ctypes.data if want_float else None, rgb8.ctypes.data if want_rgb8 else None))
        return rgb, rgb8

    def set_cameras(self, first, cameras):
        """New cameras for views first .. first + len(cameras) - 1, which start over at 0 samples."""
        arr, n = _camera_array(cameras)
        _check(lib.rt_views_set_cameras(self._h, first, n, C.cast(arr, C.c_void_p)))


class AdaptiveViews(_Handle):
    """A batch of cameras over one Scene whose converged 8x8 sub-tiles stop drawing samples, per view (rt_view_adaptive): render(n, mask)
    is one slice of the policy for the views whose byte of `mask` is not 0 (None: all), render_tiles(n, mask) one of the caller's own
    mask per (view, sub-tile).  View v is what an AdaptiveRender with the same parameters does on a Scene created with cameras[v].
    Keywords: min_batches, max_samples, dilate, then make_views_params'."""
    _destroy = "rt_view_adaptive_destroy"

    def __init__(self, scene, width, height, cameras, target_noise, min_batches=0, max_samples=0, dilate=False, **kw):
        self.scene = scene  # keeps the scene alive: an rt_view_adaptive is destroyed before its scene
        arr, n = _camera_array(cameras)
        self.params = make_views_params(width, height, n, **kw)
        self.adaptive = make_adaptive_params(target_noise, min_batches, max_samples, RT_ADAPTIVE_DILATE if dilate else 0)
        self._open(scene)
        _check(lib.rt_view_adaptive_create(scene._h, C.byref(self.params), C.byref(self.adaptive), C.cast(arr, C.c_void_p), C.byref(self._h)))

    @property
    def grid(self):
        """(rows, columns) of one view's 8x8 sub-tiles."""
        return (self.params.height + 7) // 8, (self.params.width + 7) // 8

    @staticmethod
    def _stats():
        st = rt_view_adaptive_stats()
        st.struct_size = C.sizeof(rt_view_adaptive_stats)
        return st

    def render(self, n_samples, mask=None):
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
            if mask.size != self.params.n_views:
                raise ValueError(f"mask must hold one byte per view ({self.params.n_views}), got {mask.size}")
        st = self._stats()
        _check(lib.rt_view_adaptive_render(self._h, n_samples, mask.ctypes.data if mask is not None else None, C.byref(st)))
        return st

    def render_tiles(self, n_samples, mask):
        """One slice for the (view, sub-tile) pairs whose byte of `mask` (views x rows x columns, or flat) is not 0."""
        mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
        if mask.size != self.params.n_views * self.grid[0] * self.grid[1]:
            raise ValueError(f"mask must hold one byte per view and sub-tile ({self.params.n_views} x {self.grid[0]} x {self.grid[1]}), got {mask.size}")
        st = self._stats()
        _check(lib.rt_view_adaptive_render_tiles(self._h, n_samples, mask.ctypes.data, C.byref(st)))
        return st

    def tiles(self, view):
        """One view's entries, ADAPTIVE_TILE_DTYPE records of shape (rows, columns)."""
        out = np.zeros(self.grid, dtype=ADAPTIVE_TILE_DTYPE)
        _check(lib.rt_view_adaptive_tiles(self._h, view, out.ctypes.data))
        return out

    def resolve(self, view, want_float=True, want_rgb8=True):
        """(rgb float32, rgb8) of one view, (H, W, 3) each."""
        h, w = self.params.height, self.params.width
        rgb = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        _check(lib.rt_view_adaptive_resolve(self._h, view, 0, rgb.ctypes.data if want_float else None, rgb8.ctypes.data if want_rgb8 else None))
        return rgb, rgb8

    def noise(self, view, want_map=True):
        """(standard error per pixel (H, W) or None, rt_noise_summary) of one view."""
        se = np.zeros((self.params.height, self.params.width), dtype=np.float32) if want_map else None
        summary = rt_noise_summary()
        summary.struct_size = C.sizeof(rt_noise_summary)
        _check(lib.rt_view_adaptive_noise(self._h, view, 0, se.ctypes.data if want_map else None, C.byref(summary)))
        return se, summary

    def sample_map(self, view):
        """Samples drawn per pixel of one view, int32 (H, W)."""
        out = np.zeros((self.params.height, self.params.width), dtype=np.int32)
        _check(lib.rt_view_adaptive_sample_map(self._h, view, out.ctypes.data))
        return out

    def set_cameras(self, first, cameras):
        """New cameras for views first .. first + len(cameras) - 1, which start over: no samples, every sub-tile active."""
        arr, n = _camera_array(cameras)
        _check(lib.rt_view_adaptive_set_cameras(self._h, first, n, C.cast(arr, C.c_void_p)))


class Scene(_Handle):
    """A prepared scene resident in HBM on the current HIP device (rt_scene)."""
    _destroy = "rt_scene_destroy"

    def __init__(self, data, build_flags=0):
        self.data = data
        self._open()
        desc = rt_scene_desc.from_buffer_copy(data.desc)   # the arrays stay owned by `data`
        desc.build_flags = build_flags
        _check(lib.rt_scene_create(C.byref(desc), C.byref(self._h)))

    def info(self):
        i = rt_scene_info()
        _check(lib.rt_scene_get_info(self._h, C.byref(i)))
        return i

    def light_order(self):
        n = self.info().n_lights
        out = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib.rt_scene_get_light_order(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out[:n]

    def render(self, width, height, samples, want_float=True, want_rgb8=True, counters=False, flags=0, **kw):
        """Render to host arrays. Returns (rgb float32 (H,W,3) or shard buffer, rgb8, rt_stats)."""
        p = make_params(width, height, samples, flags=(RT_FLAG_COUNTERS if counters else 0) | flags, **kw)
        n = lib.rt_output_elems(C.byref(p))
        if n == 0:
            raise RtError(-1, "bad render parameters")
        rgb = np.zeros(n, dtype=np.float32) if want_float else None
        rgb8 = np.zeros(n, dtype=np.uint8) if want_rgb8 else None
        st = rt_stats()
        _check(lib.rt_render(self._h, C.byref(p), rgb.ctypes.data if want_float else None,
                             rgb8.ctypes.data if want_rgb8 else None, C.byref(st)))
        if p.shard_count <= 1:
            rgb = None if rgb is None else rgb.reshape(height, width, 3)
            rgb8 = None if rgb8 is None else rgb8.reshape(height, width, 3)
        return rgb, rgb8, st

    def accumulator(self, width, height, **kw):
        """A resumable render of this scene (Accumulator); keywords as make_params."""
        return Accumulator(self, width, height, **kw)

    def adaptive(self, width, height, target_noise, **kw):
        """An adaptive render of this scene (AdaptiveRender)."""
        return AdaptiveRender(self, width, height, target_noise, **kw)

    def views(self, width, height, cameras, **kw):
        """A batch of cameras over this scene (ViewSet)."""
        return ViewSet(self, width, height, cameras, **kw)

    def adaptive_views(self, width, height, cameras, target_noise, **kw):
        """A batch of cameras over this scene with adaptive sampling per view (AdaptiveViews)."""
        return AdaptiveViews(self, width, height, cameras, target_noise, **kw)

    def render_device(self, params, out_rgb_ptr, out_rgb8_ptr):
        """Render into device buffers (raw pointers, e.g. torch tensor data_ptr())."""
        st = rt_stats()
        params.flags |= RT_FLAG_OUT_DEVICE
        _check(lib.rt_render(self._h, C.byref(params), out_rgb_ptr, out_rgb8_ptr, C.byref(st)))
        return st

    def _query(self, fn, rays_ptr, n, flags, out_ptr):
        st = _query_stats()
        _check(fn(self._h, rays_ptr, n, flags, out_ptr, C.byref(st)))
        return st

    def query_closest(self, o, d, flags=0):
        """Closest hits of the rays (o[i], d[i]) (rt_query_closest): (array of HIT_DTYPE records, rt_query_stats)."""
        _host_arrays_only("query_closest", flags)
        rays = pack_rays(o, d)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        return hits, self._query(lib.rt_query_closest, rays.ctypes.data, rays.shape[0], flags, hits.ctypes.data)

    def query_light_pdf(self, x, d, flags=0):
        """Light pdf of the directions d[i] seen from x[i] (rt_query_light_pdf): (float32 array, rt_query_stats)."""
        _host_arrays_only("query_light_pdf", flags)
        rays = pack_rays(x, d)
        pdf = np.zeros(rays.shape[0], dtype=np.float32)
        return pdf, self._query(lib.rt_query_light_pdf, rays.ctypes.data, rays.shape[0], flags, pdf.ctypes.data)

    def query_occluded(self, o, d, tmax=None, flags=0):
        """Is anything in front of tmax[i] on the ray (o[i], d[i]) (rt_query_occluded; tmax None: does the ray hit anything):
        (uint8 array of RT_OCCLUSION_* bits, rt_query_stats)."""
        _host_arrays_only("query_occluded", flags)
        rays = pack_rays(o, d)
        n = rays.shape[0]
        if tmax is not None:
            tmax = np.ascontiguousarray(tmax, dtype=np.float32)
            if tmax.shape != (n,):
                raise ValueError(f"tmax must have shape ({n},), one bound per ray; got {tmax.shape}")
        out = np.zeros(n, dtype=np.uint8)
        st = _query_stats()
        _check(lib.rt_query_occluded(self._h, rays.ctypes.data, None if tmax is None else tmax.ctypes.data, n, flags, out.ctypes.data, C.byref(st)))
        return out, st

    def query_occluded_device(self, rays_ptr, tmax_ptr, n, out_ptr, flags=0):
        """The same on device memory: n rt_ray and n floats (or None) in, n bytes out, no alignment demand on out."""
        st = _query_stats()
        _check(lib.rt_query_occluded(self._h, rays_ptr, tmax_ptr, n, flags | RT_QUERY_DEVICE_POINTERS, out_ptr, C.byref(st)))
        return st

    def query_closest_device(self, rays_ptr, n, out_ptr, flags=0):
        """The same on device memory of the scene's GPU (raw pointers, e.g. torch tensor data_ptr()): n rt_ray in, n rt_hit out."""
        return self._query(lib.rt_query_closest, rays_ptr, n, flags | RT_QUERY_DEVICE_POINTERS, out_ptr)

    def query_light_pdf_device(self, rays_ptr, n, out_ptr, flags=0):
        return self._query(lib.rt_query_light_pdf, rays_ptr, n, flags | RT_QUERY_DEVICE_POINTERS, out_ptr)

    def query_surface(self, hits):
        """What the shader knows about each hit before it samples a direction (rt_query_surface): (array of SURFACE_DTYPE records,
        rt_query_stats).  hits: HIT_DTYPE records, as query_closest returns them or altered."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        out = np.zeros(hits.shape[0], dtype=SURFACE_DTYPE)
        return out, self._query(lib.rt_query_surface, hits.ctypes.data, hits.shape[0], 0, out.ctypes.data)

    def query_environment(self, o, d):
        """What the rays (o[i], d[i]) see where they miss (rt_query_environment): ((n, 3) float32 array, rt_query_stats)."""
        rays = pack_rays(o, d)
        rgb = np.zeros((rays.shape[0], 3), dtype=np.float32)
        return rgb, self._query(lib.rt_query_environment, rays.ctypes.data, rays.shape[0], 0, rgb.ctypes.data)

    def camera_rays(self, width, height, xy):
        """The camera rays of a width x height frame through the points xy (n, 2) of its image plane, in pixel units
        (rt_camera_rays): (o, d), (n, 3) float32 each."""
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError(f"xy must be (n, 2), got {xy.shape}")
        rays = np.zeros(xy.shape[0], dtype=RAY_DTYPE)
        _check(lib.rt_camera_rays(self._h, width, height, xy.ctypes.data, xy.shape[0], 0, rays.ctypes.data))
        return rays["o"].copy(), rays["d"].copy()

    def render_guides(self, width, height, albedo=True, normal=True, depth=True, emission=True):
        """First-hit guide images of a width x height frame (rt_render_guides): (dict of the planes asked for -- albedo, normal,
        emission (H, W, 3), depth (H, W), float32 --, rt_query_stats)."""
        want = {"albedo": albedo, "normal": normal, "depth": depth, "emission": emission}
        planes = {k: np.zeros((height, width) if k == "depth" else (height, width, 3), dtype=np.float32) for k, v in want.items() if v}
        ptr = [planes[k].ctypes.data if k in planes else None for k in want]
        st = _query_stats()
        _check(lib.rt_render_guides(self._h, width, height, 0, *ptr, C.byref(st)))
        return planes, st

    def denoise(self, rgb, normal, depth, albedo=None, emission=None, se=None, want_float=True, want_rgb8=True, **kw):
        """The preview filter on host planes (rt_denoise): rgb, normal (H, W, 3), depth (H, W), optionally albedo, emission (H, W, 3) and
        se (H, W), float32; keywords as make_denoise_params.  Returns (rgb float32 (H, W, 3), rgb8, rt_denoise_stats)."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise ValueError(f"depth must be (H, W), got {depth.shape}")
        h, w = depth.shape
        planes = []
        for name, a, shape in (("rgb", rgb, (h, w, 3)), ("normal", normal, (h, w, 3)), ("depth", depth, (h, w)), ("albedo", albedo, (h, w, 3)),
                               ("emission", emission, (h, w, 3)), ("se", se, (h, w))):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float32)
            if a is not None and a.shape != shape:
                raise ValueError(f"{name} must be {shape}, got {a.shape}")
            planes.append(a)
        out = np.zeros((h, w, 3), dtype=np.float32) if want_float else None
        out8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        p = make_denoise_params(w, h, **kw)
        st = _denoise_stats()
        _check(lib.rt_denoise(self._h, C.byref(p), *[None if a is None else a.ctypes.data for a in planes],
                              out.ctypes.data if want_float else None, out8.ctypes.data if want_rgb8 else None, C.byref(st)))
        return out, out8, st

    def denoise_device(self, width, height, rgb_ptr, normal_ptr, depth_ptr, albedo_ptr=None, emission_ptr=None, se_ptr=None,
                       out_rgb_ptr=None, out_rgb8_ptr=None, **kw):
        """The same on device memory of the scene's GPU (raw pointers, e.g. torch tensor data_ptr()); out_rgb_ptr may be rgb_ptr."""
        p = make_denoise_params(width, height, **kw)
        p.flags |= RT_DENOISE_DEVICE_POINTERS
        st = _denoise_stats()
        _check(lib.rt_denoise(self._h, C.byref(p), rgb_ptr, normal_ptr, depth_ptr, albedo_ptr, emission_ptr, se_ptr, out_rgb_ptr, out_rgb8_ptr, C.byref(st)))
        return st

    def query_surface_device(self, hits_ptr, n, out_ptr):
        """The same on device memory of the scene's GPU: n rt_hit in, n rt_surface out, both 16-byte aligned."""
        return self._query(lib.rt_query_surface, hits_ptr, n, RT_QUERY_DEVICE_POINTERS, out_ptr)

    def query_environment_device(self, rays_ptr, n, out_ptr):
        return self._query(lib.rt_query_environment, rays_ptr, n, RT_QUERY_DEVICE_POINTERS, out_ptr)

    def camera_rays_device(self, width, height, xy_ptr, n, out_ptr):
        _check(lib.rt_camera_rays(self._h, width, height, xy_ptr, n, RT_QUERY_DEVICE_POINTERS, out_ptr))

    def render_guides_device(self, width, height, albedo_ptr=None, normal_ptr=None, depth_ptr=None, emission_ptr=None):
        st = _query_stats()
        _check(lib.rt_render_guides(self._h, width, height, RT_QUERY_DEVICE_POINTERS, albedo_ptr, normal_ptr, depth_ptr, emission_ptr, C.byref(st)))
        return st

    def query_scatter(self, o, d, hits, surfaces, rng, flags=0):
        """One bounce of Scene::getColor per record (rt_query_scatter): the rays (o[i], d[i]) that hit, their HIT_DTYPE and
        SURFACE_DTYPE records and their engines, an RNG_DTYPE array that advances in place: (array of SCATTER_DTYPE records,
        rt_query_stats).  flags: RT_QUERY_REFERENCE_WALK."""
        _host_arrays_only("query_scatter", flags)
        rays = pack_rays(o, d)
        n = rays.shape[0]
        hits, surfaces, rng = _records(hits, HIT_DTYPE, n, "hits"), _records(surfaces, SURFACE_DTYPE, n, "surfaces"), _engines(rng, n)
        out = np.zeros(n, dtype=SCATTER_DTYPE)
        st = _query_stats()
        _check(lib.rt_query_scatter(self._h, rays.ctypes.data, hits.ctypes.data, surfaces.ctypes.data, rng.ctypes.data, n, flags, out.ctypes.data, C.byref(st)))
        return out, st

    def query_scatter_device(self, rays_ptr, hits_ptr, surfaces_ptr, rng_ptr, n, out_ptr, flags=0):
        """The same on device memory of the scene's GPU: every record array but the rays 16-byte aligned; the engines advance in place."""
        st = _query_stats()
        _check(lib.rt_query_scatter(self._h, rays_ptr, hits_ptr, surfaces_ptr, rng_ptr, n, flags | RT_QUERY_DEVICE_POINTERS, out_ptr, C.byref(st)))
        return st

    def query_bsdf(self, o, d, hits, surfaces, dirs, flags=0):
        """brdf and Mix::pdf of the directions dirs[i] at the hits of the rays (o[i], d[i]) (rt_query_bsdf): ((n, 3) float32, (n,)
        float32, rt_query_stats)."""
        _host_arrays_only("query_bsdf", flags)
        rays = pack_rays(o, d)
        n = rays.shape[0]
        hits, surfaces = _records(hits, HIT_DTYPE, n, "hits"), _records(surfaces, SURFACE_DTYPE, n, "surfaces")
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        if dirs.shape != (n, 3):
            raise ValueError(f"dirs must be ({n}, 3), got {dirs.shape}")
        brdf, pdf = np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.float32)
        st = _query_stats()
        _check(lib.rt_query_bsdf(self._h, rays.ctypes.data, hits.ctypes.data, surfaces.ctypes.data, dirs.ctypes.data, n, flags, brdf.ctypes.data, pdf.ctypes.data, C.byref(st)))
        return brdf, pdf, st

    def query_bsdf_device(self, rays_ptr, hits_ptr, surfaces_ptr, dirs_ptr, n, out_brdf_ptr, out_pdf_ptr, flags=0):
        st = _query_stats()
        _check(lib.rt_query_bsdf(self._h, rays_ptr, hits_ptr, surfaces_ptr, dirs_ptr, n, flags | RT_QUERY_DEVICE_POINTERS, out_brdf_ptr, out_pdf_ptr, C.byref(st)))
        return st

    def trace_paths(self, o, d, rng, ray_depth=0, flags=0):
        """Scene::getColor(ray, ray_depth) for the rays (o[i], d[i]) with the engines rng[i], which advance in place (rt_trace_paths):
        ((n, 3) float32 radiance, rt_query_stats).  ray_depth 0 = 6."""
        _host_arrays_only("trace_paths", flags)
        rays = pack_rays(o, d)
        n = rays.shape[0]
        rng = _engines(rng, n)
        rgb = np.zeros((n, 3), dtype=np.float32)
        st = _query_stats()
        _check(lib.rt_trace_paths(self._h, rays.ctypes.data, rng.ctypes.data, n, ray_depth, flags, rgb.ctypes.data, C.byref(st)))
        return rgb, st

    def trace_paths_device(self, rays_ptr, rng_ptr, n, out_rgb_ptr, ray_depth=0, flags=0):
        st = _query_stats()
        _check(lib.rt_trace_paths(self._h, rays_ptr, rng_ptr, n, ray_depth, flags | RT_QUERY_DEVICE_POINTERS, out_rgb_ptr, C.byref(st)))
        return st

    def bake_rays(self, points, rng, mode=RT_BAKE_IRRADIANCE):
        """One ray per BAKE_POINT_DTYPE record from the record's engine (rt_bake_rays): o = p + eps * n with a cosine-distributed d
        (RT_BAKE_IRRADIANCE) or o = p with a uniform d (RT_BAKE_SH9).  rng: an RNG_DTYPE array that advances in place.  Returns
        (array of RAY_DTYPE records, rt_query_stats)."""
        points = _records(points, BAKE_POINT_DTYPE, None, "points")
        n = points.shape[0]
        rng = _engines(rng, n)
        rays = np.zeros(n, dtype=RAY_DTYPE)
        st = _query_stats()
        _check(lib.rt_bake_rays(self._h, points.ctypes.data, rng.ctypes.data, n, mode, 0, rays.ctypes.data, C.byref(st)))
        return rays, st

    def bake_rays_device(self, points_ptr, rng_ptr, n, out_ptr, mode=RT_BAKE_IRRADIANCE):
        """The same on device memory of the scene's GPU: rt_rng 16-byte aligned, points and rays 4-byte."""
        st = _query_stats()
        _check(lib.rt_bake_rays(self._h, points_ptr, rng_ptr, n, mode, RT_QUERY_DEVICE_POINTERS, out_ptr, C.byref(st)))
        return st

    def bake(self, points, rng, samples, streams=1, mode=RT_BAKE_IRRADIANCE, ray_depth=0, flags=0):
        """Irradiance (n, 3) or SH9 coefficients (n, 9, 3) at the BAKE_POINT_DTYPE records (rt_bake): per point `streams` engines,
        rng[i * streams + k], which advance in place and draw samples / streams paths each.  flags: RT_QUERY_REFERENCE_WALK,
        RT_BAKE_LOCKSTEP.  Returns (float32 array, rt_bake_stats)."""
        _host_arrays_only("bake", flags)
        if mode not in BAKE_FLOATS:
            raise ValueError(f"mode must be RT_BAKE_IRRADIANCE or RT_BAKE_SH9, got {mode}")
        points = _records(points, BAKE_POINT_DTYPE, None, "points")
        n = points.shape[0]
        rng = _engines(rng, n * max(1, streams))
        out = np.zeros((n, 3) if mode == RT_BAKE_IRRADIANCE else (n, 9, 3), dtype=np.float32)
        st = _bake_stats()
        params = make_bake_params(samples, streams, mode, ray_depth, flags)
        _check(lib.rt_bake(self._h, points.ctypes.data, n, C.byref(params), rng.ctypes.data, out.ctypes.data, C.byref(st)))
        return out, st

    def bake_device(self, points_ptr, rng_ptr, n_points, out_ptr, samples, streams=1, mode=RT_BAKE_IRRADIANCE, ray_depth=0, flags=0):
        st = _bake_stats()
        params = make_bake_params(samples, streams, mode, ray_depth, flags | RT_QUERY_DEVICE_POINTERS)
        _check(lib.rt_bake(self._h, points_ptr, n_points, C.byref(params), rng_ptr, out_ptr, C.byref(st)))
        return st

    def render_paths(self, o, d, rng, ray_depth=0):
        """trace_paths through the persistent render kernel (rt_render_paths): the same radiance and engines on a scene whose renders
        report reference_exact = 1, one launch per chunk instead of a round of launches per bounce.  Returns ((n, 3) float32, rt_query_stats)."""
        rays = pack_rays(o, d)
        n = rays.shape[0]
        rng = _engines(rng, n)
        rgb = np.zeros((n, 3), dtype=np.float32)
        st = _query_stats()
        _check(lib.rt_render_paths(self._h, rays.ctypes.data, rng.ctypes.data, n, ray_depth, 0, rgb.ctypes.data, C.byref(st)))
        return rgb, st

    def render_paths_device(self, rays_ptr, rng_ptr, n, out_rgb_ptr, ray_depth=0):
        st = _query_stats()
        _check(lib.rt_render_paths(self._h, rays_ptr, rng_ptr, n, ray_depth, RT_QUERY_DEVICE_POINTERS, out_rgb_ptr, C.byref(st)))
        return st

    def render_bake(self, points, rng, samples, streams=1, mode=RT_BAKE_IRRADIANCE, ray_depth=0):
        """bake in RT_BAKE_IRRADIANCE through the persistent render kernel (rt_render_bake; RT_BAKE_SH9 is refused: bake serves it).
        Returns ((n, 3) float32, rt_bake_stats)."""
        points = _records(points, BAKE_POINT_DTYPE, None, "points")
        n = points.shape[0]
        rng = _engines(rng, n * max(1, streams))
        out = np.zeros((n, 3), dtype=np.float32)
        st = _bake_stats()
        params = make_bake_params(samples, streams, mode, ray_depth, 0)
        _check(lib.rt_render_bake(self._h, points.ctypes.data, n, C.byref(params), rng.ctypes.data, out.ctypes.data, C.byref(st)))
        return out, st

    def render_bake_device(self, points_ptr, rng_ptr, n_points, out_ptr, samples, streams=1, mode=RT_BAKE_IRRADIANCE, ray_depth=0):
        st = _bake_stats()
        params = make_bake_params(samples, streams, mode, ray_depth, RT_QUERY_DEVICE_POINTERS)
        _check(lib.rt_render_bake(self._h, points_ptr, n_points, C.byref(params), rng_ptr, out_ptr, C.byref(st)))
        return st

    def render_probes(self, points, rng, samples, streams=1, ray_depth=0):
        """bake in RT_BAKE_SH9 through the persistent render kernel (rt_render_probes): the same coefficients and engines as bake on a
        scene whose renders report reference_exact = 1.  Returns ((n, 9, 3) float32, rt_bake_stats)."""
        points = _records(points, BAKE_POINT_DTYPE, None, "points")
        n = points.shape[0]
        rng = _engines(rng, n * max(1, streams))
        out = np.zeros((n, 9, 3), dtype=np.float32)
        st = _bake_stats()
        params = make_bake_params(samples, streams, RT_BAKE_SH9, ray_depth, 0)
        _check(lib.rt_render_probes(self._h, points.ctypes.data, n, C.byref(params), rng.ctypes.data, out.ctypes.data, C.byref(st)))
        return out, st

    def render_probes_device(self, points_ptr, rng_ptr, n_points, out_ptr, samples, streams=1, ray_depth=0):
        st = _bake_stats()
        params = make_bake_params(samples, streams, RT_BAKE_SH9, ray_depth, RT_QUERY_DEVICE_POINTERS)
        _check(lib.rt_render_probes(self._h, points_ptr, n_points, C.byref(params), rng_ptr, out_ptr, C.byref(st)))
        return st

/*
 * rtamd.h — C-ABI of the MI355X-native path-tracing render path.
 *
 * This is the drop-in boundary for the reference renderer's per-pixel render loop
 * (reference: hw8/src/sceneio.cpp:381-402 `sceneio::renderScene`, whose parallel-for body
 * calls `Scene::getPixel`, hw8/src/scene.cpp:167-177, then the tonemap chain
 * hw8/src/color.cpp:4-31).  The reference has no FFI of its own; the functions below are
 * what a binding for that seam needs (see INTEGRATION.md for the reference-side stub):
 *
 *   rt_scene_create   replaces  Scene::initBVH + Scene::initDistribution  (hw8/src/scene.cpp:65-78)
 *                     plus the upload of the flattened scene to HBM (once).
 *   rt_render         replaces  the `#pragma omp parallel for` of renderScene
 *                     (hw8/src/sceneio.cpp:387-396): per-pixel minstd_rand(y*W+x) replay,
 *                     getPixel, aces_tonemap/gamma_corrected/toExternColorFormat.
 *   rt_scene_destroy  replaces  Scene::~Scene (hw8/src/scene.cpp:56-63).
 * Below that seam, for a caller with a render loop of its own:
 *   rt_query_closest    answers  BVH::intersect (hw8/src/include/bvh.h:111-142) for a batch of rays,
 *   rt_query_light_pdf  answers  FiguresMix::pdf (hw8/src/include/distributions.h:122-124),
 *   rt_query_occluded   answers  whether BVH::intersect reports a hit below a bound tmax[i] (a visibility pass's yes / no),
 *   rt_query_surface / rt_query_environment / rt_camera_rays  answer  the material fetch, the miss colour and getCameraRay of
 *                     Scene::getColor / getPixel (hw8/src/scene.cpp:90-149,179-186); rt_render_guides composes them per pixel.
 *
 * Conventions: plain C, plain pointers and sizes, no exceptions cross the boundary.
 * Every function returns 0 on success and a negative rt_status on failure;
 * rt_last_error() returns a thread-local message for the last failure.  The library owns all
 * device memory; the caller owns every host buffer passed in and may free the rt_scene_desc
 * arrays as soon as rt_scene_create returns.  One rt_scene lives on one GPU (the HIP device
 * current at creation); calls on one rt_scene must be serialised by the caller.
 * There is no CPU fallback: if no HIP device is usable the calls fail with RT_ERR_NO_DEVICE.
 */
#ifndef RTAMD_H
#define RTAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTAMD_ABI_VERSION 6

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,
    RT_ERR_NO_DEVICE = -2,
    RT_ERR_HIP = -3,
    RT_ERR_UNSUPPORTED = -4,
    RT_ERR_IO = -5,
    RT_ERR_PARSE = -6,
    RT_ERR_LIMIT = -7
} rt_status;

/* Which reference integrator the render loop replays. */
typedef enum rt_integrator {
    RT_INTEGRATOR_HW1 = 1, /* ray caster,  hw1/src/scene.cpp:7-30   */
    RT_INTEGRATOR_HW2 = 2, /* Whitted-style: point/directional lights, shadow rays, mirror + Fresnel-weighted refraction, hw2/src/scene.cpp:30-84 */
    RT_INTEGRATOR_HW3 = 3, /* first path tracer over analytic primitives, hw3/src/scene.cpp:31-107 */
    RT_INTEGRATOR_HW4 = 4, /* + cosine / box-light / ellipsoid-light mixture sampling, hw4/src/scene.cpp:10-112, distributions.h */
    RT_INTEGRATOR_HW5 = 5, /* + TRIANGLE primitives, BVH over non-planes, per-pixel engines, hw5/src/scene.cpp:47-112 */
    RT_INTEGRATOR_HW6 = 6, /* triangles, DIFFUSE/METALLIC/DIELECTRIC, hw6/src/scene.cpp:47-105    */
    RT_INTEGRATOR_HW7 = 7, /* hw8's integrator without textures: per-material BRDF without the v.n / l.n gates, alpha = roughness^2,
                              geometric normal in the light pdf (hw7/src/scene.cpp:29-61); renders scenes created for HW8 */
    RT_INTEGRATOR_HW8 = 8  /* glTF PBR + textures + mixture sampling, hw8/src/scene.cpp:84-165     */
} rt_integrator;

/* hw3/hw6 material classes (hw3/src/include/primitives.h, hw6/src/include/primitives.h). */
typedef enum rt_material_kind { RT_MAT_DIFFUSE = 0, RT_MAT_METALLIC = 1, RT_MAT_DIELECTRIC = 2 } rt_material_kind;

/* glTF material as the reference keeps it (hw8/src/include/gltf_structs.h:38-47).
 * Texture fields are glTF *texture* indices (into rt_scene_desc.texture_source) or -1. */
typedef struct rt_material {
    float base_color[3];   /* baseColorFactor rgb, default 1,1,1 */
    float emission[3];     /* emissiveFactor * KHR_materials_emissive_strength, default 0 */
    float metallic_factor; /* default 1 */
    float roughness_factor;/* default 1 */
    int32_t base_color_texture;
    int32_t emissive_texture;
    int32_t metallic_roughness_texture;
    int32_t normal_texture;
    int32_t kind;          /* rt_material_kind; used by the HW3/HW6 integrators only */
    float ior;             /* HW3/HW6 dielectric index of refraction */
} rt_material;

/* 8-bit RGB image, row 0 first, tightly packed (what stbi_load(...,3) hands the reference,
 * hw8/src/sceneio.cpp:374-379). */
typedef struct rt_image {
    int32_t width, height;
    const uint8_t *rgb;
} rt_image;

/* Analytic primitive of the .txt scenes (hw1/hw3: hw3/src/include/primitives.h:17-44). */
typedef enum rt_primitive_type { RT_PRIM_ELLIPSOID = 0, RT_PRIM_PLANE = 1, RT_PRIM_BOX = 2, RT_PRIM_TRIANGLE = 3 } rt_primitive_type;
typedef struct rt_primitive {
    int32_t type;        /* rt_primitive_type */
    float data[3];       /* radii | plane normal | box half-sizes | triangle: Figure::data (third vertex of the TRIANGLE line) */
    float position[3];
    float rotation[4];   /* quaternion x,y,z,w exactly as parsed (may be non-unit) */
    float color[3];
    float emission[3];
    int32_t kind;        /* rt_material_kind */
    float ior;
    float data2[3];      /* TRIANGLE (hw5/src/sceneio.cpp:27-29): second vertex of the line */
    float data3[3];      /* TRIANGLE: first vertex of the line (the BVH / light code's "a") */
} rt_primitive;

/* hw2 light source (hw2/src/include/light_source.h:15-30). */
typedef enum rt_light_type { RT_LIGHT_POINT = 0, RT_LIGHT_DIRECTIONAL = 1 } rt_light_type;
typedef struct rt_light {
    int32_t type;         /* rt_light_type */
    float intensity[3];
    float position[3];    /* point light */
    float attenuation[3]; /* point light: c0 + c1*r + c2*r^2 */
    float direction[3];   /* directional light, as parsed (normalised per query like the reference) */
} rt_light;

typedef struct rt_camera {
    float position[3], right[3], up[3], forward[3];
    float fov_y;         /* glTF scenes (hw6-hw8): yfov in radians */
    float fov_x;         /* .txt scenes (hw1-hw5): CAMERA_FOV_X in radians */
} rt_camera;

/* Scene description: host arrays in LOAD order (the order the reference's loader appends
 * Figures, hw8/src/sceneio.cpp:247-310).  Per triangle the three vertices are stored in the
 * order of the reference's Figure members (data, data2, data3) — i.e. glTF corners (1,3,2),
 * hw8/src/sceneio.cpp:289. */
typedef struct rt_scene_desc {
    uint32_t struct_size;            /* = sizeof(rt_scene_desc) */
    uint32_t n_triangles;            /* hw7 / hw8 scenes: at most 2^24 - 2 (24 bits of figure index in a hit record) */
    const float *positions;          /* n_triangles * 9  */
    const float *texcoords;          /* n_triangles * 6  (may be NULL for HW6) */
    const float *normals;            /* n_triangles * 9  (may be NULL for HW6) */
    const float *tangents;           /* n_triangles * 12 (xyz,w; may be NULL for HW6) */
    const uint32_t *material_index;  /* n_triangles */
    uint32_t n_materials;
    const rt_material *materials;
    uint32_t n_textures;
    const uint32_t *texture_source;  /* glTF textures[i].source */
    uint32_t n_images;
    const rt_image *images;
    const rt_image *environment_map; /* NULL = none (hw8/src/scene.cpp:90-97) */
    uint32_t n_primitives;           /* analytic primitives (HW1-HW5); a scene with neither triangles nor primitives is a .txt
                                        scene when camera.fov_y == 0 && camera.fov_x != 0, else a glTF scene */
    const rt_primitive *primitives;
    rt_camera camera;
    float bg_color[3];
    uint32_t n_lights;               /* HW2 only */
    const rt_light *lights;
    float ambient_light[3];          /* HW2 only (AMBIENT_LIGHT) */
    uint32_t build_flags;            /* RT_BUILD_* */
    uint32_t reserved;
} rt_scene_desc;

/* rt_scene_desc.build_flags (glTF scenes with per-vertex normals, i.e. the hw7 / hw8 integrators):
 * RT_BUILD_DEVICE_BVH  build the scene tree on the GPU (binned SAH, device/rt_bvh_build.h: milliseconds instead of the host's replay of
 *                      the reference's builder, hw8/src/include/bvh.h:34-109) and take the LOAD order as the figure order.  Closest hits
 *                      are the same triangles; what changes is everything the reference's figure order decides: which of two hits at
 *                      exactly equal distance wins, the numbering of the emissive triangles (int(u * N) picks a different light for the
 *                      same random number) and the order of the light-pdf additions.  Frames of such a scene follow the reference's
 *                      estimator, not its pixels -- the contract of throughput mode (rt_render_params.sample_streams).
 *                      hw6 scenes (no normals) always get their tree this way: hw6's own tree never was the reference's, the figure
 *                      order is still replayed on the host and the pixels are the reference's (RTAMD_HOST_BVH=1: host-built tree). */
#define RT_BUILD_DEVICE_BVH 1u

#define RT_FLAG_OUT_DEVICE 1u /* out_rgb_linear / out_rgb8 are device pointers on the scene's GPU */
#define RT_FLAG_COUNTERS   2u /* also fill the work counters of rt_stats (slower kernel variant) */
/* Throughput mode only (sample_streams > 1; not the reference's estimator any more, statistical parity only):
 * RT_FLAG_SAMPLE_SEEDS     every camera sample draws from its own engine, seeded with a hash of (pixel, sample index), instead of
 *                          continuing its stream's engine: samples of a pixel are then independent of how they are dealt to streams;
 * RT_FLAG_RUSSIAN_ROULETTE from the third bounce on a path survives a bounce with probability q = clamp(max component of the
 *                          path's accumulated throughput up to and including this bounce, 0.25, 1) and the bounce's factor is divided
 *                          by q (the reference ends paths by depth and its clamp hack only, hw8/src/scene.cpp:85-87,161-163; both
 *                          stay in force).
 * Both are RT_INTEGRATOR_HW8 / HW7 only (hw6 has the streams, not these options). */
#define RT_FLAG_SAMPLE_SEEDS     4u
#define RT_FLAG_RUSSIAN_ROULETTE 8u

typedef struct rt_render_params {
    uint32_t struct_size; /* = sizeof(rt_render_params) */
    int32_t width, height, samples;
    int32_t ray_depth;    /* 0 = reference default (6, hw8/src/include/scene.h:32) */
    int32_t integrator;   /* rt_integrator */
    /* Sharding for multi-GPU: the image is cut into tile_w x tile_h tiles numbered row-major;
     * tile t belongs to shard (t % shard_count).  shard_count <= 1 renders the whole image
     * into a plain W*H*3 row-major buffer; otherwise the output is the compact sequence of
     * this shard's tiles (each tile_h*tile_w*3, border tiles zero-padded). */
    int32_t tile_w, tile_h;
    int32_t shard_index, shard_count;
    uint32_t flags;
    void *stream;         /* hipStream_t to launch on, NULL = default stream */
    /* 0 or 1 = replay mode: one std::minstd_rand per pixel seeded y*W+x draws all of the pixel's samples, as the reference does
     * (hw8/src/sceneio.cpp:389-391) -- the mode every parity claim is made in.
     * K > 1 = throughput mode (RT_INTEGRATOR_HW8 / HW7 / HW6): K independent streams per pixel, stream k seeded
     * y*W+x + k*W*H and drawing samples/K samples (samples must be a multiple of K, W*H*K < 2^31-1); the same estimator
     * with decorrelated sub-streams, so a small frame or shard fills the GPU.  Deterministic, but NOT the reference's pixels:
     * it agrees with replay mode statistically only. */
    int32_t sample_streams;
    int32_t reserved;     /* must be 0 */
} rt_render_params;

typedef struct rt_stats {
    double kernel_ms;       /* HIP-event time of the render kernel(s) on the launch stream */
    double total_ms;        /* host wall time of rt_render */
    uint64_t samples;       /* camera samples rendered by this call */
    uint64_t closest_hit_queries, light_pdf_queries; /* RT_FLAG_COUNTERS */
    uint64_t node_visits, triangle_tests;            /* RT_FLAG_COUNTERS */
    uint32_t launches;
    uint32_t dominant_kernel_launches; /* launches of the dominant kernel (rt_stats.pipeline says which) */
    double dominant_kernel_ms;         /* sum of their HIP-event durations on the launch stream */
    uint32_t pipeline;                 /* rt_pipeline: how the kernels of this render were organised */
    uint32_t reference_exact;          /* hw6 / hw7 / hw8 renders: 1 = every box decision of this render was the reference's own (the walkers'
                                          hits went through the exactness gate, the doubtful ones through the reference-exact walk);
                                          0 = the answer of the walkers' padded boxes stood (RTAMD_NO_EXACT_BOXES, RT_BUILD_DEVICE_BVH,
                                          RTAMD_KERNEL=wavefront|mega, or a tree beyond the gated pipelines' limits): a pixel in ~1e5 may
                                          then differ from the reference's.  hw5: always 1 (its kernel walks the reference's trees with the reference's own box
                                          test).  0 for hw1..hw4 (no boxes: nothing to decide). */
    uint64_t exact_closest_hits, exact_light_sums; /* RT_PIPELINE_PERSISTENT: queries re-walked with the reference's own box
                                                      arithmetic (hw8/src/primitives.cpp:29-53,163-165) because the fast walk's
                                                      answer was not robust against it */
} rt_stats;

/* Kernel organisations of the hw8 / hw7 integrators (the others are always RT_PIPELINE_SINGLE).  Environment RTAMD_KERNEL =
 * persistent (default) | wavefront | mega selects; all three replay the same arithmetic. */
typedef enum rt_pipeline {
    RT_PIPELINE_SINGLE = 0,     /* one launch of a whole-path kernel: render_hw8_kernel ("mega") and render_hw1..hw6_kernel */
    RT_PIPELINE_ROUNDS = 1,     /* per bounce round: wf_traverse_kernel (dominant) + wf_shade_kernel */
    RT_PIPELINE_PERSISTENT = 2  /* pt_persistent_kernel: one launch per frame, per-path dataflow inside each workgroup */
} rt_pipeline;

typedef struct rt_scene rt_scene;

int rt_abi_version(void);
const char *rt_last_error(void);

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out);
void rt_scene_destroy(rt_scene *scene);

/* Number of floats (or bytes for rgb8) rt_render writes for these params. */
size_t rt_output_elems(const rt_render_params *params);

int rt_render(rt_scene *scene, const rt_render_params *params,
              float *out_rgb_linear /* nullable */, uint8_t *out_rgb8 /* nullable */,
              rt_stats *stats /* nullable */);

/* Scatter a compact shard buffer (layout above) into a full W*H*3 host image. */
int rt_unshard(const rt_render_params *params, const void *shard_buf, size_t elem_size,
               void *full_image);

/* ---- resumable renders: advance a frame in slices of samples --------------------------------------------------------------
 * A pixel is the sum of its samples, drawn in order from its one engine, times (float)(1.0 / samples).  An rt_accum keeps that
 * sum and the engine per pixel on the scene's GPU between calls, so a frame can be shown while it converges, continued later
 * ("64 more samples") and checkpointed.  A frame rendered in ANY number of slices is bit for bit the frame of one
 * rt_render call, floats and bytes, and the picture after d samples is bit for bit rt_render(samples = d): the same additions
 * in the same order, the factor applied once at the end.
 *
 * Replay mode only (sample_streams 0 or 1), RT_INTEGRATOR_HW8 / HW7 / HW6 on the pipelines they use by default (both
 * persistent kernels and the round pipeline).  The megakernels (RTAMD_KERNEL=mega, trees beyond the other pipelines' limits),
 * hw1 .. hw5 and throughput mode answer RT_ERR_UNSUPPORTED; there is no fallback.  Several rt_accum may exist per scene, and
 * rt_render on the scene between two slices disturbs none of them; like all calls on one rt_scene they are serialised by the
 * caller.  Destroy every rt_accum before its scene.
 *
 * rt_accum_create   params as for rt_render (width, height, ray_depth, integrator, tile_w/h, shard_index/count, stream);
 *                   params->samples is ignored; flags other than RT_FLAG_COUNTERS -> RT_ERR_UNSUPPORTED.
 * rt_accum_render   every pixel draws n_samples more samples.  rt_stats as rt_render reports them, samples = pixels x
 *                   n_samples.  The total per pixel stays below 2^25 (hw6: 2^24), the sample index field of a path record:
 *                   a slice that would cross it is RT_ERR_LIMIT and leaves the state as it was.  A slice that fails under
 *                   way (launch deadline, HIP error) leaves the rt_accum broken: every later call fails with that first
 *                   error's message.  Cost of slicing: every slice pays its launches, the kernels' init blocks and the exit
 *                   spread of the workgroups, and reads and writes the state once (2 x 24 bytes per pixel slot); the first
 *                   sixteenth of every slice runs under the round-robin deal.  Measured on one MI355X, 1920x1080x256 on
 *                   synth_room_v1, one resolve to the host per slice included: 4 slices of 64 samples take 2.9 % longer than the
 *                   one-shot rt_render (290 ms of kernels per slice), 16 slices of 16 take 15.5 % longer (80 ms per slice);
 *                   DESIGN.md section 4, profiles/r05_sliced_render.txt.
 * rt_accum_samples  samples per pixel so far.
 * rt_accum_resolve  the picture of the state: (float)(1.0 / d) * sum and its tonemapped bytes, in rt_render's output layout
 *                   (sharded or not, padding of border tiles zeroed).  flags: RT_FLAG_OUT_DEVICE.  d == 0 is
 *                   RT_ERR_INVALID_ARG.  The state is only read.
 * rt_accum_state_bytes / rt_accum_save / rt_accum_load   a checkpoint in host memory.  The blob is little-endian: a 128-byte
 *                   header of 32-bit words {magic "RTAC", format version, header bytes, bytes per pixel slot, width, height,
 *                   integrator, effective ray depth, tile_w, tile_h, shard_index, shard_count, pixel slots, samples so far,
 *                   triangle count, light count, FNV-1a hash of the scene's light order, zeros}, then per pixel slot of the
 *                   shard (64 per 8x8 sub-tile, border padding included) {sum r, g, b as float, engine state x}, then per
 *                   pixel slot {the normal distribution's saved value as float, 1 if it is available else 0}: 24 bytes per
 *                   slot.  The engine is the one BEFORE the camera ray of the next sample is drawn.  rt_accum_load rejects
 *                   a blob whose header differs from the rt_accum's in anything but the samples, and a truncated one, with
 *                   RT_ERR_INVALID_ARG and a message naming the field.  rt_accum_state_bytes needs no GPU; 0 = bad params. */
typedef struct rt_accum rt_accum;
int rt_accum_create(rt_scene *scene, const rt_render_params *params, rt_accum **out);
int rt_accum_render(rt_accum *accum, int32_t n_samples, rt_stats *stats /* nullable */);
int rt_accum_samples(const rt_accum *accum);
int rt_accum_resolve(rt_accum *accum, uint32_t flags, float *out_rgb_linear /* nullable */, uint8_t *out_rgb8 /* nullable */);
size_t rt_accum_state_bytes(const rt_render_params *params);
int rt_accum_save(rt_accum *accum, void *blob, size_t capacity);
int rt_accum_load(rt_accum *accum, const void *blob, size_t size);
void rt_accum_destroy(rt_accum *accum);

/* ---- several GPUs in one process ---------------------------------------------------------------------------------------
 * The reference shards nothing (one OpenMP loop over the pixels, hw8/src/sceneio.cpp:387-396, driven from main,
 * hw8/src/main.cpp:7-18); pixels are independent and seeded by their global index, so the frame's 32x32 tiles are dealt
 * round-robin to the devices, every device renders its shard from its own host thread, and ONE exchange step brings the shards
 * to the first device (hipMemcpyPeerAsync over xGMI) where the tiles are scattered into the frame.  The result is bit-identical
 * to the one-device render.  `devices` = HIP device indices (NULL = 0 .. n_devices-1; an index may repeat, which renders two
 * shards on one GPU — used by the tests on a one-GPU machine).  rt_multi_render takes the params of an UNSHARDED frame
 * (shard_count 0 or 1); out pointers are host memory, or memory on the first device with RT_FLAG_OUT_DEVICE; stats are summed
 * over the devices except kernel_ms / dominant_kernel_ms (the slowest device: they render side by side) and total_ms (wall). */
typedef struct rt_multi rt_multi;
int rt_device_count(void);
int rt_multi_create(const rt_scene_desc *desc, const int *devices, int n_devices, rt_multi **out);
int rt_multi_render(rt_multi *multi, const rt_render_params *params, float *out_rgb_linear /* nullable */, uint8_t *out_rgb8 /* nullable */,
                    rt_stats *stats /* nullable */);
void rt_multi_destroy(rt_multi *multi);

/* ---- resumable renders on several GPUs ---------------------------------------------------------------------------------
 * rt_multi_* and rt_accum_* composed: one sharded rt_accum per device entry of the rt_multi (shard i of N, 32x32 tiles dealt
 * round-robin, on that entry's own stream), advanced side by side, one host thread per device.  The frame after any slicing
 * on any number of devices is bit for bit the one rt_render call's, and the picture after d samples is rt_render(samples = d).
 * Like everything in rt_multi the path has so far run with repeated entries of ONE physical GPU only (the peer copies are
 * then copies within the device); two physical devices were never involved.
 *
 * rt_multi_accum_create   params of the UNSHARDED frame, as for rt_multi_render (shard_count 0 or 1, square tiles, default 32;
 *                         samples ignored).  What rt_accum_create refuses is refused here with its code and its reason:
 *                         hw1 .. hw5, throughput mode, the megakernels and flags other than RT_FLAG_COUNTERS are
 *                         RT_ERR_UNSUPPORTED.  With more entries than tiles some shards are empty.  Several rt_multi_accum may
 *                         live on one rt_multi, rt_multi_render between two slices disturbs none of them; destroy them before
 *                         the rt_multi.  Calls on one rt_multi and its rt_multi_accums are serialised by the caller.
 * rt_multi_accum_render   every device draws n_samples more samples for the pixels of its shard.  Whatever can be refused is
 *                         refused before any device launches and leaves the state as it was; that includes the sample index
 *                         limit (the smallest of the devices' limits, RT_ERR_LIMIT).  A device that fails under way leaves the
 *                         whole object broken: every later call fails with that first message.  rt_stats as rt_multi_render
 *                         sums them, samples = W*H*n_samples, reference_exact = the AND over the shards that have pixels,
 *                         pipeline = that of a shard that has pixels.
 * rt_multi_accum_samples  samples per pixel so far.
 * rt_multi_accum_resolve  every device resolves its shard on the device; the shards go through rt_multi_render's exchange (push to
 *                         the first device, tiles scattered into the frame there).  Outputs are host memory, or with
 *                         RT_FLAG_OUT_DEVICE memory on the first device.  d == 0 is RT_ERR_INVALID_ARG.  The state is only read.
 * rt_multi_accum_save / rt_multi_accum_load   the PORTABLE checkpoint: the blob is byte for byte the blob an unsharded
 *                         single-device rt_accum of the same frame writes after the same samples -- the header of shard 0 of 1
 *                         in 8x8 tiles with ceil(W/8)*ceil(H/8)*64 pixel slots, then the two per-slot arrays in the order of
 *                         the image's 8x8 sub-tiles, row-major.  Its size is rt_accum_state_bytes(the unsharded params): there
 *                         is no size function of its own.  So a checkpoint saved on N devices loads on M devices for any M,
 *                         one included, and into a plain unsharded rt_accum, and an unsharded rt_accum's blob loads here; the
 *                         continued frame is bit for bit the one-shot rt_render.  Save: every device pushes its shard's state
 *                         to the first device, which regroups the shards into that order and copies the blob to the host once;
 *                         load is the reverse.  rt_multi_accum_load checks every header field but the samples against the frame
 *                         and the samples against the limit; a mismatch or a truncated blob is RT_ERR_INVALID_ARG with a
 *                         message naming the field and leaves the state as it was.
 * Measured on one MI355X (profiles/r10_multi_accum.txt): the 1920x1080x256 frame in 4 slices of 64 with a resolve
 * to the host per slice takes 1,124 ms on one device entry (rt_accum: 1,131 - 1,141 ms) and 1,246 ms as two shards on that one GPU;
 * save / load of its 49.8 MB checkpoint 14 / 25 ms through the Python binding. */
typedef struct rt_multi_accum rt_multi_accum;
int rt_multi_accum_create(rt_multi *multi, const rt_render_params *params, rt_multi_accum **out);
int rt_multi_accum_render(rt_multi_accum *accum, int32_t n_samples, rt_stats *stats /* nullable */);
int rt_multi_accum_samples(const rt_multi_accum *accum);
int rt_multi_accum_resolve(rt_multi_accum *accum, uint32_t flags, float *out_rgb_linear /* nullable */, uint8_t *out_rgb8 /* nullable */);
int rt_multi_accum_save(rt_multi_accum *accum, void *blob, size_t capacity);
int rt_multi_accum_load(rt_multi_accum *accum, const void *blob, size_t size);
void rt_multi_accum_destroy(rt_multi_accum *accum);

/* ---- noise monitor of a resumable render: per-pixel error of the picture, so that a caller can stop at a target -------------------
 * An rt_noise watches an rt_accum and only READS its state between slices: no render kernel knows of it, no pixel draws other
 * samples because of it, and every picture stays bit for bit rt_render(samples = d).  What it measures is the noise of the
 * picture's luminance, by batch means: a pixel's samples come in order from its one engine, so the sums of consecutive slices
 * are disjoint batches of one stream, and the scatter of the batch means gives the variance per sample.  One small kernel per
 * slice over state that is already on the device.
 *
 * Arithmetic (float32, one rounding per operation; tests/noise_model.py restates it in numpy bit for bit).  Per pixel slot three
 * floats y0, yp, m2; per monitor B batches and N samples observed.  Y(r, g, b) = ((0.2126f*r) + (0.7152f*g)) + (0.0722f*b) of the
 * slot's sum in the rt_accum.
 *   create / reset  y0 = yp = Y(sum), m2 = 0, B = N = 0.
 *   update          n = samples drawn since the last update / create / reset; yc = Y(sum); mb = (yc - yp) / n;
 *                   mu0 = N == 0 ? mb : (yp - y0) / N;  mu1 = (yc - y0) / (N + n);  m2 = m2 + n * ((mb - mu0) * (mb - mu1));
 *                   yp = yc; then B += 1, N += n  (West's weighted incremental variance: batches of unequal length are fine).
 *   estimate        d = rt_accum_samples; s2 = (m2 < 0 ? 0 : m2) / (B - 1) (a NaN stays a NaN); se2 = s2 / d; se = sqrt(se2): the
 *                   standard error of the pixel's luminance in the picture of d samples; its mean luminance is yc / d.
 * Padding slots of border tiles take part in nothing.  Per 8x8 sub-tile (one wave) the kernel sums se2 and the mean luminance over
 * the pixels where both are finite, in a fixed order without float atomics, and counts them and the non-finite ones; the host adds
 * those entries in double in the order of the frame's sub-tiles, row-major.  Two runs, and any sharding, give the same bits.
 *
 * rt_noise_create    snapshots the sums as they are (a monitor may be attached at any time; several may watch one rt_accum).
 * rt_noise_update    after rt_accum_render: the samples drawn since the last update / create / reset are one batch.
 *                    RT_ERR_INVALID_ARG, with the cause in the message, when no sample was drawn since, when the rt_accum is
 *                    broken, and when rt_accum_load has replaced the state since the last snapshot (call rt_noise_reset).
 * rt_noise_reset     snapshot again, batches = 0.
 * rt_noise_estimate  needs 2 batches (else RT_ERR_INVALID_ARG).  out_se: one float per pixel in rt_accum_resolve's layout with one
 *                    channel instead of three (W*H row-major, or the compact shard tiles, padding zeroed), host memory or with
 *                    RT_FLAG_OUT_DEVICE memory on the scene's GPU; a pixel with a non-finite estimate holds that NaN / inf.
 *                    summary->struct_size must be sizeof(rt_noise_summary).  The monitor's and the rt_accum's state are only read.
 * rt_noise_destroy   before its rt_accum.
 * The statistics are NOT part of a checkpoint (the blob of rt_accum_save is as it was): a render continued from a checkpoint starts
 * its batches afresh, at the state it loaded.
 *
 * Measured on one MI355X (profiles/r17_noise_monitor.txt): on the 1920x1080x256 frame in 16 slices of 16 an update and
 * an estimate (summary only) per slice take 0.23 - 0.27 ms together, launches, copy and synchronisations included, next to 72 ms of render
 * kernels per slice; on the sphere scene at 96x64 the estimated rms_error is 1.7 % (d = 64) and 1.1 % (d = 256) above the actual RMS error.
 *
 * What the figures do not see: correlation between pixels, the bias of the reference's clamp, and that B - 1 degrees of freedom make
 * one pixel's value rough -- the frame figures average thousands of pixels.
 *
 * rt_multi_noise_*   the same on an rt_multi_accum: one monitor per non-empty shard, on that shard's device and stream; the map is
 *                    scattered into the W*H frame and the sub-tile entries are put into the frame's order on the host, so the
 *                    summary equals the unsharded single-device monitor's of the same slicing in every field, bit for bit.
 *                    rt_multi_accum_load ends the batches as rt_accum_load does.  flags must be 0: the outputs are host memory. */
typedef struct rt_noise_summary {
    uint32_t struct_size;        /* in: sizeof(rt_noise_summary) */
    int32_t  batches;            /* slices observed since create / reset */
    int32_t  samples_observed;   /* samples per pixel in those slices */
    int32_t  samples_total;      /* rt_accum_samples: the d of the picture */
    uint64_t pixels;             /* pixels of the frame / shard with a finite estimate */
    uint64_t nonfinite_pixels;   /* pixels whose luminance sum or estimate is NaN / inf: counted here, left out of every sum below */
    double   mean_luminance;     /* mean over `pixels` of Y(sum) / d */
    double   rms_error;          /* sqrt(mean over `pixels` of se^2): estimated RMS error of the picture's luminance */
    double   noise;              /* rms_error / mean_luminance, 0 when mean_luminance is 0 */
    double   worst_tile_noise;   /* sqrt(max over 8x8 sub-tiles of their mean se^2) / mean_luminance */
} rt_noise_summary;

typedef struct rt_noise rt_noise;
int  rt_noise_create(rt_accum *accum, rt_noise **out);
int  rt_noise_update(rt_noise *n);
int  rt_noise_reset(rt_noise *n);
int  rt_noise_batches(const rt_noise *n);
int  rt_noise_estimate(rt_noise *n, uint32_t flags, float *out_se /* nullable */, rt_noise_summary *summary /* nullable */);
void rt_noise_destroy(rt_noise *n);

typedef struct rt_multi_noise rt_multi_noise;
int  rt_multi_noise_create(rt_multi_accum *accum, rt_multi_noise **out);
int  rt_multi_noise_update(rt_multi_noise *n);
int  rt_multi_noise_reset(rt_multi_noise *n);
int  rt_multi_noise_batches(const rt_multi_noise *n);
int  rt_multi_noise_estimate(rt_multi_noise *n, uint32_t flags, float *out_se /* nullable */, rt_noise_summary *summary /* nullable */);
void rt_multi_noise_destroy(rt_multi_noise *n);

/* ---- batched ray queries: below the render loop ----------------------------------------------------------------------------
 * The two functions the render loop spends its time in, for rays of the caller's own (an integrator, a picker, a visibility or
 * baking pass, a debugger): the closest hit, BVH::intersect (hw8/src/include/bvh.h:111-142) with Figure::intersectAsTriangle's
 * attributes (hw8/src/primitives.cpp:85-125), and the light pdf, FiguresMix::pdf (hw8/src/include/distributions.h:122-124: the
 * all-hits sum getTotalPdf, :148-165, divided by the light count).  Both answer bit for bit what the reference computes, over the
 * trees and with the walkers the renders use (device/rt_query.h).  ABI version 6 still: the additions change nothing that existed.
 *
 * Scenes created for hw8 / hw7 are served (hw6 and .txt scenes: RT_ERR_UNSUPPORTED).  The light pdf is hw8's, with the shading
 * normal (hw7's own uses the geometric normal, hw7/src/include/distributions.h:140-145: not offered); on a scene without lights
 * rt_query_light_pdf is RT_ERR_INVALID_ARG.  n == 0 is RT_OK and launches nothing.
 *
 * rt_ray   d as the reference takes it: any length, t is in units of d (the reference reports hits with 0 < t < 1e4).
 * rt_hit   64 bytes.  triangle: index in LOAD order (the order of rt_scene_desc's arrays), 0xFFFFFFFF = miss, and then every other
 *          field but flags is 0.  ng: the geometric normal, normalised, flipped against the ray when it hits the back
 *          (RT_HIT_INSIDE); texcoord, ns (normalised, flipped likewise) and tangent (xyz normalised, w of the first vertex) are
 *          interpolated as the shader does.  flags: RT_HIT_INSIDE, RT_HIT_EXACT_WALK (the answer came from the reference-order walk,
 *          not from the fast walk: informative, it changes no other field), RT_HIT_INVALID_RAY.
 * Invalid rays: a ray with a NaN or an infinity in o or d, or with d == 0, is never walked; it is answered as a miss with
 *          RT_HIT_INVALID_RAY (light pdf: 0) and counted in rt_query_stats.invalid_rays.
 * flags    RT_QUERY_DEVICE_POINTERS: rays and out are device memory on the scene's GPU (out of rt_query_closest 16-byte aligned),
 *          read and written in place; the work is ordered on the null stream and has finished when the call returns.
 *          RT_QUERY_REFERENCE_WALK: every valid ray takes the reference-order walk, one lane per ray -- the referee of the fast path;
 *          the answers are the same bits.
 * Memory   rays are processed in chunks of 262,144, so the staging (29 MB per scene, allocated by the first query, freed with the
 *          scene; 57 MB once a surface query or a guide pass has run) does not grow with n.  Queries are serialised with the scene's other calls by the caller, like every call; they
 *          only read the scene and disturb no rt_accum.
 * stats    struct_size in: sizeof(rt_query_stats).  exact_walks: valid rays answered by the reference-order walk -- those the gate
 *          (device/rt_exact.h) sent there, and those outside what the gate was derived for: an origin coordinate beyond the largest
 *          |coordinate| of scene and camera, a direction with a zero component or a length outside [1/16, 16], all rays under
 *          RT_QUERY_REFERENCE_WALK.  kernel_ms: HIP-event time of the kernels; total_ms: host wall time of the call.
 *          reference_exact: 1 = every answer of this call is the reference's own.  0 on RT_BUILD_DEVICE_BVH scenes and under
 *          RTAMD_NO_EXACT_BOXES: the answers are then the closest triangles of the padded boxes' walk, with the tie rule (equal t: the
 *          lowest index) in load order on RT_BUILD_DEVICE_BVH scenes, and the light sums add in that order. */
typedef struct rt_ray { float o[3]; float d[3]; } rt_ray;
typedef struct rt_hit {
    float t; uint32_t triangle;
    float ng[3]; float texcoord[2]; float ns[3]; float tangent[4];
    uint32_t flags;
    uint32_t reserved;
} rt_hit;
#define RT_HIT_INSIDE      1u
#define RT_HIT_EXACT_WALK  2u
#define RT_HIT_INVALID_RAY 4u
typedef struct rt_query_stats {
    uint32_t struct_size; uint32_t reference_exact;
    uint64_t rays, exact_walks, invalid_rays;
    double kernel_ms, total_ms;
    uint32_t launches, reserved;
} rt_query_stats;
#define RT_QUERY_DEVICE_POINTERS 1u
#define RT_QUERY_REFERENCE_WALK  2u
int rt_query_closest(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, rt_hit *out, rt_query_stats *stats /* nullable */);
int rt_query_light_pdf(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, float *out, rt_query_stats *stats /* nullable */);

/* ---- occlusion queries: is anything in front of tmax? ------------------------------------------------------------------------
 * The yes/no question of a visibility pass (shadow rays, ambient occlusion and light-map baking, line of sight, portal culling):
 * bit 0 of out[i] (RT_OCCLUSION_OCCLUDED) is set exactly when the reference's BVH::intersect reports a hit for ray i with
 * t < tmax[i] -- a strict float32 compare, t in units of d as above.  The walk ends at the first triangle below the bound instead
 * of looking for the closest, interpolates nothing and writes one byte per ray; the gate (device/rt_query.h) asks only whether the
 * reference, too, ends with a hit below the bound, not which one.  ABI version 6 still.
 *
 * tmax     n floats, nullable.  NULL, or tmax[i] == +inf, asks "does the ray hit anything": the answer is rt_query_closest's
 *          triangle != 0xFFFFFFFF.  A segment p -> q is the ray o = p, d = q - p with tmax = 1, or a little less to spare the far
 *          end; segments whose |d| lies outside [1/16, 16] take the reference-order walk, by the rule of the fast list above (scale
 *          d and tmax together to stay on the fast path).  tmax[i] <= 0 (-0 and -inf too) is valid: the answer is 0 and the ray is
 *          not walked.  A NaN tmax[i] makes ray i invalid.
 * out      one byte per ray: RT_OCCLUSION_OCCLUDED, RT_OCCLUSION_EXACT_WALK (informative, as RT_HIT_EXACT_WALK) or, for an invalid
 *          ray (the rule of rt_query_closest, or a NaN bound), RT_OCCLUSION_INVALID_RAY alone; invalid rays are counted in
 *          rt_query_stats.invalid_rays and never walked.
 * Scenes, refusals, n == 0, the chunks of 262,144 (RTAMD_QUERY_CHUNK), both flags and rt_query_stats are rt_query_closest's.  With
 *          RT_QUERY_DEVICE_POINTERS rays, tmax and out are device memory; out is byte-addressed with no alignment demand, tmax is
 *          4-byte aligned.  On scenes with reference_exact 0 the answer is "the padded boxes' walk has its closest hit below tmax":
 *          rt_query_closest's t on the same scene, compared with tmax.
 * Memory   with host arrays the first call grows the scene's staging by 4 + 1 bytes per ray of a chunk (1.3 MB).
 * Measured on one MI355X, synth_room_v1, 2,073,600 rays per call, kernel time (profiles/r24_occlusion.txt): 1,049 / 1,451 / 811 Mrays/s
 *          on the camera rays of the 1080p frame with tmax NULL / half / twice the closest t, 1,271 / 1,665 / 1,248 on their bounce rays,
 *          where rt_query_closest runs at 509 and 809; 2 - 32 of the rays take the reference-order walk (rt_query_closest: 61 and 27), and
 *          the bytes equal the forced reference walk's on all six sets.  Host arrays: 3.3 - 4.8 ms a call against 12.1 - 14.0 ms. */
#define RT_OCCLUSION_OCCLUDED    1u
#define RT_OCCLUSION_EXACT_WALK  2u
#define RT_OCCLUSION_INVALID_RAY 4u
int rt_query_occluded(rt_scene *scene, const rt_ray *rays, const float *tmax /* nullable: n floats */, size_t n,
                      uint32_t flags, uint8_t *out /* n bytes */, rt_query_stats *stats /* nullable */);

/* ---- the first-hit layer: surface, environment, camera rays, guide images ---------------------------------------------------
 * What a caller with a render loop of its own needs next to the closest hit, each the reference's own arithmetic bit for bit and
 * with the device functions the renders use (device/rt_query_surface.h).  Same scenes, same refusals, same chunks of 262,144 and
 * the same staging as the two queries above; flags takes RT_QUERY_DEVICE_POINTERS only.  ABI version 6 still.
 *
 * rt_query_surface      what Scene::getColor knows about a hit before it samples a direction (hw8/src/scene.cpp:99-149), with hw8's
 *          material rule (textures, normal map, roughness floor 0.08; hw7's own is not offered).  In: the rt_hit records that
 *          rt_query_closest wrote, or records of the caller's own: only triangle (LOAD order), texcoord, ns and tangent (xyz, w) are
 *          read, the ray is not needed.  Out, 64 bytes per hit: color = the base-colour texture tap (sRGB decoded) or 1,1,1;
 *          alpha = max(0.08, roughnessFactor * mr.y)^2; emission = emissiveFactor (* the emissive tap); metallic = mr.z of the
 *          metallic-roughness tap (1 without one); sn = the shading normal after the normal map; material = the material's index;
 *          base_color, base_metallic = the material's factors (the other two arguments of the reference's brdf).
 *          A miss (triangle 0xFFFFFFFF) answers zeros with material = 0xFFFFFFFF.  So does a record with triangle >= n_triangles
 *          or with a NaN or an infinity in texcoord, ns or tangent; those are counted in rt_query_stats.invalid_rays and lead to
 *          no read of the scene.  exact_walks is 0.  With RT_QUERY_DEVICE_POINTERS both arrays are 16-byte aligned.
 *          The first call grows the scene's staging to 57 MB and makes a table of 4 bytes per triangle; neither is part of
 *          rt_scene_info.device_bytes, both go with the scene.
 * rt_query_environment  what a ray that misses sees (scene.cpp:90-97) in its direction d as given: the background colour, or the
 *          equirect lookup of the environment map (a d.y beyond +-1 gives the reference's NaN).  n x 3 floats.  Invalid rays (the
 *          rule of rt_query_closest) answer 0,0,0 and are counted.
 * rt_camera_rays        Scene::getCameraRay (scene.cpp:179-186) for a frame of width x height and n points (nx, ny) of its image
 *          plane in pixel units: the renderer's sample is nx = x + u1, ny = y + u2 with its two random draws, a pixel's centre
 *          x + 0.5, y + 0.5.  width or height < 1 is RT_ERR_INVALID_ARG, and so is a NaN or an infinity in a host xy array; from a
 *          device array such a point comes out as a NaN direction, which every query then answers as an invalid ray.
 * rt_render_guides      the guide images a denoiser takes next to a noisy frame, row-major, row 0 first, every plane nullable: per
 *          pixel the camera ray through its centre, rt_query_closest, then on a hit albedo = base_color * color (one float product
 *          per channel), normal = sn, depth = t and the surface's emission, on a miss albedo = rt_query_environment's answer and
 *          0 elsewhere.  No plane depends on a random number, a sample count or the pipeline.  The rays are made, walked and
 *          shaded on the device chunk by chunk, so the memory is the staging whatever the frame's size; stats are those of the
 *          closest-hit query over width * height rays, with every launch counted.  One GPU, unsharded frames. */
typedef struct rt_surface {
    float color[3];      float alpha;
    float emission[3];   float metallic;
    float sn[3];         uint32_t material;
    float base_color[3]; float base_metallic;
} rt_surface;
int rt_query_surface(rt_scene *scene, const rt_hit *hits, size_t n, uint32_t flags, rt_surface *out, rt_query_stats *stats /* nullable */);
int rt_query_environment(rt_scene *scene, const rt_ray *rays, size_t n, uint32_t flags, float *out_rgb /* n*3 */, rt_query_stats *stats /* nullable */);
int rt_camera_rays(rt_scene *scene, int32_t width, int32_t height, const float *xy /* n*2 */, size_t n, uint32_t flags, rt_ray *out);
int rt_render_guides(rt_scene *scene, int32_t width, int32_t height, uint32_t flags,
                     float *albedo /* W*H*3 */, float *normal /* W*H*3 */, float *depth /* W*H */, float *emission /* W*H*3 */,
                     rt_query_stats *stats /* nullable */);

/* ---- the bounce step: scatter queries and rt_trace_paths ---------------------------------------------------------------------
 * What Scene::getColor DECIDES at a hit (hw8/src/scene.cpp:151-164), for a caller with an integrator of its own -- a light-map or
 * probe baker, another camera model, a path debugger, next-event estimation: Mix::sample, MaterialModel::brdf, Mix::pdf, the weight
 * and the two early returns, with the device functions the renders use (device/rt_query_scatter.h) and bit for bit the reference's
 * answers.  With the queries above, a frame folded from public calls only -- camera ray, closest, surface / environment, scatter,
 * repeated -- is rt_render's frame word for word.  Same scenes, refusals, chunks (RTAMD_QUERY_CHUNK) and n == 0 as
 * rt_query_surface.  Offered: hw8's rules only.  Not offered: hw7's brdf and light pdf, the throughput-mode options (sample streams,
 * Russian roulette).  ABI version 6 still.
 *
 * rt_rng   the engine of a path as a record: x the state of std::minstd_rand, saved / has_saved the second value of
 *          std::normal_distribution<float> -- what an rt_accum checkpoint stores per pixel slot.  rt_rng_seed is minstd_rand::seed
 *          (seed mod (2^31-1), 0 -> 1, no saved value), rt_rng_uniform one draw of uniform_real_distribution<float>(0, 1) on it
 *          (float(x' - 1) * 2^-31, kept below 1); both run on the host and need no GPU: a caller replays getPixel's two jitter draws
 *          with them before rt_camera_rays.  A state with x == 0 or x >= 2147483647 is one the engine never has, and the normal
 *          distribution's rejection loop would never leave it: host arrays are checked before any launch (RT_ERR_INVALID_ARG, the
 *          message names the record), a record from device memory is marked RT_SCATTER_INVALID and never sampled.  A record comes
 *          back with saved = 0 whenever has_saved is 0; reserved is handed through.
 *
 * rt_query_scatter   one bounce, per record i from rays[i] (the ray that hit), hits[i] (t and ng are read, triangle only compared
 *          with 0xFFFFFFFF), surfaces[i] (every field but material, which is only compared with 0xFFFFFFFF) and rng[i].  No index of
 *          a caller's record is dereferenced; the scene is read at the light the engine picks and in the light tree, nowhere else.
 *            x = o + t*d;  out.o = x + eps*ng, eps = (float)1e-4L                                           scene.cpp:104, :151
 *            component = (int)(u01 * (2 + (lights ? 1 : 0)));  out.d = cosine (0), vndf (1) or light (2) sample   distributions.h:256-265
 *            brdf = MaterialModel(base_metallic, base_color).brdf(out.d, -d, sn, color, metallic, alpha)     :153
 *            every brdf channel < eps: RT_SCATTER_END_BRDF                                                    :154-156
 *            pdf = (cosine pdf + vndf pdf (+ light pdf of (out.o, out.d))) / components                        distributions.h:267-279
 *            weight = (float)(1. / pdf * fabs(out.d . sn)) * brdf                                             :159
 *            a weight channel > 6 or a NaN: RT_SCATTER_END_CLAMP                                              :161-163
 *          A path that ends returns the surface's emission; one that goes on has L = emission + weight * L(out.o, out.d)  (:164).
 *          NaNs in a record flow through the arithmetic as in the reference and normally end in RT_SCATTER_END_CLAMP.  The engine is
 *          written back after its draws, for an ended record too: it has drawn.  A record is judged in this order: no surface
 *          (RT_SCATTER_NO_SURFACE), then invalid (RT_SCATTER_INVALID); both answer zeros and leave the engine as it was.
 *          Launches per chunk: the sample kernel, on a scene with lights rt_query_light_pdf's launches over (out.o, out.d) -- records
 *          that need no walk ride along as invalid rays, which no walker touches and invalid_rays does not count --, the finish kernel.
 *          flags: RT_QUERY_DEVICE_POINTERS (all five arrays are device memory; rt_hit, rt_surface, rt_rng and rt_scatter 16-byte
 *          aligned, rays 4-byte) and RT_QUERY_REFERENCE_WALK (handed to the light walk; the same bits).  stats.exact_walks: light walks
 *          answered by the reference-order walk; invalid_rays: RT_SCATTER_INVALID records.
 * rt_query_bsdf      the two evaluations for directions of the caller's own: out_brdf = brdf(dirs[i], -d, sn, ...), out_pdf = the full
 *          Mix::pdf of dirs[i] at out.o; the pdf is always evaluated.  It is rt_query_scatter's finish kernel: on a scatter's own d
 *          both equal the scatter's words wherever it evaluated them.  No-surface and invalid records (also: a non-finite or zero
 *          dirs[i]) answer zeros.  With RT_QUERY_DEVICE_POINTERS dirs, out_brdf and out_pdf are 4-byte aligned.
 * rt_trace_paths     Scene::getColor(ray, ray_depth) for rays and engines of the caller's own.  Per bounce, on the device, chunk by
 *          chunk: rt_query_closest; a miss ends the path with rt_query_environment's colour; rt_query_surface; rt_query_scatter; an
 *          RT_SCATTER_END_* ends it with the emission; else e[b] = emission, m[b] = weight and the ray becomes (o, d).  After
 *          ray_depth bounces (0 = 6; above 16: RT_ERR_LIMIT, as rt_render) the tail is 0; then L = e[b] + m[b] * L backwards, two
 *          roundings per channel.  Radiance and engine afterwards equal that composition of the public calls bit for bit, hence
 *          rt_render's sample.  An invalid ray answers 0, 0, 0 with its engine untouched and is counted.  Ended paths ride along as
 *          invalid rays until the depth is spent: nothing is compacted.  The per-bounce stack is 24 bytes x depth + 16 bytes per
 *          path of a chunk (37 MB at depth 6), kept by the scene like the staging and not part of rt_scene_info.device_bytes.
 *          stats: rays = n, exact_walks summed over all walks of the call, every launch counted.
 * Memory   the first of these calls grows the scene's staging to 85 MB.
 * Measured on one MI355X, synth_room_v1, the 2,073,600 camera-ray records of the 1080p frame (profiles/r28_scatter_paths.txt, DESIGN.md
 *          section 4): rt_query_scatter 3.37 ms of kernels = 615 Mrecords/s with device pointers (the call 3.6 ms), of which the sample
 *          kernel is 0.19 ms, the finish kernel 0.10 ms and the light walk 2.98 ms; through host arrays the call takes 19.8 ms.
 *          rt_trace_paths at depth 6: 44.5 ms = 46.6 Mpaths/s, 8.6 x rt_render(samples = 1) of the same frame (5.2 ms): 528 launches,
 *          records through memory, and what no compaction costs -- 27.8 % of the ray slots over the six bounces (48.2 % at the last)
 *          belong to paths already ended.  Sample kernel: 108 VGPRs, no scratch. */
typedef struct rt_rng { uint32_t x; float saved; uint32_t has_saved; uint32_t reserved; } rt_rng;   /* 16 bytes */
void rt_rng_seed(rt_rng *r, uint32_t seed);
extern float rt_rng_uniform(rt_rng *r);
typedef struct rt_scatter {           /* 64 bytes */
    float o[3]; float pdf;            /* x + eps*ng; Mix::pdf of d */
    float d[3]; uint32_t flags;       /* the sampled direction; RT_SCATTER_* */
    float weight[3]; uint32_t component; /* mult of scene.cpp:159; 0 cosine, 1 vndf, 2 lights */
    float brdf[3]; uint32_t reserved;
} rt_scatter;
#define RT_SCATTER_END_BRDF   1u  /* every brdf channel < eps (:154): the path returns the surface's emission; pdf and weight are 0, no light walk */
#define RT_SCATTER_END_CLAMP  2u  /* a weight channel > 6 or NaN (:161): likewise; weight 0, pdf and brdf as computed */
#define RT_SCATTER_NO_SURFACE 4u  /* hit.triangle or surface.material is 0xFFFFFFFF: zeros, engine untouched, not counted */
#define RT_SCATTER_INVALID    8u  /* invalid ray (rt_query_closest's rule), non-finite t or ng, bad engine: zeros, engine untouched, counted in invalid_rays */
int rt_query_scatter(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, rt_rng *rng /* in and out */,
                     size_t n, uint32_t flags, rt_scatter *out, rt_query_stats *stats /* nullable */);
int rt_query_bsdf(rt_scene *scene, const rt_ray *rays, const rt_hit *hits, const rt_surface *surfaces, const float *dirs /* n*3 */,
                  size_t n, uint32_t flags, float *out_brdf /* n*3 */, float *out_pdf /* n */, rt_query_stats *stats /* nullable */);
int rt_trace_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng /* in and out */, size_t n, int32_t ray_depth,
                   uint32_t flags, float *out_rgb /* n*3 */, rt_query_stats *stats /* nullable */);

/* ---- the baker: irradiance and SH probes at points of the caller's, paths restarted in place ----------------------------------
 * The first caller of the query layer above, kept a composition of its public calls: per sample a ray from the engine (rt_bake_rays),
 * rt_trace_paths over it, and a float32 sum.  Same scenes, refusals and chunks (RTAMD_QUERY_CHUNK) as rt_trace_paths; hw8's rules
 * only.  New on the device are the ray maker and the advance / fold / accumulate / restart step (device/rt_bake.h); the walks are
 * the launches of the queries above, untouched.  ABI version 6 still.
 *
 * rt_bake_rays   the rt_camera_rays of a baker: one ray per record from the record's engine, which advances in place.
 *            RT_BAKE_IRRADIANCE:  o = p + eps*n, eps = (float)1e-4L, n used as given (a unit normal: rt_hit.ng, rt_surface.sn);
 *                                 d = the cosine-distributed direction around n that rt_query_scatter's component 0 draws.
 *            RT_BAKE_SH9:         o = p, n is not read;  d = normalize(a, b, c) of three normal draws: a uniform direction.
 *          A record with a NaN or an infinity in p, (irradiance) a NaN or an infinity in n or n == 0, or an engine state outside
 *          1 .. 2^31-2 is invalid: it gets an invalid ray (o = 0, d = NaN), keeps its engine and is counted in invalid_rays.  Host
 *          engine arrays are checked before any launch, as rt_query_scatter's.  flags: RT_QUERY_DEVICE_POINTERS (points and rays
 *          4-byte aligned, rt_rng 16-byte).
 * rt_bake        per point i and stream k (params.streams = K, 1 .. 64, 0 = 1; samples >= 1 and a multiple of K) the engine
 *          rng[i*K+k] draws q = samples / K samples back to back: rt_bake_rays, rt_trace_paths(ray, engine, ray_depth), then
 *            irradiance:  acc_k = acc_k + L                           per channel, in sample order
 *            SH9:         acc_k[m][c] = acc_k[m][c] + (Y_m(d) * L[c])    d the sample's first direction, and
 *                         Y_0 = 0.282095f, Y_1 = 0.488603f*y, Y_2 = 0.488603f*z, Y_3 = 0.488603f*x, Y_4 = 1.092548f*(x*y),
 *                         Y_5 = 1.092548f*(y*z), Y_6 = 0.315392f*((3.0f*(z*z)) - 1.0f), Y_7 = 1.092548f*(x*z),
 *                         Y_8 = 0.546274f*((x*x) - (y*y))
 *          in float32 with one rounding per operation.  out = scale * (((acc_0 + acc_1) + acc_2) ...), scale =
 *          (float)(pi / (double)samples) for the irradiance (3 floats per point), (float)(4 * pi / (double)samples) for SH9 (27
 *          floats per point, [m][c]).  Streams exist so that a few thousand probes with thousands of samples fill the GPU; the
 *          caller seeds the engines (rt_rng_seed) and may carry them into a later call.  A point with an invalid record (the rule
 *          of rt_bake_rays, over all K of its engines) answers zeros, leaves all its engines untouched and is counted once in
 *          invalid_points.  ray_depth: 0 = 6, above 16 RT_ERR_LIMIT; streams > 64 or n_points * streams >= 2^31: RT_ERR_LIMIT; a bad
 *          mode, flags, struct_size or a non-zero reserved word: RT_ERR_INVALID_ARG, the message names the field.
 * Scheduling  a slot (i, k) owns its engine, so it runs its q paths back to back: in the round (closest hit, surface, scatter,
 *          light walk, advance) in which its path ends -- a miss, an RT_SCATTER_END_*, or ray_depth bounces spent -- the advance
 *          step folds L = e[b] + m[b]*L, accumulates, makes the slot's next ray from the engine as the scatter left it and resets the
 *          path; a slot without a sample left parks as an invalid ray.  The host reads a live-slot count after every round and
 *          stops at 0.  No compaction, no sort, no change to a walker.  RT_BAKE_LOCKSTEP: every slot starts sample j in the same
 *          round and every sample takes ray_depth rounds -- the plain composition, the referee: outputs and engines are the same
 *          bits, since a slot's samples come from its one engine in the same order whatever the schedule.
 * flags    RT_QUERY_DEVICE_POINTERS (points and out 4-byte aligned, rt_rng 16-byte), RT_QUERY_REFERENCE_WALK, RT_BAKE_LOCKSTEP.
 * stats    points = n_points; paths = valid slots * q; rounds = rounds launched, summed over chunks; ray_slots = rounds * slots of
 *          the chunk, summed; live_ray_slots = closest-hit queries made for live paths; exact_walks over all walks of the call.
 * Memory   a chunk holds floor(chunk / K) whole points, so the stream sum never crosses a seam.  The bake grows the scene's staging
 *          by 24 (the point) + 12 (the first direction) + 12 or 108 (the accumulator) + 4 (the samples left) bytes per slot of a
 *          chunk (13.6 or 38.8 MB), with host arrays by the chunk's answer too, and uses rt_trace_paths' per-bounce stack.
 * Measured on one MI355X, synth_room_v1, device pointers, depth 6, kernel time (profiles/r29_bake.txt):
 *          2,073,600 texels x 16 samples, K = 1: 749 ms = 44.3 Mpaths/s; RT_BAKE_LOCKSTEP 759 ms; the loop of rt_bake_rays +
 *          rt_trace_paths from outside 736 ms; 768 rounds either way, 76.1 % of the ray slots live.  4,096 SH9 probes x 4,096
 *          samples, K = 64: 362 ms = 46.3 Mpaths/s in 366 rounds (83.0 % live); lockstep 382 ms in 384; outside loop 363 ms.
 *          Restarting in place does not shorten a chunk whose slowest slot runs q * ray_depth rounds, and among 262,144 slots
 *          one does; the bits of all three are the same.  The per-round poll costs 19 us a round.  rq_bake_advance_kernel: 45 VGPRs,
 *          28 bytes of scratch per lane (rq_path_advance_kernel's), no LDS; rq_bake_rays_kernel 34 VGPRs, rq_bake_resolve_kernel 12. */
typedef struct rt_bake_point { float p[3]; float n[3]; } rt_bake_point;   /* 24 bytes */
#define RT_BAKE_IRRADIANCE 0   /* out: 3 floats per point  */
#define RT_BAKE_SH9        1   /* out: 27 floats per point, [m][c], m = 0..8, c = r,g,b */
#define RT_BAKE_LOCKSTEP   4u  /* flag, next to RT_QUERY_DEVICE_POINTERS (1) and RT_QUERY_REFERENCE_WALK (2) */
typedef struct rt_bake_params {
    uint32_t struct_size; int32_t mode; int32_t samples; int32_t streams; int32_t ray_depth; uint32_t flags; uint32_t reserved[2];
} rt_bake_params;
typedef struct rt_bake_stats {
    uint32_t struct_size, reference_exact; uint64_t points, invalid_points, paths, exact_walks;
    uint64_t rounds, ray_slots, live_ray_slots; double kernel_ms, total_ms; uint32_t launches, reserved;
} rt_bake_stats;
int rt_bake_rays(rt_scene *scene, const rt_bake_point *points, rt_rng *rng /* in and out */, size_t n, int32_t mode, uint32_t flags,
                 rt_ray *out, rt_query_stats *stats /* nullable */);
int rt_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params,
            rt_rng *rng /* n_points*streams, [i*streams+k], in and out */, float *out, rt_bake_stats *stats /* nullable */);

/* ---- rt_render_paths, rt_render_bake: a caller's paths at render speed -----------------------------------------------------------
 * rt_trace_paths and rt_bake (RT_BAKE_IRRADIANCE) through the persistent render kernel: one launch per chunk instead of a round of
 * launches per bounce, no record through memory between the stages, no dead ray slots.  The kernel is rt_render's, compiled with a
 * path source (device/rt_path_source.h): a slot's first ray comes from the caller's array, or from rt_bake_rays' expressions on the
 * slot's point, instead of the camera; sum, engine and end of slot are a resumable render's (rt_accum_*) over 24 bytes per slot.  The
 * frame is an unsharded strip 8 pixels wide and 8 * ceil(n / 64) high, whose pixel slots are the record indices.  ABI version 6 still.
 *
 * Contract   on a scene whose renders and queries report reference_exact = 1, out and rng are bit for bit rt_trace_paths' / rt_bake's
 *          for the same arguments; the composed calls are the referees (tests/test_gpu_render_paths.py).  Floats leave through the
 *          queries' rule: a NaN has its sign bit set.  An engine leaves with saved = 0 whenever has_saved is 0.  Invalid records (the
 *          referees' rules) answer zeros, keep their engines and are counted.  On a scene with reference_exact = 0
 *          (RT_BUILD_DEVICE_BVH, RTAMD_NO_EXACT_BOXES) the calls are served, the stats say reference_exact = 0, the answers are the
 *          persistent walkers' padded-box answers, and equality with the composed calls is NOT promised.
 * First rays the walkers were not derived for -- an origin outside the walkers' node grid, a ray off rt_query_closest's fast list
 *          (|o| beyond scene and camera, a zero direction component, |d| outside 1/16 .. 16), one that pierces a tripwire -- are
 *          walked by the exact role from the start and counted in exact_walks.
 * Refusals   before any device work.  RT_ERR_INVALID_ARG: null arguments, struct_size, reserved words, flags other than
 *          RT_QUERY_DEVICE_POINTERS (alignments as rt_trace_paths / rt_bake), a host engine outside 1 .. 2^31-2 (the record is named).
 *          RT_ERR_LIMIT: ray_depth > 16, streams > 64, n_points * streams >= 2^31, samples / streams >= 2^25.  RT_ERR_UNSUPPORTED:
 *          RT_BAKE_SH9 (rt_bake serves it, and rt_render_probes below at this speed), hw6 and .txt scenes, and whatever keeps the persistent hw8 kernel from the scene
 *          (RTAMD_KERNEL=wavefront|mega, trees beyond its stack columns): there is no fallback, as with rt_accum_create.  n = 0: RT_OK.
 * stats    rt_query_stats: rays = n, invalid_rays, exact_walks = exact closest hits + exact light sums of the launches, kernel_ms =
 *          the render launches' (the pack and unpack launches are in total_ms), launches, reference_exact.  rt_bake_stats: points,
 *          invalid_points, paths, exact_walks, times, launches; rounds = ray_slots = live_ray_slots = 0: there are no rounds.
 * Memory   a chunk holds 2,073,600 slots (whole points: floor(chunk / K)), the pixel slots of a 1080p frame, so the kernel's path
 *          records never exceed what rt_render of that frame allocates (256 bytes per slot at depth 6).  The state (24 bytes per slot
 *          of a chunk, 50 MB) and, with host arrays, the chunk's records (52 bytes per slot) are kept by the scene, not part of
 *          rt_scene_info.device_bytes, freed with it.  RTAMD_QUERY_CHUNK lowers the chunk.  The calls only read the scene: an
 *          rt_accum of it and the next rt_render see nothing of them.
 * Measured on one MI355X, synth_room_v1, device pointers, depth 6, kernel time, alternating with the referee in one process
 *          (profiles/r30_render_paths.txt): the 2,073,600 camera-ray records of the 1080p frame 5.52 ms = 376
 *          Mpaths/s against rt_trace_paths' 44.55 ms, rt_render(samples = 1) of that frame 5.22 ms; 2,073,600 texels x 16 samples,
 *          K = 1: 79.9 ms = 415 Mpaths/s against rt_bake's 745 ms; 4,096 points x 4,096 samples, K = 64: 62.9 ms = 267 Mpaths/s
 *          against 368 ms.  The chunk: 262,144 slots 8.55 and 123.4 ms, 1,048,576 5.66 and 94.8 ms, 2,073,600 5.52 and 79.9 ms.  The
 *          two kernels: 87 VGPRs, no scratch, five waves per SIMD, 31,680 bytes of LDS; the renderer's own kernels are unchanged. */
int rt_render_paths(rt_scene *scene, const rt_ray *rays, rt_rng *rng /* in and out */, size_t n, int32_t ray_depth,
                    uint32_t flags, float *out_rgb /* n*3 */, rt_query_stats *stats /* nullable */);
int rt_render_bake(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params,
                   rt_rng *rng /* n_points*streams, [i*streams+k], in and out */, float *out /* n_points*3 */, rt_bake_stats *stats /* nullable */);

/* ---- rt_render_probes: SH9 probe bakes at render speed ---------------------------------------------------------------------------
 * rt_bake (RT_BAKE_SH9) through the persistent render kernel, the way rt_render_bake serves irradiance.  What does not fit the
 * kernel's path record -- 27 accumulators and the sample's first direction -- lives beside the slots' state, 120 bytes per slot
 * (device/rt_path_source.h), and the kernel is a third source kernel of its own: rt_render_paths' and rt_render_bake's are the code
 * they were, and rt_render_bake keeps refusing RT_BAKE_SH9.  ABI version 6 still.
 *
 * Contract   on a scene whose renders and queries report reference_exact = 1, out and rng are bit for bit rt_bake's for the same
 *          arguments with mode = RT_BAKE_SH9 (the referee, tests/test_gpu_render_probes.py).  The same expressions: o = p, d =
 *          normalize of three normal draws, acc[m][c] = acc[m][c] + (Y_m(d) * L[c]) with the nine Y_m as rt_bake spells them, one
 *          rounding per operation, d the sample's first direction; out = (float)(4 pi / (double)samples) * (((acc_0 + acc_1) + acc_2)
 *          ...) over the point's streams, through the queries' rule for floats (a NaN leaves with its sign bit set).  An engine leaves
 *          with saved = 0 whenever has_saved is 0, `reserved` is handed through.  On a scene with reference_exact = 0 the call is
 *          served, the stats say 0 and equality with rt_bake is NOT promised (as rt_render_bake).
 * Invalid points   rt_bake's SH9 rule: a NaN or an infinity in p, or any of the point's K engines outside 1 .. 2^31-2.  n is not read:
 *          n == 0 or a NaN n is a valid point.  An invalid point answers 27 zeros, keeps all its engines and is counted once in
 *          invalid_points.  Host engine arrays are checked before any launch (RT_ERR_INVALID_ARG, the record named); device arrays are
 *          judged on the device.
 * First rays   a probe's ray starts at p itself, no epsilon offset, and p may lie anywhere: every sample's first ray is classified
 *          as rt_render_paths classifies a caller's ray, and what the walkers were not derived for (an origin outside their node
 *          grid, ...) is walked by the exact role and counted in exact_walks.  Too cautious costs speed only.
 * Refusals   before any device work, each naming its field: rt_render_bake's (null arguments, struct_size, reserved words, flags
 *          other than RT_QUERY_DEVICE_POINTERS, alignments, host engines; RT_ERR_LIMIT: ray_depth > 16, streams > 64, n_points *
 *          streams >= 2^31, samples / streams >= 2^25); RT_ERR_INVALID_ARG: mode = RT_BAKE_IRRADIANCE (rt_render_bake serves it);
 *          RT_ERR_UNSUPPORTED: hw6 and .txt scenes and whatever keeps the persistent hw8 kernel from the scene
 *          (RTAMD_KERNEL=wavefront|mega, trees beyond its stack columns): no fallback.  n_points = 0: RT_OK, no launch.
 * stats    as rt_render_bake: points, invalid_points, paths, exact_walks, times, launches (three per chunk and phase: pack, render,
 *          unpack), reference_exact; rounds = ray_slots = live_ray_slots = 0.
 * Memory   chunks as rt_render_bake's (2,073,600 slots, whole points; RTAMD_QUERY_CHUNK lowers it).  Per slot of a chunk 24 bytes of
 *          state and 120 bytes of accumulators and first direction: 144 bytes, 299 MB for a full chunk, 38 MB for 4,096 probes of 64
 *          streams; with host arrays 40 bytes per slot (engines, points) and 108 bytes of answer per point beside them.  Kept in the
 *          scene's source staging: not part of rt_scene_info.device_bytes, freed with the scene.  The call only reads the scene.
 * Measured on one MI355X, synth_room_v1, device pointers, depth 6, kernel time, five repeats alternating with the referee in one
 *          process (profiles/r34_render_probes.txt): 4,096 probes x 4,096 samples, K = 64: 63.4 ms (62.8 .. 63.4)
 *          = 265 Mpaths/s against rt_bake's 365.1 ms (364.9 .. 365.4), 5.8 x, the referee's bits; rt_render_bake irradiance on the
 *          same points 62.2 ms: the SH mode costs 1.2 ms.  2,073,600 texels x 16 samples, K = 1 (one full chunk): 79.3 ms (78.4 .. 81.1)
 *          = 419 Mpaths/s against 747.0 ms (745.0 .. 748.2), 9.4 x; irradiance 78.8 ms.  In that run ONE of the 2,073,600 points
 *          differs from rt_bake: a path on which the persistent kernel itself (rt_render_paths, too) parts from the reference on its
 *          sixth ray, 1 in 33 million, located in the profile file and not fixed.  The kernel: 89 VGPRs, no scratch, five waves per
 *          SIMD, 31,680 bytes of LDS; every other kernel is, instruction for instruction, the one it was. */
int rt_render_probes(rt_scene *scene, const rt_bake_point *points, size_t n_points, const rt_bake_params *params,
                     rt_rng *rng /* n_points*streams, [i*streams+k], in and out */, float *out /* n_points*27, [m][c] */,
                     rt_bake_stats *stats /* nullable */);

/* ---- denoised previews: a variance-guided edge-avoiding filter on the guide images -------------------------------------------
 * What consumes rt_render_guides' planes: a noisy frame of few samples in, a usable preview out.  An a-trous wavelet filter (five
 * taps per axis, stride doubling per level) whose weights stop at normal, depth and -- with rt_noise_estimate's map -- luminance edges
 * as wide as the pixel's own noise.  rt_denoise is an image filter: the scene only names the GPU, owns the working set and serialises the
 * call, so it works on a scene of any kind and on frames of rt_multi_*; no render kernel knows of it and no picture changes because
 * of it.  ABI version 6 still.
 *
 * rt_denoise        planes row-major, row 0 first: rgb, normal W*H*3, depth W*H (rt_render_guides' normal and depth), albedo and
 *                   emission W*H*3 or NULL, se W*H (rt_noise_estimate's map) or NULL; out_rgb W*H*3 floats and / or out_rgb8 their
 *                   tonemapped bytes.  Host memory, or with RT_DENOISE_DEVICE_POINTERS memory on the scene's GPU, read and written in
 *                   place; out_rgb may be rgb.  The work is ordered on the null stream and has finished when the call returns.
 *                   albedo NULL = no demodulation.  Demodulating by the pixel-centre albedo is opt-in: at preview sizes textures are
 *                   undersampled and the centre tap is not the albedo of the pixel's footprint.
 * rt_accum_denoise  the preview of a frame in progress, composed on the device with no trip to the host: the outputs equal, bit for
 *                   bit, rt_denoise applied to what rt_accum_resolve, rt_render_guides (device path, made by the first call and kept
 *                   until the rt_accum is destroyed: 40 bytes per pixel) and, if `noise` is given, rt_noise_estimate return.  The
 *                   emission plane is always passed, the albedo plane only with RT_DENOISE_ALBEDO, no error map when noise is NULL.
 *                   width and height of the params must be 0 or the accumulator's.  Outputs are host memory, or device memory with
 *                   RT_DENOISE_DEVICE_POINTERS.  It only reads: the checkpoint and the monitor's figures are the same bytes afterwards.
 * Refused before any device work, with a message naming the field: a null scene / accum, params, rgb, normal or depth, a wrong
 * struct_size (params, stats), reserved != 0, unknown flags, iterations outside 0 .. 8, a negative or non-finite sigma, both outputs
 * null, width or height < 1 (RT_ERR_INVALID_ARG); width * height > 2^26 (RT_ERR_LIMIT).  rt_accum_denoise: a sharded accumulator or
 * one of an hw6 scene is RT_ERR_UNSUPPORTED (what rt_render_guides refuses); no samples yet, a monitor of another accumulator or
 * with fewer than 2 batches, and a broken accumulator (its first error in the message) are RT_ERR_INVALID_ARG.
 *
 * Arithmetic (float32, one rounding per operation, no transcendental function; tests/denoise_model.py restates it in numpy bit for bit).
 *   Y(r, g, b) = ((0.2126f*r) + (0.7152f*g)) + (0.0722f*b);  max(a, b) = (a < b) ? b : a (a NaN b gives a)
 *   e16(x): t = max(0, 1 - x*0.0625f), squared four times: about exp(-x), zero from x = 16 and for a NaN.
 *   fixed   a pixel with depth not > 0 (a miss), with an emission channel != 0, or with a NaN / inf in its rgb, normal, depth,
 *           albedo or se.  Its output is its input bit for bit, it is no neighbour of any pixel, and rt_denoise_stats.fixed_pixels
 *           counts it: directly seen lights and the environment pass through unchanged.
 *   pack    a = max(1/64, albedo) per channel, 1 without the plane; irr = rgb / a; with se: s = se / Y(a), v = s*s, else v = 0.
 *           gx = (z(xr, y) - z(xl, y)) / (float)(xr - xl), xr = min(x+1, W-1), xl = max(x-1, 0), 0 when xr == xl; gy likewise
 *           (z the depth plane as given).
 *   level i = 0 .. iterations-1, step = 1 << i, for every pixel p that is not fixed:
 *           with se: pv = the 3x3 Gaussian of v around p (weights 1/2, 1/4 per axis, dy outer, dx inner) over the neighbours in the
 *           image that are not fixed, divided by the sum of the weights used; sd = sqrt(max(0, pv)).
 *           The 25 taps q = p + step*(dx, dy), dy outer, dx inner, both -2 .. 2; taps outside the image and fixed taps are skipped:
 *             h  = k[|dy|] * k[|dx|], k = (3/8, 1/4, 1/16)
 *             wn = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z), squared six times
 *             xz = |z_p - z_q| / (((sigma_depth * |gx_p*(float)(dx*step) + gy_p*(float)(dy*step)|) + 1e-3f*z_p) + 1e-12f)
 *             xl = |Y(irr_p) - Y(irr_q)| / ((sigma_luminance * sd) + 1e-6f), with se only
 *             w  = (h * e16(xz + xl)) * wn        (without se: e16(xz))
 *             acc += w*irr_q;  accw += w;  accv += (w*w)*v_q
 *           irr' = acc / accw, v' = accv / (accw*accw); a pixel whose accw is not > 0 keeps irr and v.  Levels ping-pong between
 *           two buffers; one lane sums a pixel in that order, so the bits depend on nothing but the planes.
 *   end     out = irr * a (a fixed pixel: its rgb as given); the bytes are rt_render's tonemap chain of those floats.
 * Working set: 56 bytes per pixel (116 MB at 1920x1080) plus the staging of host planes, a buffer of the scene grown on demand and
 * freed with it, not part of rt_scene_info.device_bytes.  One launch packs the planes, one per level follows.
 *
 * Measured on one MI355X (profiles/r22_denoise.txt): rt_denoise on a 1920x1080 frame with device planes, five
 * levels, takes 0.88 ms of kernels with the error map and 0.71 ms without (0.08 - 0.14 ms per level), 0.91 / 0.74 ms for the call with its
 * launches and its synchronisation, next to 72 ms of render kernels per slice of 16 samples.  On the sphere scene at 64x48 the filtered
 * frame of 16 samples has a third of the noisy frame's luminance RMSE against the 1,024-sample frame (0.041 against 0.129, on the CPU).
 *
 * What the filter does not do: no temporal reuse (every call stands alone), no supersampled albedo, and nothing to fixed pixels. */
typedef struct rt_denoise_params {
    uint32_t struct_size;      /* = sizeof(rt_denoise_params) */
    int32_t  width, height;    /* >= 1, width*height <= 2^26 (else RT_ERR_LIMIT); rt_accum_denoise: 0 or the accumulator's */
    int32_t  iterations;       /* 0 = default 5; 1 .. 8; level i taps at stride 2^i */
    float    sigma_depth;      /* 0 = default 1 */
    float    sigma_luminance;  /* 0 = default 4 */
    uint32_t flags;            /* RT_DENOISE_DEVICE_POINTERS, RT_DENOISE_ALBEDO (rt_accum_denoise only) */
    uint32_t reserved;         /* must be 0 */
} rt_denoise_params;
typedef struct rt_denoise_stats {
    uint32_t struct_size;      /* in: sizeof(rt_denoise_stats) */
    uint32_t launches;         /* 1 + iterations */
    uint64_t fixed_pixels;
    double   kernel_ms;        /* HIP-event time from the pack kernel to the last level */
    double   total_ms;         /* host wall time of the call (rt_accum_denoise: resolve, guides and estimate included) */
} rt_denoise_stats;
#define RT_DENOISE_DEVICE_POINTERS 1u /* rt_denoise: every plane and output is device memory; rt_accum_denoise: the outputs are */
#define RT_DENOISE_ALBEDO          2u /* rt_accum_denoise: demodulate by the albedo plane */
extern int rt_denoise(rt_scene *scene, const rt_denoise_params *params,
                      const float *rgb /* W*H*3 */, const float *normal /* W*H*3 */, const float *depth /* W*H */,
                      const float *albedo /* nullable: NULL = no demodulation */, const float *emission /* nullable */,
                      const float *se /* nullable: W*H, rt_noise_estimate's map */,
                      float *out_rgb /* nullable */, uint8_t *out_rgb8 /* nullable */, rt_denoise_stats *stats /* nullable */);
extern int rt_accum_denoise(rt_accum *accum, rt_noise *noise /* nullable */, const rt_denoise_params *params,
                            float *out_rgb /* nullable */, uint8_t *out_rgb8 /* nullable */, rt_denoise_stats *stats /* nullable */);

/* ---- adaptive sampling: freeze converged 8x8 sub-tiles -------------------------------------------------------------------------
 * What rt_accum, rt_noise and RTAMD_TARGET_NOISE lead up to: a resumable render that stops drawing samples where the picture is done.
 * An rt_adaptive owns its state -- it is NOT a mode of rt_accum, whose checkpoints, monitors, previews and multi-GPU frames all assume
 * one sample count per frame.  The state is rt_accum's (24 bytes per pixel slot) plus, per 8x8 sub-tile, its sample count, its
 * batches and observed samples, its flags and the noise monitor's three planes y0 / yp / m2 (12 bytes per pixel slot).  ABI version 6
 * still: additions only.
 *
 * Contract   pixels are independent and a camera ray depends only on the pixel and its engine, so a sub-tile that has drawn d samples
 *          holds exactly rt_render(samples = d)'s pixels, floats and bytes, whatever its neighbours drew (tests/test_gpu_adaptive.py:
 *          np.array_equal per distinct count).  With every sub-tile active in every slice the picture is rt_accum_resolve's and the
 *          map and summary are rt_noise_estimate's for the same slicing, bit for bit.
 * A slice    the state of the active sub-tiles is gathered into a compact strip (8 pixels wide, one sub-tile per 64 slots), the
 *          persistent hw8 kernel runs a slice of a resumable render over it with a path source of its own (src_mode 4, device/
 *          rt_path_source.h: the REAL frame's camera ray for the pixel behind each slot, the same code as the renders'), and the
 *          state is scattered back.  Every kernel that existed before is, instruction for instruction, the one it was.  Frames with
 *          more active pixel slots than one path-source chunk (2,073,600; RTAMD_QUERY_CHUNK lowers it) run the list in chunks.
 * Arithmetic the noise monitor's (rt_noise above), with n, N, B and d per sub-tile: a slice is one batch of the sub-tiles it drew
 *          for, the statistics of a frozen sub-tile do not move.  A sub-tile with fewer than 2 batches has no estimate: 0 in the map,
 *          RT_ADAPTIVE_NO_ESTIMATE in its entry, part of no frame figure.  rt_adaptive_resolve: pixel = (float)(1.0 / d_s) * sum as
 *          rt_accum_resolve, d_s the sub-tile's count; a sub-tile with d_s = 0 is zeros.
 * Decision (rt_adaptive_render; on the host, in double, in the frame's sub-tile order, after the slice's update and estimate).
 *          L = the frame's mean luminance as rt_noise_estimate sums it, over the sub-tiles that have an estimate.  A sub-tile with
 *          an estimate, batches >= min_batches and pixels > 0 becomes CONVERGED when sqrt(sum_se2 / pixels) <= target_noise * L; one
 *          with an estimate and pixels == 0 (every pixel non-finite) at once.  CONVERGED is sticky.  CAPPED: samples + n_samples >
 *          max_samples, n_samples the slice length of the call that decides.  ACTIVE = not CAPPED and (not CONVERGED, or
 *          RT_ADAPTIVE_DILATE and some 8-neighbour is neither CONVERGED nor CAPPED: no seams one sub-tile wide).  A fresh object has
 *          every sub-tile ACTIVE | NO_ESTIMATE.  rt_adaptive_render decides once more before it launches (the cap depends on this
 *          call's n_samples), draws n_samples for the ACTIVE sub-tiles, updates, estimates and decides.  With no active sub-tile it
 *          is RT_OK, launches nothing and reports samples = 0: the caller's stop condition.
 * rt_adaptive_render_tiles   the mechanism without the policy: mask[t] != 0 draws n_samples for sub-tile t (one byte per sub-tile,
 *          row-major over ceil(W/8) x ceil(H/8)); update and estimate as above, ACTIVE / CONVERGED / CAPPED are left as they were.
 * rt_adaptive_tiles   the sub-tiles' entries, host memory, ceil(W/8) * ceil(H/8) of them.
 * rt_adaptive_noise   the map (W*H floats, host memory or with RT_FLAG_OUT_DEVICE memory on the scene's GPU) and the frame figures
 *          as rt_noise_estimate adds them; batches, samples_observed and samples_total are the largest over the sub-tiles.
 *          RT_ERR_INVALID_ARG while no sub-tile has 2 batches.
 * rt_adaptive_sample_map   W*H counts, host memory.
 * stats    active_tiles: sub-tiles this call drew for; converged_tiles / capped_tiles: as flagged when it returns; samples: camera
 *          samples drawn (pixels inside the image x n_samples); min_samples / max_samples per pixel over the frame; kernel_ms: the
 *          persistent kernel's launches; gather_ms / scatter_ms: the two kernels around it; total_ms: host wall time of the call.
 * Refusals   before anything is launched, the state untouched.  RT_ERR_UNSUPPORTED, no fallback: integrators other than
 *          RT_INTEGRATOR_HW8, shard_count > 1, sample_streams > 1, render flags other than 0, and whatever keeps the persistent hw8
 *          kernel from the scene (RTAMD_KERNEL=wavefront|mega, a tree beyond its stack columns).  RT_ERR_INVALID_ARG: null arguments,
 *          struct_size, reserved words, target_noise not finite or <= 0, min_batches < 0 or 1, max_samples < 0, unknown flags,
 *          n_samples <= 0, a broken object.  RT_ERR_LIMIT: width or height above 65,535 (the slot's pixel is one packed word), and a
 *          slice that would take an active sub-tile's count to the path records' sample index limit (2^25).  A slice that fails
 *          under way leaves the object broken, as with rt_accum.
 * Out of scope   checkpoints of an rt_adaptive, rt_multi_*, hw7 / hw6, rt_accum_denoise on it.
 * Measured on one MI355X: profiles/r35_adaptive.txt. */
typedef struct rt_adaptive_params {
    uint32_t struct_size;
    float    target_noise;   /* a sub-tile converges when sqrt(its mean se^2) <= target_noise * frame mean luminance; > 0, finite */
    int32_t  min_batches;    /* never judged before this many slices of its own; >= 2; 0 = 4 (RTAMD_NOISE_MIN_BATCHES' default) */
    int32_t  max_samples;    /* a sub-tile whose next slice would pass this stops ("capped"); 0 = the sample-index limit */
    uint32_t flags;          /* RT_ADAPTIVE_DILATE */
    int32_t  reserved;       /* 0 */
} rt_adaptive_params;
#define RT_ADAPTIVE_DILATE 1u
typedef struct rt_adaptive_tile {   /* 32 bytes, one per 8x8 sub-tile, row-major over ceil(W/8) x ceil(H/8) */
    int32_t  samples, batches;
    uint32_t pixels, nonfinite;     /* of the last estimate: pixels with a finite estimate, pixels inside the image without */
    float    sum_se2, sum_luminance;
    uint32_t flags;                 /* RT_ADAPTIVE_ACTIVE, _CONVERGED, _CAPPED, _NO_ESTIMATE */
    uint32_t reserved;
} rt_adaptive_tile;
#define RT_ADAPTIVE_ACTIVE      1u
#define RT_ADAPTIVE_CONVERGED   2u
#define RT_ADAPTIVE_CAPPED      4u
#define RT_ADAPTIVE_NO_ESTIMATE 8u
typedef struct rt_adaptive_stats {
    uint32_t struct_size;           /* in: sizeof(rt_adaptive_stats) */
    uint32_t active_tiles, converged_tiles, capped_tiles;
    uint64_t samples;
    int32_t  min_samples, max_samples;
    double   kernel_ms, gather_ms, scatter_ms, total_ms;
    uint32_t launches, reference_exact;
    uint64_t exact_walks;
} rt_adaptive_stats;
typedef struct rt_adaptive rt_adaptive;
int  rt_adaptive_create(rt_scene *scene, const rt_render_params *params, const rt_adaptive_params *adaptive, rt_adaptive **out);
int  rt_adaptive_render(rt_adaptive *a, int32_t n_samples, rt_adaptive_stats *stats /* nullable */);
int  rt_adaptive_render_tiles(rt_adaptive *a, int32_t n_samples, const uint8_t *mask, rt_adaptive_stats *stats /* nullable */);
int  rt_adaptive_tiles(rt_adaptive *a, rt_adaptive_tile *out);
int  rt_adaptive_resolve(rt_adaptive *a, uint32_t flags, float *out_rgb /* nullable */, uint8_t *out_rgb8 /* nullable */);
int  rt_adaptive_noise(rt_adaptive *a, uint32_t flags, float *out_se /* nullable */, rt_noise_summary *summary /* nullable */);
int  rt_adaptive_sample_map(rt_adaptive *a, int32_t *out /* W*H */);
void rt_adaptive_destroy(rt_adaptive *a);

/* ---- view sets: a batch of cameras over one live scene -------------------------------------------------------------------------
 * A scene is bound to the one camera of its rt_scene_desc; a second viewpoint used to mean rt_scene_create again.  An rt_views renders
 * n_views cameras of the caller's, one frame size for all, from the scene as it stands, many small views in one launch.  It owns its
 * state -- rt_accum's, 24 bytes per pixel slot, per view -- and only READS the scene: the scene's own camera, its node grid, box_c2,
 * every rt_accum and rt_adaptive on it and the next rt_render see nothing of a view set.  ABI version 6 still: additions only.
 *
 * Contract   on a scene whose renders report reference_exact = 1, view v after d samples holds, bit for bit, floats and bytes, what
 *          rt_render(samples = d) returns on a scene created from the same rt_scene_desc with camera = cameras[v] -- whatever the other
 *          views are, whatever they drew and however the samples were sliced (tests/test_gpu_views.py).  The engines are the
 *          reference's: pixel (x, y) of every view starts from minstd_rand(y * W + x).  On a scene with reference_exact = 0 the calls
 *          are served and the stats say 0; equality is then not promised, as with rt_render_bake.
 * Cameras    position, right, up, forward and fov_y are used as given (not normalised, not orthogonalised, as the reference uses
 *          them); tan_fov_y = (float)tan((double)(fov_y / 2)) by the host libm and tan_fov_x = tan_fov_y * width / height, the
 *          expressions of the scene's own camera.  fov_x is ignored.
 * A slice    (rt_views_render) every view with mask[v] != 0 -- a NULL mask: every view -- draws n_samples more samples; counts are
 *          per view (rt_views_samples).  The state of the active views' 8x8 sub-tiles is gathered into a compact strip, the persistent
 *          hw8 kernel runs a slice of a resumable render over it with a path source of its own (src_mode 5, device/rt_path_source.h:
 *          the camera ray of the view behind each slot, from a device array of per-view camera records), and the state is scattered
 *          back.  Every kernel that existed before is, instruction for instruction, the one it was.  More active pixel slots than one
 *          path-source chunk (2,073,600; RTAMD_QUERY_CHUNK lowers it) run in chunks of whole sub-tiles.  With no active view the call
 *          is RT_OK, launches nothing and reports samples = 0.
 * First rays  the walkers' 16-bit node grid and the query layer's origin bound were derived for the SCENE's camera.  A view's first
 *          ray whose origin lies outside the grid or beyond the bound, or that pierces a tripwire, is the exact role's from the start
 *          (pt_source_exact, as rt_render_paths' rays): the pixels are the same, the speed is not.  Create the scene with a camera
 *          that spans the volume the views will move in; profiles/r36_views.txt has the cost when every first ray is exact.
 * rt_views_set_cameras   replaces the cameras of views first .. first + n - 1 and resets those views: sum 0, engines reseeded,
 *          0 samples.  The other views are untouched.
 * rt_views_resolve   view `view`: (float)(1.0 / d_v) * sum and the tonemapped bytes, W x H x 3 row-major, host memory or with
 *          RT_FLAG_OUT_DEVICE memory on the scene's GPU, as rt_accum_resolve.  A view with 0 samples is RT_ERR_INVALID_ARG.  The state
 *          is only read.
 * stats    active_views: views this call drew for; samples: camera samples drawn (active views x W x H x n_samples); min_samples /
 *          max_samples per pixel over all views when the call returns; kernel_ms: the persistent kernel's launches; gather_ms /
 *          scatter_ms: the two kernels around it; total_ms: host wall time of the call; exact_walks: closest hits and light sums the
 *          exact role answered.
 * Refusals   before any device work, the state untouched; the message names the field and, where it applies, the view.
 *          RT_ERR_INVALID_ARG: null arguments, struct_size of the params or the stats, reserved words or flags other than 0,
 *          n_views < 1, width or height below 1, first / n / view out of range, n_samples <= 0, a broken object, and a bad camera: a
 *          component that is not finite or above 2^40 in magnitude (with that bound no float expression of the camera ray overflows
 *          at any frame size allowed here), fov_y outside (0, 3], or right, up and forward not linearly independent (the determinant
 *          in double against the product of the three lengths; with independent vectors cx * right - cy * up + forward is never
 *          zero, so no first direction is a NaN).  RT_ERR_LIMIT: width or height above 65,535 (a slot's pixel is one packed word),
 *          ray_depth above 16, n_views x the pixel slots of a view (64 per 8x8 sub-tile) at or above 2^31, and a slice that would
 *          take an active view's count to the path records' sample index limit (2^25).  RT_ERR_UNSUPPORTED, no fallback, as
 *          rt_adaptive_create answers: scenes that are not hw8 scenes, and whatever keeps the persistent hw8 kernel from the scene
 *          (RTAMD_KERNEL=wavefront|mega, a tree beyond its stack columns).  A slice that fails under way leaves the object broken,
 *          as with rt_accum.
 * Out of scope   an rt_views has no adaptive sampling per view: every pixel of a view draws what the view draws.  That lives in
 *          rt_view_adaptive_* below, an object of its own over the same kind of state.  Out of scope for both: checkpoints of a view set;
 *          rt_noise, rt_denoise, guide images and rt_camera_rays for a view's camera; rt_multi_*; hw7 and hw6; views of different sizes.
 * Measured on one MI355X: profiles/r36_views.txt. */
typedef struct rt_views_params {
    uint32_t struct_size;
    int32_t  width, height;   /* one frame size for all views; 1 .. 65,535 each */
    int32_t  ray_depth;       /* 0 = 6; > 16: RT_ERR_LIMIT */
    int32_t  n_views;         /* >= 1; n_views * pixel slots of a view < 2^31 */
    uint32_t flags;           /* 0 */
    void    *stream;          /* hipStream_t of the set's launches and copies; NULL = the default stream */
    uint32_t reserved[2];     /* 0 */
} rt_views_params;
typedef struct rt_views_stats {
    uint32_t struct_size;                   /* in: sizeof(rt_views_stats) */
    uint32_t active_views;
    uint64_t samples;                       /* camera samples drawn by this call */
    int32_t  min_samples, max_samples;      /* per pixel, over the views */
    double   kernel_ms, gather_ms, scatter_ms, total_ms;
    uint32_t launches, reference_exact;
    uint64_t exact_walks;
} rt_views_stats;
typedef struct rt_views rt_views;
int  rt_views_create(rt_scene *scene, const rt_views_params *params, const rt_camera *cameras /* n_views */, rt_views **out);
int  rt_views_set_cameras(rt_views *v, int32_t first, int32_t n, const rt_camera *cameras /* n */);
int  rt_views_render(rt_views *v, int32_t n_samples, const uint8_t *mask /* nullable: n_views bytes */, rt_views_stats *stats);
int  rt_views_samples(const rt_views *v, int32_t *out /* n_views */);
int  rt_views_resolve(rt_views *v, int32_t view, uint32_t flags /* RT_FLAG_OUT_DEVICE */, float *out_rgb /* nullable */, uint8_t *out_rgb8 /* nullable */);
void rt_views_destroy(rt_views *v);

/* ---- adaptive view sets: freeze converged 8x8 sub-tiles per camera -------------------------------------------------------------
 * rt_adaptive stops drawing samples where ONE camera's picture is done; rt_views renders many cameras in one launch, every pixel the
 * same count.  An rt_view_adaptive does both: the strip of a slice holds the ACTIVE sub-tiles of ALL views, in any mix, so a wall and
 * a glossy object under an emitter each draw what they need and many small views still fill one launch.  The persistent kernel is
 * the one rt_views runs (src_mode 5 reads the view per 64-slot group and the pixel per slot); no variant was added.  ABI version 6
 * still: additions only.  rt_views_params, rt_adaptive_params, rt_adaptive_tile and rt_noise_summary are those above;
 * rt_views_params.flags stays 0.
 *
 * State      per view one rt_accum block (24 bytes per pixel slot) plus the noise monitor's three planes y0 / yp / m2 (12 bytes per
 *          slot); per (view, sub-tile) what rt_adaptive keeps per sub-tile: samples, batches, observed samples, flags and the last
 *          estimate's entry.
 * Contract   on a scene whose renders report reference_exact = 1: take view v of a set driven by rt_view_adaptive_render with v in the
 *          mask for slices n_1, n_2, ..., and an rt_adaptive with the same rt_adaptive_params on a scene created from the same
 *          rt_scene_desc with camera = cameras[v], driven by rt_adaptive_render with the same slice lengths.  The 32-byte tile
 *          entries, the resolved floats and bytes, the noise map and every summary field, and the sample map are the same, bit for
 *          bit -- whatever the other views are and whatever they drew (tests/test_gpu_view_adaptive.py).  Consequently a sub-tile
 *          that has drawn d samples holds rt_render(samples = d)'s pixels on that scene.
 * Decision   per view, the decision of rt_adaptive_render over that view's table with that view's own mean luminance L; dilation looks
 *          at the 8 neighbours inside the view only.  A view whose view_mask byte is 0 (a NULL mask: every view takes part) draws
 *          nothing in that call and keeps its entries and flags.  The call decides once more before it launches (the cap depends on
 *          this call's n_samples), draws, updates, estimates and decides, as rt_adaptive_render does.  With no active sub-tile in any
 *          masked view it is RT_OK, launches nothing and reports samples = 0: the caller's stop condition.
 * A slice    per chunk one gather, the persistent kernel, one scatter; then ONE update launch over the list and ONE estimate launch
 *          over all sub-tiles of all views: the launch count does not grow with n_views.  A strip entry is one word
 *          view * tiles + sub-tile, the list ascending.  Chunks are RTAMD_QUERY_CHUNK-sized, made of whole sub-tiles, and may split
 *          a view.  Cameras and first rays outside the node grid follow rt_views' rules above.
 * rt_view_adaptive_render_tiles   the mechanism without the policy: one byte per (view, sub-tile), view-major; update and estimate as
 *          above, ACTIVE / CONVERGED / CAPPED are left as they were.
 * rt_view_adaptive_set_cameras   replaces the cameras of views first .. first + n - 1 and resets those views: sums 0, engines reseeded,
 *          counts and batches 0, every sub-tile ACTIVE | NO_ESTIMATE.  The other views are untouched.
 * rt_view_adaptive_tiles / _resolve / _noise / _sample_map   one view's, as the rt_adaptive_* calls of the same name.
 *          rt_view_adaptive_noise is RT_ERR_INVALID_ARG while no sub-tile of that view has 2 batches; samples_total, batches and
 *          samples_observed are the largest over the view's sub-tiles.
 * stats    active_views: views for which at least one sub-tile drew in this call; active_tiles: (view, sub-tile) pairs it drew for;
 *          converged_tiles / capped_tiles: over all views, as flagged when the call returns; samples: camera samples drawn (pixels
 *          inside the image x n_samples); min_samples / max_samples per pixel over all views; noise_ms: the update and estimate
 *          launches; the rest as rt_views_stats.
 * Refusals   before any device work, the state untouched; the message names the field and, where it applies, the view or sub-tile.
 *          What rt_views_create refuses (struct sizes, reserved words, flags, n_views, sizes, bad cameras, the limits, scenes that are
 *          not hw8 scenes or that the persistent hw8 kernel cannot take), what rt_adaptive_create refuses (target_noise, min_batches,
 *          max_samples, unknown adaptive flags), and what a slice refuses (n_samples <= 0, the 2^25 sample-index limit per active
 *          sub-tile), each with that call's status.  A slice that fails under way leaves the object broken, as with rt_views.
 * Out of scope   checkpoints of an adaptive view set; rt_multi_*; hw7 and hw6; rt_denoise and guide images for a view's camera; views
 *          of different sizes.
 * Measured on one MI355X, 64 views of 128x128 in slices of 16 (profiles/r38_view_adaptive.txt): an all-active
 *          slice costs what rt_views_render's does (51.6 against 51.8 ms; update and estimate 0.021 ms); to the median of the views'
 *          worst-sub-tile noise the set draws 0.512 of the uniform 64-sample set's camera samples in 0.587 x its wall time.  The target
 *          is relative to each view's own mean luminance: a view with almost no light in it runs to max_samples, so set one.  Not
 *          measured: RT_ADAPTIVE_DILATE on a set, sets beyond one chunk. */
typedef struct rt_view_adaptive_stats {
    uint32_t struct_size, active_views;                              /* in: sizeof(rt_view_adaptive_stats) */
    uint32_t active_tiles, converged_tiles, capped_tiles, launches;
    uint64_t samples;
    int32_t  min_samples, max_samples;
    double   kernel_ms, gather_ms, scatter_ms, noise_ms, total_ms;
    uint32_t reference_exact, reserved;
    uint64_t exact_walks;
} rt_view_adaptive_stats;
typedef struct rt_view_adaptive rt_view_adaptive;
int  rt_view_adaptive_create(rt_scene *scene, const rt_views_params *params, const rt_adaptive_params *adaptive,
                             const rt_camera *cameras /* n_views */, rt_view_adaptive **out);
int  rt_view_adaptive_set_cameras(rt_view_adaptive *a, int32_t first, int32_t n, const rt_camera *cameras /* n */);
int  rt_view_adaptive_render(rt_view_adaptive *a, int32_t n_samples, const uint8_t *view_mask /* nullable: n_views bytes */, rt_view_adaptive_stats *stats);
int  rt_view_adaptive_render_tiles(rt_view_adaptive *a, int32_t n_samples, const uint8_t *tile_mask /* n_views * tiles bytes */, rt_view_adaptive_stats *stats);
int  rt_view_adaptive_tiles(rt_view_adaptive *a, int32_t view, rt_adaptive_tile *out /* tiles */);
int  rt_view_adaptive_resolve(rt_view_adaptive *a, int32_t view, uint32_t flags /* RT_FLAG_OUT_DEVICE */, float *out_rgb /* nullable */, uint8_t *out_rgb8 /* nullable */);
int  rt_view_adaptive_noise(rt_view_adaptive *a, int32_t view, uint32_t flags, float *out_se /* nullable */, rt_noise_summary *summary /* nullable */);
int  rt_view_adaptive_sample_map(rt_view_adaptive *a, int32_t view, int32_t *out /* W*H */);
void rt_view_adaptive_destroy(rt_view_adaptive *a);

/* Scene info the host side needs after preparation. */
typedef struct rt_scene_info {
    uint32_t n_triangles, n_lights, n_bvh_nodes, n_light_bvh_nodes;
    uint32_t bvh_depth, light_bvh_depth;
    uint64_t device_bytes;
    double prep_ms, upload_ms;   /* host preparation; upload (+ the tree build on the GPU when bvh_on_device) */
    double bvh_build_ms;         /* GPU time of the on-device scene-tree build (device/rt_bvh_build.h), 0 when built on the host */
    uint32_t bvh_on_device;      /* 1 = the traversal tree of the scene was built on the GPU */
    uint32_t reserved;
} rt_scene_info;
int rt_scene_get_info(const rt_scene *scene, rt_scene_info *info);
/* Light order chosen by preparation (indices into the LOAD-order triangle arrays);
 * parity-critical: reference hw8/src/include/distributions.h:103-115. */
int rt_scene_get_light_order(const rt_scene *scene, uint32_t *out, uint32_t capacity);

/* Host-only part of rt_scene_create (no GPU needed): the figure order after the reference's BVH build and the light order,
 * as indices into the LOAD-order arrays, for the integrator family the desc belongs to (`integrator` = HW8 / HW6 for glTF
 * scenes, HW5 for .txt scenes).  Either output may be NULL; capacities in elements.  Returns the number of lights. */
int rt_host_prepare_orders(const rt_scene_desc *desc, int integrator, uint32_t *figure_order, uint32_t figure_capacity,
                           uint32_t *light_order, uint32_t light_capacity);

/* ---- host-side front-end (replaces sceneio::loadScene / loadTexture) -------------------- */
typedef struct rt_host_scene rt_host_scene; /* owns the arrays a desc points into */

/* glTF 2.0 subset loader, float-for-float the reference's (hw8/src/sceneio.cpp:348-372).
 * flavor: RT_INTEGRATOR_HW6 or RT_INTEGRATOR_HW8 (material interpretation differs). */
int rt_load_gltf(const char *path, int flavor, rt_host_scene **out);
/* .txt scene loader (flavor RT_INTEGRATOR_HW1..HW5 picks that snapshot's grammar: hw1/src/sceneio.cpp:8-97,
 * hw2/src/sceneio.cpp:8-147, hw3/src/sceneio.cpp:8-107, hw5/src/sceneio.cpp:8-101). Fills width/height/samples/ray_depth. */
int rt_load_txt(const char *path, int flavor, rt_host_scene **out,
                int32_t *width, int32_t *height, int32_t *samples, int32_t *ray_depth);
int rt_host_scene_set_environment(rt_host_scene *hs, const char *image_path);
const rt_scene_desc *rt_host_scene_desc(const rt_host_scene *hs);
void rt_host_scene_free(rt_host_scene *hs);
/* Binary PPM writer (hw8/src/sceneio.cpp:383-385,397-401). */
int rt_write_ppm(const char *path, int32_t width, int32_t height, const uint8_t *rgb8);
/* Image file -> 3-channel RGB8 like stbi_load(path, ..., 3): PNG (8-bit gray/RGB/RGBA/palette, non-interlaced) or
 * baseline JPEG (grayscale / YCbCr, 1x or 2x chroma subsampling), chosen by magic bytes; caller frees with rt_free. */
int rt_decode_png(const char *path, int32_t *width, int32_t *height, uint8_t **rgb);
void rt_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* RTAMD_H */

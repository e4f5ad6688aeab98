"""Scenes and ray sets of the first-hit layer's GPU tests (test_gpu_query_surface.py, test_gpu_guides.py), built once per process."""
import ctypes as C
import functools
import os

import numpy as np

import oracle_lib
import pin_cases

rt = pin_cases.rt
MISS = 0xFFFFFFFF
KINDS = ("base_color_texture", "emissive_texture", "metallic_roughness_texture", "normal_texture")
# Which of the four texture kinds each of a soup's six materials carries: dealt by hand, not by chance.
TABLES = {"soup_a": ((1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1)),
          "soup_b": ((0, 1, 1, 0), (1, 1, 1, 1), (1, 0, 0, 1), (0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 1, 0))}
# Image sizes (w, h), handed out in order: the smallest, the largest, and odd non-square ones in between.
SIZES = ((2, 2), (32, 32), (3, 17), (31, 2), (5, 5), (16, 9), (2, 32), (7, 13), (32, 3), (11, 11), (4, 29), (23, 6))
SOUP_SEEDS = {"soup_a": 211, "soup_b": 212}


def table_is_fair(table):
    """Each kind on at least two of the six materials and absent on at least one; at least one material with all four."""
    t = np.array(table)
    return t.shape == (6, 4) and bool(np.all(t.sum(axis=0) >= 2) and np.all(t.sum(axis=0) <= 5) and np.any(t.sum(axis=1) == 4))


def _with(sd, environment=None, bg=None):
    return rt.SceneData(sd.positions, sd.texcoords, sd.normals, sd.tangents, sd.material_index, list(sd.materials)[:sd.n_materials],
                        sd.texture_source, sd.images, sd.camera, sd.bg if bg is None else bg, environment)


def env_map():
    return np.random.default_rng(77).integers(0, 256, (16, 32, 3)).astype(np.uint8)


def _soup(name):
    """A soup as test_randomised_scenes_match_oracle makes them (texture coordinates in [-1, 2), images of random bytes, normal
    maps mostly "up"), with the textures dealt by TABLES[name]."""
    seed = SOUP_SEEDS[name]
    rng = np.random.default_rng(seed)
    sd = pin_cases.random_triangle_scene(n=300, seed=seed, n_emissive_mats=3)
    images, tsrc = [], []
    for m, row in zip(sd.materials[:6], TABLES[name]):
        for field, on in zip(KINDS, row):
            if not on:
                continue
            w, h = SIZES[len(images) % len(SIZES)]
            img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            if field == "normal_texture":
                img = np.clip(img // 4 + np.array([96, 96, 180]), 0, 255).astype(np.uint8)
            images.append(img)
            tsrc.append(len(images) - 1)
            setattr(m, field, len(tsrc) - 1)
    return rt.SceneData(sd.positions, sd.texcoords, sd.normals, sd.tangents, sd.material_index, list(sd.materials)[:sd.n_materials],
                        tsrc, images, sd.camera, (0.05, 0.07, 0.1), None)


# ---- texture_edges: camera-facing quads, one material and one uv layout each, dealt by this table ---------------------------------
# name: (uv of the quad's four corners (x0y0, x1y0, x1y1, x0y1), or one uv per triangle when "constant"; {kind: image}; tangent w;
# "parallel" = the tangent is the normal; emission factor).  Images are named: a texture_cases size, or a constant colour.
def _uv_box(u0, v0, u1, v1):
    return ((u0, v0), (u1, v0), (u1, v1), (u0, v1))


EDGE_ROWS = (
    ("uv_on_0_and_1", _uv_box(0, 0, 1, 1), {"base_color_texture": (3, 5)}, 1, False, 0),
    ("uv_negative", _uv_box(-3, -3, -2, -2), {"base_color_texture": (17, 13), "metallic_roughness_texture": (2, 2)}, 1, False, 0),
    ("uv_times_1e4", _uv_box(0, 0, 1e4, 1e4), {"base_color_texture": (32, 32), "metallic_roughness_texture": (3, 5)}, 1, False, 0),
    ("uv_constant", "constant", {"base_color_texture": (2, 2), "emissive_texture": (3, 5)}, 1, False, 0.5),
    ("image_1x1", _uv_box(-0.5, -0.5, 1.5, 1.5), {"base_color_texture": (1, 1), "metallic_roughness_texture": (1, 1)}, 1, False, 0),
    ("image_1x7", _uv_box(0, 0, 1, 1), {"base_color_texture": (1, 7)}, 1, False, 0),
    ("image_7x3", _uv_box(0, 0, 2, 2), {"base_color_texture": (7, 3), "normal_texture": "up"}, 1, False, 0),
    ("image_255x3", _uv_box(0, 0, 1, 1), {"base_color_texture": (255, 3), "metallic_roughness_texture": (255, 3)}, 1, False, 0),
    ("normal_128_128_255", _uv_box(0, 0, 1, 1), {"normal_texture": (128, 128, 255)}, 1, False, 0),
    ("normal_grey", _uv_box(0, 0, 3, 3), {"normal_texture": "grey"}, 1, False, 0),
    ("tangent_w_minus_1", _uv_box(0, 0, 1, 1), {"normal_texture": "up", "base_color_texture": (7, 1)}, -1, False, 0),
    ("tangent_parallel", _uv_box(0, 0, 1, 1), {"normal_texture": "up"}, 1, True, 0),
    ("emitter", _uv_box(0, 0, 1, 1), {"emissive_texture": (7, 1)}, 1, False, 6),
    ("plain", _uv_box(0, 0, 1, 1), {}, 1, False, 0),
    ("plain_emitter", _uv_box(0, 0, 1, 1), {}, 1, False, 3),
    ("all_four", _uv_box(-1, -1, 2, 2), {"base_color_texture": (17, 13), "emissive_texture": (32, 32), "metallic_roughness_texture": (7, 3),
                                         "normal_texture": "up"}, 1, False, 1),
)


def _edge_image(name, rng):
    import texture_cases
    if name == "up":                        # a normal map that mostly points up, as _soup's
        return np.clip(rng.integers(0, 256, (5, 5, 3)) // 4 + np.array([96, 96, 180]), 0, 255).astype(np.uint8)
    if name == "grey":                      # 127 and 128 in turn: 2 * sample - 1 is about +-0.004 per channel, and crosses 0 between texels
        g = np.where((np.arange(16).reshape(4, 4) + np.arange(4)[:, None]) % 2, 127, 128)
        return np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8)
    if len(name) == 3:
        return np.tile(np.array(name, np.uint8), (2, 2, 1))
    return texture_cases.images()[1 + texture_cases.IMAGE_SIZES.index(name)]


def _texture_edges():
    """A 4 x 4 grid of quads that fills the 48 x 32 frame, each a little tilted and offset in depth so that bounces meet other quads."""
    rng = np.random.default_rng(213)
    cam = rt.rt_camera()
    cam.position, cam.right, cam.up, cam.forward, cam.fov_y = (0, 0, 6), (1, 0, 0), (0, 1, 0), (0, 0, -1), 0.9
    pos, uvs, nrm, tan, mat_idx, mats, images, tsrc = [], [], [], [], [], [], [], []
    for q, (name, uv, kinds, tanw, parallel, emit) in enumerate(EDGE_ROWS):
        cx, cy = -3.3 + 2.2 * (q % 4), -2.1 + 1.4 * (q // 4)
        ax, ay = rng.uniform(-0.35, 0.35, 2)
        rot = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]) @ \
            np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        centre = np.array([cx, cy, rng.uniform(-0.6, 0.6)])
        corner = [centre + rot @ np.array([sx * 1.08, sy * 0.68, 0]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        n, t = np.float32(rot @ np.array([0, 0, 1.0])), np.float32(rot @ np.array([1.0, 0, 0]))
        if parallel:
            t = n
        for tri, const in (((0, 1, 2), (0.25, 0.75)), ((0, 2, 3), (-1.5, 3.0))):
            pos.append(np.concatenate([corner[k] for k in tri]))
            uvs.append(np.tile(const, 3) if uv == "constant" else np.concatenate([uv[k] for k in tri]))
            nrm.append(np.tile(n, 3))
            tan.append(np.tile(np.append(t, tanw), 3))
            mat_idx.append(q)
        m = rt.rt_material()
        m.base_color = tuple(rng.uniform(0.3, 1, 3).astype(np.float32))
        m.emission = (emit, emit * 0.8, emit * 0.6)
        m.metallic_factor, m.roughness_factor = float(np.float32(rng.uniform(0, 1))), float(np.float32(rng.uniform(0.1, 1)))
        for kind in KINDS:
            setattr(m, kind, -1)
            if kind in kinds:
                images.append(_edge_image(kinds[kind], rng))
                tsrc.append(len(images) - 1)
                setattr(m, kind, len(tsrc) - 1)
        mats.append(m)
    return rt.SceneData(np.float32(pos), np.float32(uvs), np.float32(nrm), np.float32(tan), np.uint32(mat_idx), mats, tsrc, images, cam,
                        (0.3, 0.35, 0.4), None)


_gltf = lambda name: rt.load_gltf(os.path.join(pin_cases.SCENES, "hw8_sphere", name + ".gltf"))
BUILDERS = {"sphere": lambda: _gltf("sphere"), "sphere_emissive": lambda: _gltf("sphere_emissive"), "sphere_roughness": lambda: _gltf("sphere_roughness"),
            "soup_a": lambda: _soup("soup_a"), "soup_b": lambda: _soup("soup_b"),
            "sphere_emissive_env": lambda: _with(_gltf("sphere_emissive"), env_map()),
            "sphere_env": lambda: _with(_gltf("sphere"), env_map()),
            "soup_a_env": lambda: _with(_soup("soup_a"), env_map()),
            "sphere_roughness_env": lambda: _with(_gltf("sphere_roughness"), env_map()), "soup_b_env": lambda: _with(_soup("soup_b"), env_map()),
            "texture_edges": _texture_edges}


@functools.lru_cache(maxsize=None)
def scene_data(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    return oracle_lib.Hw8Oracle(scene_data(name))


@functools.lru_cache(maxsize=None)
def traced_frame(name, w, h):
    """Per pixel of a w x h frame at one sample and depth 1, the oracle's camera ray and whether it hit: (o, d, hit), (h * w, 3) each
    and (h * w,) bool, in frame order."""
    L = oracle_lib.lib()
    L.rto_hw8_trace_pixel.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int]
    rec = np.zeros((h * w, 12), np.float32)
    for y in range(h):
        for x in range(w):
            assert L.rto_hw8_trace_pixel(oracle(name)._h, w, h, 1, 1, x, y, rec[y * w + x].ctypes.data, 12) == 12
    rec.setflags(write=False)
    return rec[:, 0:3], rec[:, 3:6], rec[:, 7] >= 0


def jitter(w, h):
    """The renderer's first two draws per pixel: nx = x + u1, ny = y + u2 with the engine seeded y * w + x; (h * w, 2) float32."""
    L = oracle_lib.lib()
    xy = np.zeros((h * w, 2), np.float32)
    u = np.zeros(2, np.float32)
    for y in range(h):
        for x in range(w):
            L.rto_rng_kat(y * w + x, 2, 0, u.ctypes.data)
            xy[y * w + x] = np.float32(x) + u[0], np.float32(y) + u[1]
    return xy


def centres(w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return np.stack([x.reshape(-1) + np.float32(0.5), y.reshape(-1) + np.float32(0.5)], axis=1)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def first_difference(a, b):
    rows = np.nonzero(np.any(a != b, axis=1))[0]
    return f"{len(rows)} of {len(a)} differ, first {rows[:5].tolist()}: {a[rows[0]].tolist()} != {b[rows[0]].tolist()}" if len(rows) else ""

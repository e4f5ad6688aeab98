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


_gltf = lambda name: rt.load_gltf(os.path.join(pin_cases.SCENES, "hw8_sphere", name + ".gltf"))
BUILDERS = {"sphere": lambda: _gltf("sphere"), "sphere_emissive": lambda: _gltf("sphere_emissive"), "sphere_roughness": lambda: _gltf("sphere_roughness"),
            "soup_a": lambda: _soup("soup_a"), "soup_b": lambda: _soup("soup_b"),
            "sphere_emissive_env": lambda: _with(_gltf("sphere_emissive"), env_map()),
            "sphere_env": lambda: _with(_gltf("sphere"), env_map()),
            "soup_a_env": lambda: _with(_soup("soup_a"), env_map())}


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

"""Scenes and ray sets with a known number of light hits per ray, for pinning light-pdf sums to the reference by hit count.

A light-pdf query adds one float term per emissive triangle the ray hits, in the shape of the reference's light tree.  stack_scene piles
L emissive quads along z, so a ray along z hits any number of them from 0 to L (and 2 L triangles where it runs in the plane of the
quads' shared diagonals); hit_terms gives each ray's terms one light at a time, which says how many hits a sum has and what its plain
left fold would be.  tests/test_light_sum_cases.py holds the conditions on these inputs and the oracle to the compiled reference
(tests/golden/pins_light_sums.npz); tests/test_gpu_light_sums.py and tests/test_gpu_light_sums_hw6.py hold the kernels to both."""
import functools
import importlib

import numpy as np

import oracle_lib
import pin_cases

rt = importlib.import_module("raytracing-course-hw_amd")

SEED = 1
HW8_LAYERS = (2, 5, 6, 12)         # 2: a tree of at most 4 lights (pseudo depths inside a leaf); 5 | 6: either side of WF_MAX_LIGHT_HITS
HW6_LAYERS = (3, 4, 13, 16, 20)    # inline 3 and 4; 13 | 14: P6_MERGE_HITS ends; 16 | 17: RT6_MAX_LIGHT_HITS ends
# hw6 frames beyond the boundaries: (layers, seed) on which the inline three- and four-hit additions of P6LightWalk::end take outcomes that
# the L = 3 and L = 4 frames never reach (a census with a throwaway counter, profiles/r37_light_sums.txt: L = 4 takes one of the five)
HW6_OUTCOME_FRAMES = ((5, 3), (6, 1), (6, 2), (6, 3), (8, 2))
HW6_FRAMES = tuple((L, SEED) for L in HW6_LAYERS) + HW6_OUTCOME_FRAMES
RAY_SETS = ("through", "diagonal", "floor")
RAY_COUNTS = {"through": 1024, "diagonal": 256, "floor": 512}
FRAME = (32, 24, 8)                # width, height, samples of the rendered frames
FRAME_LAYERS = (5, 6, 12)          # hw8 scenes that are rendered as well


def _material(base, emission, hw6):
    m = rt.rt_material()
    m.base_color, m.emission = tuple(base), tuple(emission)
    m.metallic_factor, m.roughness_factor = 0.0, 1.0
    m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = m.normal_texture = -1
    if hw6:
        m.kind, m.ior = 0, 1.5
    return m


@functools.lru_cache(maxsize=None)
def stack_scene(L, seed=SEED, hw6=False):
    """L emissive quads (two triangles each, sharing the diagonal from corner 0 to corner 2) stacked along z at irregular spacing, each a
    [-1,1]^2 square scaled by 0.8 .. 1.6 with every corner's z jittered by +-0.05, over a diffuse floor [-3,3]^2 at z = -1; the camera at
    (0.2, 0.1, -0.9) looks along +z.  The emissive triangles come first in LOAD order: triangles 2 i and 2 i + 1 are layer i."""
    rng = np.random.default_rng(seed)
    z = np.cumsum(rng.uniform(0.15, 1.2, L))
    scale = rng.uniform(0.8, 1.6, L)
    jitter = rng.uniform(-0.05, 0.05, (L, 4))
    square = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
    tris = []
    for i in range(L):
        c = np.concatenate([square * scale[i], (z[i] + jitter[i])[:, None]], axis=1)
        tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    f = np.concatenate([square * 3, np.full((4, 1), -1.0)], axis=1)
    tris += [f[[0, 1, 2]], f[[0, 2, 3]]]
    tri = np.array(tris).astype(np.float32)
    n = len(tri)
    mats = [_material((0.7, 0.7, 0.7), (2.0, 1.5, 1.0), hw6), _material((0.6, 0.5, 0.4), (0, 0, 0), hw6)]
    mat_idx = np.array([0] * (2 * L) + [1, 1], np.uint32)
    cam = rt.rt_camera()
    cam.position, cam.right, cam.up, cam.forward = (0.2, 0.1, -0.9), (1, 0, 0), (0, 1, 0), (0, 0, 1)
    cam.fov_y = 1.2
    if hw6:
        return rt.SceneData(tri.reshape(n, 9), None, None, None, mat_idx, mats, camera=cam, bg=(0.1, 0.2, 0.3))
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.repeat(pin_cases.unit(np.cross(e1.astype(np.float64), e2.astype(np.float64)))[:, None, :], 3, axis=1)
    tan = np.tile(np.array([1, 0, 0, 1], np.float32), (n, 3, 1))
    uv = np.zeros((n, 3, 2), np.float32)
    return rt.SceneData(tri.reshape(n, 9), uv.reshape(n, 6), nrm.reshape(n, 9), tan.reshape(n, 12), mat_idx, mats, camera=cam)


def layer_range(sd):
    """(lowest, highest) z of the emissive triangles."""
    z = sd.positions.reshape(-1, 3, 3)[:-2, :, 2]
    return float(z.min()), float(z.max())


@functools.lru_cache(maxsize=None)
def rays(L, which, seed=SEED):
    """(o, d) of a ray set on stack_scene(L, seed), float32, read-only.
    through    origins with x, y in +-0.4 and z from below the first layer to the last, directions (+-0.08, +-0.08, +-1) normalised: sums
               that start in the middle of the stack, from either side of the quads
    diagonal   the same with o.x == o.y and d.x == d.y: the ray lies in the plane of the shared diagonals, so the reference's own edge
               rule decides whether a layer counts twice, once or not at all
    floor      origins 1e-4 above the floor, cosine-like directions upwards: the rays a render sends"""
    sd = stack_scene(L, seed)
    z0, z1 = layer_range(sd)
    n = RAY_COUNTS[which]
    rng = np.random.default_rng(1000 * seed + 10 * L + RAY_SETS.index(which))
    if which == "floor":
        o = np.concatenate([rng.uniform(-3, 3, (n, 2)), np.full((n, 1), -1 + 1e-4)], axis=1)
        r, phi = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        d = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(1e-6, 1 - r * r))], axis=1)
    else:
        o = np.concatenate([rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(z0 - 0.5, z1, (n, 1))], axis=1)
        d = np.concatenate([0.08 * rng.choice([-1.0, 1.0], (n, 2)), rng.choice([-1.0, 1.0], (n, 1))], axis=1)
        if which == "diagonal":
            o[:, 1], d[:, 1] = o[:, 0], d[:, 0]
    o, d = o.astype(np.float32), pin_cases.unit(d)
    if which == "diagonal":
        assert np.array_equal(o[:, 0], o[:, 1]) and np.array_equal(d[:, 0], d[:, 1])
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def light_pdfs(impl, o, d):
    """impl.light_pdf over the rays, float32."""
    return np.array([impl.light_pdf(o[i], d[i]) for i in range(len(o))], np.float32)


def _single_light(sd, tri):
    """The scene that holds triangle `tri` of sd alone."""
    pick = lambda a, k: None if a is None else a[tri:tri + 1]
    return rt.SceneData(sd.positions[tri:tri + 1], pick(sd.texcoords, 6), pick(sd.normals, 9), pick(sd.tangents, 12), np.zeros(1, np.uint32),
                        [sd.materials[int(sd.material_index[tri])]], camera=sd.camera)


def hit_terms(sd, o, d):
    """Each ray's light-pdf terms, one column per light in the reference's light order (n x lights, float32; 0 = not hit): the light pdf
    of the one-light scene that holds the light alone.  The full scene's sum is these terms added in the shape of its light tree, then
    divided by the light count; a ray's hit count is the number of its non-zero terms."""
    order = oracle_lib.Hw8Oracle(sd).light_order()
    terms = np.zeros((len(o), len(order)), np.float32)
    for j, tri in enumerate(order):
        one = _single_light(sd, int(tri))
        terms[:, j] = light_pdfs(oracle_lib.Hw8Oracle(one), o, d)
    return terms


@functools.lru_cache(maxsize=None)
def terms_of(L, which, seed=SEED):
    t = hit_terms(stack_scene(L, seed), *rays(L, which, seed))
    t.setflags(write=False)
    return t


def hit_counts(terms):
    return (terms != 0).sum(axis=1)


def left_fold(terms):
    """The plain left fold of each ray's non-zero terms in reference light order, divided by the light count: float32 throughout."""
    acc = np.zeros(len(terms), np.float32)
    for j in range(terms.shape[1]):
        acc = np.where(terms[:, j] != 0, acc + terms[:, j], acc).astype(np.float32)
    return (acc / np.float32(terms.shape[1])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_pdfs(L, which, seed=SEED):
    """Hw8Oracle.light_pdf over a ray set, computed once and shared."""
    out = light_pdfs(oracle_lib.Hw8Oracle(stack_scene(L, seed)), *rays(L, which, seed))
    out.setflags(write=False)
    return out


def fixture_key(L, which):
    return f"L{L}_{which}"

"""The inputs on which the texture layer (hw8/src/scene.cpp:9-53: sampleTexture, loadSingleFromTexture, applyNormalMaps) is pinned at its
edges: one table for the golden generator (golden/make_goldens.py -> pins_texture_edges.npz), the host pin (test_texture_pins.py) and the
GPU test (test_gpu_texture.py).  Everything is deterministic: fixed seeds, float32 arrays built from bit-exact operations.  A family is a
dict of arrays with one row per case.

families()   texel        slot, uv, srgb     every byte value through a tap with dx == dy == 0: the tap is the texel
             tap          slot, uv, srgb     every image of IMAGE_SIZES and the environment map, uv on and beside every texel boundary
             past_end     slot, uv, srgb     the rows of tap whose wrapped coordinate times the size rounds up to the size itself
             nonfinite    slot, uv, srgb     NaN and infinities in either coordinate (oracle and device only: the reference converts NaN to int)
             normal_map   rows               sn 3, tangent 4 (xyz, w), sample 3

All images live in ONE scene (scene_data()): slot i is image i of IMAGES, slot -1 is the environment map."""
import ctypes as C
import functools

import numpy as np

import oracle_lib

F = np.float32
rt = oracle_lib.rt
# (w, h).  The ramp first: its 256 texels hold every byte value in every channel.  7x3 last, and again as the environment map, which scene
# preparation stores behind the images: 63 bytes are 15 (mod 16), so the fourth byte of the 4-byte load of its last texel is the single
# spare byte at the end of the texel array.
IMAGE_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 13), (32, 32), (255, 3), (1000, 3), (7, 3))
ENV_SIZE = (7, 3)
ENV = -1
REFERENCE_FAMILIES = ("texel", "tap", "past_end", "normal_map")
DENORM = 1e-45


@functools.lru_cache(maxsize=None)
def images():
    """Slot 0 the ramp, then IMAGE_SIZES in order; (h, w, 3) uint8 each."""
    b = np.arange(256)
    ramp = np.stack([b, 255 - b, (b * 7 + 3) % 256], axis=1).astype(np.uint8).reshape(1, 256, 3)
    rng = np.random.default_rng(3301)
    out = [ramp] + [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in IMAGE_SIZES]
    for im in out:
        im.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def env_image():
    im = np.random.default_rng(3302).integers(0, 256, (ENV_SIZE[1], ENV_SIZE[0], 3)).astype(np.uint8)
    im.setflags(write=False)
    return im


def image_of(slot):
    return env_image() if slot < 0 else images()[slot]


@functools.lru_cache(maxsize=None)
def scene_data():
    """The geometry of a triangle soup (its materials untextured) with every image of the table and the environment map: what the device's
    tap hook works over."""
    import pin_cases
    sd = pin_cases.random_triangle_scene(n=300, seed=3305)
    return rt.SceneData(sd.positions, sd.texcoords, sd.normals, sd.tangents, sd.material_index, list(sd.materials)[:sd.n_materials],
                        list(range(len(images()))), list(images()), sd.camera, (0, 0, 0), env_image())


def _neighbours(v):
    v = np.asarray(v, F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))])


def _boundaries(size, rng):
    """The k of k / size: all of them for a small image; for a large one both ends, the middle and 24 drawn ones."""
    if size <= 32:
        return np.arange(size + 1)
    drawn = rng.integers(3, size - 2, 24)
    return np.unique(np.concatenate([[0, 1, 2, size // 2, size - 2, size - 1, size], drawn]))


SPECIAL = F([0.0, -0.0, DENORM, -DENORM, 1e-8, -1e-8, 1.0, -1.0, 1e6 + 0.5, -(1e6 + 0.5), 8388607.5, 2.0 ** 24, 1e30])


def _axis_values(size, rng):
    """Per axis: k / size and its two float neighbours, the same shifted by +1, -1 and -2 (float additions), and SPECIAL."""
    base = _neighbours(F(_boundaries(size, rng)) / F(size))
    return np.concatenate([base, base + F(1), base - F(1), base - F(2), SPECIAL]).astype(F)


def _tap():
    rng = np.random.default_rng(3303)
    slot, uv, srgb = [], [], []
    for s in list(range(1, len(images()))) + [ENV]:
        h, w = image_of(s).shape[:2]
        xs, ys = _axis_values(w, rng), _axis_values(h, rng)
        # every value of one axis against a walk through the other's, so that each boundary of x meets several of y and the reverse
        a = np.stack([xs, ys[(np.arange(len(xs)) * 7 + 3) % len(ys)]], axis=1)
        b = np.stack([xs[(np.arange(len(ys)) * 11 + 5) % len(xs)], ys], axis=1)
        corners = np.stack(np.meshgrid(SPECIAL, SPECIAL), axis=-1).reshape(-1, 2)
        r = rng.uniform(-2, 2, (120, 2)).astype(F)
        rows = np.concatenate([a, b, corners, r]).astype(F)
        # both curves on every row of a small image; alternating on the two large ones
        flags = (0, 1) if max(w, h) <= 32 else (None,)
        for f in flags:
            slot.append(np.full(len(rows), s, np.int32))
            uv.append(rows)
            srgb.append(np.full(len(rows), f, np.int32) if f is not None else (np.arange(len(rows)) % 2).astype(np.int32))
    return {"slot": np.concatenate(slot), "uv": np.ascontiguousarray(np.concatenate(uv), F), "srgb": np.concatenate(srgb)}


def _texel():
    b = np.arange(256)
    uv = np.stack([F(b) / F(256), np.zeros(256, F)], axis=1)        # k / 256 * 256 == k exactly: dx == 0; 0 * 1 == 0: dy == 0
    return {"slot": np.zeros(512, np.int32), "uv": np.ascontiguousarray(np.concatenate([uv, uv]), F), "srgb": np.repeat([0, 1], 256).astype(np.int32)}


def wrapped_index(u, size):
    """scene.cpp:19-29 in float32, one axis: the index floor((u - floor(u)) * size) and the fraction behind it."""
    with np.errstate(all="ignore"):
        u = np.asarray(u, F)
        t = (u - np.floor(u)).astype(F) * F(size)
        i = np.floor(t)
        return i.astype(np.int64), (t - i).astype(F)


def sizes_of(slot):
    wh = np.array([image_of(int(s)).shape[1::-1] for s in range(-1, len(images()))])      # row 0 is the environment map
    return wh[np.asarray(slot) + 1]


def past_end_mask(fam):
    wh = sizes_of(fam["slot"])
    ix, _ = wrapped_index(fam["uv"][:, 0], wh[:, 0])
    iy, _ = wrapped_index(fam["uv"][:, 1], wh[:, 1])
    return (ix == wh[:, 0]) | (iy == wh[:, 1])


def _nonfinite():
    bad = F([np.nan, np.inf, -np.inf, -np.nan])
    fine = F([0.25, -0.75, 0.0, 1e6])
    slot, uv, srgb = [], [], []
    for k in range(60):
        s = (1 + k % len(IMAGE_SIZES)) if k % 6 else ENV
        a, b = bad[k % 4], (fine[(k // 4) % 4] if k % 5 else bad[(k // 5) % 4])
        slot.append(s), uv.append((a, b) if k % 2 else (b, a)), srgb.append(k % 3 == 0)
    return {"slot": np.array(slot, np.int32), "uv": np.ascontiguousarray(uv, F), "srgb": np.array(srgb, np.int32)}


def _unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(F)


LATTICE = F([[128, 128, 255], [127, 127, 127], [128, 128, 128], [0, 0, 0], [255, 255, 255], [255, 0, 128], [0, 255, 127]]) / F(255)
SAMPLES = np.concatenate([LATTICE, F([[0.5, 0.5, 1.0], [0.5, 0.5, 0.5]])])          # the default, and the one whose local normal is 0


def _normal_map():
    """sn and the tangent unit, non-unit, zero, parallel and antiparallel; tanw +-1, +-0 and 2; samples on the k / 255 lattice, the default
    (0.5, 0.5, 1), (0.5, 0.5, 0.5) whose local normal is 0 (normalize answers NaN), blends as a bilinear tap gives them, random ones."""
    rng = np.random.default_rng(3304)
    n = 4000
    sn = _unit(rng.normal(0, 1, (n, 3)))
    tan = _unit(rng.normal(0, 1, (n, 3)))
    kind = np.arange(n) % 16
    perp = kind < 6                                                     # a proper frame: the tangent orthogonal to sn, then rounded
    t64 = tan[perp].astype(np.float64) - (tan[perp].astype(np.float64) * sn[perp]).sum(axis=1, keepdims=True) * sn[perp]
    tan[perp] = _unit(t64)
    tan[kind == 6] = sn[kind == 6]                                      # parallel
    tan[kind == 7] = -sn[kind == 7]                                     # antiparallel
    tan[kind == 8] = 0                                                  # zero tangent
    sn[kind == 9] = 0                                                   # zero normal
    sn[kind == 10] *= rng.uniform(0.5, 2, ((kind == 10).sum(), 1)).astype(F)      # non-unit
    tan[kind == 11] *= rng.uniform(1e-3, 1e3, ((kind == 11).sum(), 1)).astype(F)
    sn[kind == 12] *= F(1e-20)                                          # the squared length underflows
    tan[kind == 13] *= F(1e20)                                          # and overflows
    tanw = F([1, -1, 1, -1, 0.0, -0.0, 2, 1])[(np.arange(n) // 16) % 8]
    which = (np.arange(n) // 3) % 4
    sample = np.zeros((n, 3), F)
    lat = SAMPLES[rng.integers(0, len(SAMPLES), n)]
    a, b = LATTICE[rng.integers(0, len(LATTICE), n)], LATTICE[rng.integers(0, len(LATTICE), n)]
    dx = rng.uniform(0, 1, (n, 1)).astype(F)
    blend = (F(1) - dx) * a + dx * b                                    # as the last line of a tap blends two texels
    up = np.clip(rng.integers(96, 160, (n, 3)) + np.array([0, 0, 96]), 0, 255).astype(F) / F(255)      # a normal map that mostly points up
    anyv = rng.uniform(0, 1, (n, 3)).astype(F)
    for k, src in enumerate((lat, blend, up, anyv)):
        sample[which == k] = src[which == k]
    flat = np.arange(n) % 97 == 0                                       # the local normal exactly 0 on every kind of frame
    sample[flat] = F([0.5, 0.5, 0.5])
    return {"rows": np.ascontiguousarray(np.concatenate([sn, tan, tanw[:, None], sample], axis=1), F)}


@functools.lru_cache(maxsize=None)
def families():
    tap = _tap()
    m = past_end_mask(tap)
    out = {"texel": _texel(), "tap": tap, "past_end": {k: np.ascontiguousarray(v[m]) for k, v in tap.items()}, "nonfinite": _nonfinite(),
           "normal_map": _normal_map()}
    for fam in out.values():
        for a in fam.values():
            a.setflags(write=False)
    return out


def _p(a):
    return a.ctypes.data


def taps(fn, fam):
    """fn(w, h, data, tx, ty, srgb, out3) -- rto_sample_texture or ref8_sample_texture -- on the rows of a tap family: n x 3."""
    fn.argtypes, fn.restype = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p], None
    out = np.zeros((len(fam["slot"]), 3), F)
    for i, (s, (u, v), f) in enumerate(zip(fam["slot"], fam["uv"], fam["srgb"])):
        im = image_of(int(s))
        fn(im.shape[1], im.shape[0], _p(im), u, v, int(f), _p(out[i]))
    return out


def normal_maps(fn, rows):
    """fn(sn3, tan4, sample3, out3) -- rto_apply_normal_map or ref8_apply_normal_map -- on the rows of normal_map: n x 3."""
    fn.argtypes, fn.restype = [C.c_void_p] * 4, None
    rows = np.ascontiguousarray(rows, F)
    out = np.zeros((len(rows), 3), F)
    for i in range(len(rows)):
        fn(_p(rows[i]), _p(rows[i, 3:]), _p(rows[i, 7:]), _p(out[i]))
    return out


def ref_scene_lib():
    p = oracle_lib.ref_path("libref_hw8_scene.so")
    if p is None:
        raise FileNotFoundError("oracle/_ref/libref_hw8_scene.so not built")
    return C.CDLL(p)


def evaluate(which):
    """The answers of the oracle ("oracle": every family) or of the compiled reference ("reference": REFERENCE_FAMILIES)."""
    fams = families()
    L = oracle_lib.lib() if which == "oracle" else ref_scene_lib()
    tap_fn = L.rto_sample_texture if which == "oracle" else L.ref8_sample_texture
    nm_fn = L.rto_apply_normal_map if which == "oracle" else L.ref8_apply_normal_map
    out = {name: taps(tap_fn, fams[name]) for name in ("texel", "tap", "past_end") + (("nonfinite",) if which == "oracle" else ())}
    out["normal_map"] = normal_maps(nm_fn, fams["normal_map"]["rows"])
    return out


@functools.lru_cache(maxsize=None)
def oracle_answers():
    out = evaluate("oracle")
    for a in out.values():
        a.setflags(write=False)
    return out


def model_tap(fam, lut):
    """A tap restated in numpy float32 with the texels past the end of an image read as 0: scene.cpp:9-35 on flat texel arrays.  lut: (2,
    256) float32, the value of byte b under each curve (the reference's answers to the texel family).  n x 3."""
    out = np.zeros((len(fam["slot"]), 3), F)
    wh = sizes_of(fam["slot"])
    ix1, dx = wrapped_index(fam["uv"][:, 0], wh[:, 0])
    iy1, dy = wrapped_index(fam["uv"][:, 1], wh[:, 1])
    ix2, iy2 = (ix1 + 1) % wh[:, 0], (iy1 + 1) % wh[:, 1]
    for i, s in enumerate(fam["slot"]):
        flat = image_of(int(s)).reshape(-1, 3)
        w = wh[i, 0]

        def texel(ix, iy):
            k = ix + w * iy
            return lut[fam["srgb"][i]][flat[k]] if k < len(flat) else np.zeros(3, F)
        one = F(1)
        left = (one - dy[i]) * texel(ix1[i], iy1[i]) + dy[i] * texel(ix1[i], iy2[i])
        right = (one - dy[i]) * texel(ix2[i], iy1[i]) + dy[i] * texel(ix2[i], iy2[i])
        out[i] = (one - dx[i]) * left + dx[i] * right
    return out


# ---- the hits of the camera set on the scene `texture_edges` (surface_cases.py), for the first-hit layer's test ----------------------
def edge_hits():
    """The oracle's rt_hit records of test_gpu_query's camera set on texture_edges (its closest hits are pinned to the reference's by
    test_oracle_pins.py and to the device's by test_gpu_query.py)."""
    import surface_cases
    import test_gpu_query as tq
    sd = surface_cases.scene_data("texture_edges")
    o, d = tq._camera_rays(sd)
    return tq._expected_hits(surface_cases.oracle("texture_edges"), sd, o, d)


def edge_taps(fn, hits):
    """Per hit, the taps of its material's four texture kinds (surface_cases.KINDS order, sRGB for the first two) at the hit's texcoord
    through fn (as taps()); zeros where the material has no such texture or the ray missed: n x 4 x 3."""
    import surface_cases
    sd = surface_cases.scene_data("texture_edges")
    fn.argtypes, fn.restype = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p], None
    out = np.zeros((len(hits), 4, 3), F)
    for i, h in enumerate(hits):
        if h["triangle"] == surface_cases.MISS:
            continue
        m = sd.materials[int(sd.material_index[h["triangle"]])]
        for k, kind in enumerate(surface_cases.KINDS):
            t = getattr(m, kind)
            if t >= 0:
                im = sd.images[int(sd.texture_source[t])]
                fn(im.shape[1], im.shape[0], _p(im), h["texcoord"][0], h["texcoord"][1], int(k < 2), _p(out[i, k]))
    return out

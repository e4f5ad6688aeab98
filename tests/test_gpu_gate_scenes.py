"""The exactness gate at work: constructed scenes through the query calls and two render pipelines.

test_gpu_intersection.py checks the gate's arithmetic on rows; here whole scenes are built so that its hard cases are the common ones:
  walls        an axis-aligned room with a face at coordinate 0, tessellated walls (quads sharing edges and vertices), stacks of coplanar
               quads and exact duplicates inside: every triangle's box is flat, every hit lies in a face of its box
  walls_far    the same translated by (1000, -1000, 1000): the rounding is that of the large coordinates
  walls_small  the same scaled by 1e-3
  tripwired    a soup plus 12 triangles whose normal is perpendicular to magic1 x magic2 within |cos| < 2^-16 (their test accepts points
               far from the triangle), each with an ordinary triangle between its leaf box and the rays' origins
262,144 rays per scene (fixed seeds, one chunk): aimed at shared edges and vertices, grazing inside a wall's plane within a few ulp,
starting on a surface (1e-4 off it and not at all) and pointing into it and along it, short rays (t from 1e-5 to 1e-2), and a quarter
camera-like rays.  rt_query_closest, rt_query_occluded and rt_query_light_pdf answer as their forced reference walks do, and as
Hw8Oracle (and Ref8 where oracle/_ref is built) on 2,048 of the rays; each scene renders bit-exactly on the default pipeline and on
the round pipeline with exact re-walks, which puts the persistent walkers on the same geometry."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import intersection_cases as ic
import oracle_lib
import pin_cases
from test_gpu_query import MISS, _camera_rays, _expected_hits, _first_difference, _words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_RAYS = 262144
N_ORACLE = 1024
TRIPWIRE_COS = 2.0 ** -14                       # RTAMD_TRIPWIRE_COS's default (host/scene_prep.cpp)
SCENE_NAMES = ("walls", "walls_far", "walls_small", "tripwired")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _quad(axis, at, lo, hi):
    """Two triangles of the axis-aligned rectangle [lo, hi] (two coordinates) in the plane coordinate `axis` = at; they share a diagonal."""
    u, v = [k for k in range(3) if k != axis]
    c = np.zeros((4, 3), F)
    c[:, axis] = at
    c[:, u] = (lo[0], hi[0], hi[0], lo[0])
    c[:, v] = (lo[1], lo[1], hi[1], hi[1])
    return [c[[0, 1, 2]], c[[0, 2, 3]]]


def _walls_triangles():
    g = [np.arange(5, dtype=F), F(0.75) * np.arange(5, dtype=F), F(1.3) * np.arange(5, dtype=F)]     # the room [0, 4] x [0, 3] x [0, 5.2]
    tris = []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for at in (g[axis][0], g[axis][4]):                              # the six walls, 4 x 4 quads each
            for i in range(4):
                for j in range(4):
                    tris += _quad(axis, at, (g[u][i], g[v][j]), (g[u][i + 1], g[v][j + 1]))
    inner = []
    inner += _quad(2, g[2][2], (g[0][1], g[1][1]), (g[0][3], g[1][3]))   # a stack in the plane z = 2.6: a large quad,
    inner += _quad(2, g[2][2], (g[0][1], g[1][1]), (g[0][2], g[1][2]))   # a quarter of it in the same plane,
    inner += _quad(2, g[2][2], (g[0][2], g[1][1]), (g[0][3], g[1][2]))   # its neighbour (a shared edge),
    inner += _quad(2, g[2][2], (g[0][2], g[1][2]), (g[0][3], g[1][3]))   # and one that shares a vertex with the quarter
    inner += _quad(0, g[0][2], (g[1][1], g[2][1]), (g[1][3], g[2][3]))   # crossing stacks in x = 2 and y = 1.5
    inner += _quad(0, g[0][2], (g[1][1], g[2][1]), (g[1][2], g[2][2]))
    inner += _quad(1, g[1][2], (g[0][1], g[2][1]), (g[0][3], g[2][3]))
    inner += _quad(1, g[1][2], (g[0][2], g[2][2]), (g[0][3], g[2][3]))
    inner += _quad(2, g[2][1], (g[0][0], g[1][0]), (g[0][4], g[1][4]))   # a sheet across the room: shares its rim with the walls
    tris += inner + inner[:6] + tris[:8] + inner[8:12]                   # exact duplicates: ties in t, settled by the figure order
    return np.stack(tris).astype(F)


def _scene_of(tris, cam_pos, cam_forward, seed):
    """SceneData around the triangles the way pin_cases.random_triangle_scene makes one: random normals, tangents, texcoords, six
    materials of which two are emissive."""
    n = len(tris)
    rng = np.random.default_rng(seed)
    nrm = pin_cases.unit(rng.normal(0, 1, (n, 3, 3)))
    tan = np.concatenate([pin_cases.unit(rng.normal(0, 1, (n, 3, 3))), np.sign(rng.normal(0, 1, (n, 3, 1))).astype(F)], axis=2)
    uv = rng.uniform(-1, 2, (n, 3, 2)).astype(F)
    rt = pin_cases.rt
    mats = []
    for i in range(6):
        m = rt.rt_material()
        m.base_color = tuple(rng.uniform(0.1, 1, 3).astype(F))
        m.emission = tuple((rng.uniform(0.5, 4, 3) if i < 2 else np.zeros(3)).astype(F))
        m.metallic_factor = float(F(rng.uniform(0, 1)))
        m.roughness_factor = float(F(rng.uniform(0.05, 1)))
        m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = m.normal_texture = -1
        mats.append(m)
    mat_idx = rng.integers(0, 6, n).astype(np.uint32)
    cam = rt.rt_camera()
    fwd = np.asarray(cam_forward, np.float64)
    right = np.cross(fwd, (0.0, 1.0, 0.0)) if abs(fwd[1]) < 0.9 else np.cross(fwd, (1.0, 0.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    cam.position, cam.right, cam.up, cam.forward = tuple(float(F(x)) for x in cam_pos), tuple(right), tuple(up), tuple(fwd)
    cam.fov_y = 1.1
    return rt.SceneData(tris.reshape(n, 9), uv.reshape(n, 6), nrm.reshape(n, 9), tan.reshape(n, 12), mat_idx, mats, camera=cam)


def near_singular_triangle(rng, centre, size, cos):
    """A triangle around `centre` whose normal makes the angle arccos(cos) with magic1 x magic2 (built in double, then rounded)."""
    k = ic.kernel_direction()
    e = ic.unit64(np.cross(k, rng.normal(size=3)))
    normal = cos * k + np.sqrt(1 - cos * cos) * e
    t1 = ic.unit64(k - np.dot(k, normal) * normal)                        # in the plane, as nearly along k as the plane allows
    t2 = np.cross(normal, t1)
    ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
    return (centre + size * (np.cos(ang)[:, None] * t1 + np.sin(ang)[:, None] * t2)).astype(F)


def float_cos(tris):
    """|cos| between each triangle's normal and magic1 x magic2 as the host's tripwire rule computes it: |den| / (|n| |k|), den and n
    the float32 values of make_isect (den = (magic1 x magic2) . n up to rounding)."""
    rec = ic.tri_records(np.concatenate([tris.reshape(-1, 9), np.zeros((len(tris), 6), F)], axis=1))
    nn = np.linalg.norm(rec["n"].astype(np.float64), axis=1)
    kn = np.linalg.norm(np.cross(ic.MAGIC1.astype(np.float64), ic.MAGIC2.astype(np.float64)))
    with np.errstate(all="ignore"):
        return np.where(nn > 0, np.abs(rec["den"].astype(np.float64)) / (nn * kn), np.inf)


N_WIRES = 12


@functools.lru_cache(maxsize=None)
def _tripwired_parts(cos):
    """The soup, the 12 near-singular triangles at |cos| = cos (0: as near perpendicular as rounding leaves them), their blockers, and per
    wire the side the rays come from."""
    rng = np.random.default_rng(8600)
    soup = pin_cases.random_triangle_scene(n=300, seed=31).positions.reshape(-1, 3, 3)
    centres = rng.uniform(-1.8, 1.8, (N_WIRES, 3))
    side = ic.unit64(rng.normal(size=(N_WIRES, 3)))
    wires = np.stack([near_singular_triangle(rng, centres[i], 0.45, cos * rng.choice([-1.0, 1.0])) for i in range(N_WIRES)])
    blockers = []
    for i in range(N_WIRES):                                             # an ordinary triangle across the way from the origins to the wire's box
        a = ic.unit64(np.cross(side[i], rng.normal(size=3)))
        b = np.cross(side[i], a)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        blockers.append((centres[i] + 1.1 * side[i] + 0.7 * (np.cos(ang)[:, None] * a + np.sin(ang)[:, None] * b) + 0.05 * rng.normal(size=(3, 1)) * side[i]).astype(F))
    return soup.astype(F), wires, np.stack(blockers), centres, side


@functools.lru_cache(maxsize=None)
def scene_data(name, cos=0.0):
    if name.startswith("walls"):
        tris = _walls_triangles()
        cam = F([2.0, 1.5, 4.9])
        if name == "walls_far":
            shift = F([1000.0, -1000.0, 1000.0])
            tris, cam = (tris + shift).astype(F), (cam + shift).astype(F)
        if name == "walls_small":
            tris, cam = (tris * F(1e-3)).astype(F), (cam * F(1e-3)).astype(F)
        return _scene_of(tris, cam, (0.0, 0.0, -1.0), 8601)
    soup, wires, blockers, _, _ = _tripwired_parts(cos)
    return _scene_of(np.concatenate([soup, wires, blockers]), (0.0, 0.0, 6.0), (0.0, 0.0, -1.0), 8602)


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def _directions(rng, d, lo=0.1, hi=10.0):
    """Unit directions scaled to lengths log-uniform in [lo, hi] (the fast path takes 1/16 .. 16)."""
    return (ic.unit64(d) * ic.log_uniform(rng, lo, hi, (len(d), 1))).astype(F)


def _off_by_ulps(c, k):
    """The floats c moved by k units in the last place; a zero moves to the k-th denormal of either sign."""
    moved = (ic.bits(c).astype(np.int64) + np.where(c < 0, -k, k)).astype(np.uint32).view(F)
    return np.where(c == 0, (k * 1.4e-45).astype(F), moved)


def _camera_like(sd, seed):
    o, d = _camera_rays(sd, 256, 256, seed=seed)                          # 65,536 rays: a quarter of the set
    return o, d


def _walls_rays(name):
    sd = scene_data(name)
    tris = sd.positions.reshape(-1, 3, 3)
    rng = np.random.default_rng(8610)
    lo, hi = tris.reshape(-1, 3).min(axis=0).astype(np.float64), tris.reshape(-1, 3).max(axis=0).astype(np.float64)
    L = float((hi - lo).max()) / 5.2                                      # 1 for the room as built, 1e-3 for the small one
    centre = (lo + hi) / 2
    n = (N_RAYS - N_RAYS // 4) // 6
    flat = np.argmin(tris.max(axis=1) - tris.min(axis=1), axis=1)         # every triangle is flat on one axis
    assert ((tris.max(axis=1) - tris.min(axis=1)).min(axis=1) == 0).all()

    def surface(k):
        """k points on random triangles (exactly in their planes), each with the unit normal that points to the room's middle."""
        pick = rng.integers(0, len(tris), k)
        w = rng.dirichlet((1, 1, 1), k)
        P = (tris[pick].astype(np.float64) * w[:, :, None]).sum(axis=1).astype(F)
        ax = flat[pick]
        P[np.arange(k), ax] = tris[pick, 0, ax]
        nrm = np.zeros((k, 3))
        nrm[np.arange(k), ax] = np.where(centre[ax] >= P[np.arange(k), ax], 1.0, -1.0)
        return P, nrm, ax

    def tangent(nrm, k):
        t = rng.normal(size=(k, 3))
        t -= (t * nrm).sum(axis=1, keepdims=True) * nrm
        return ic.unit64(t)

    inside = lambda k: rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (k, 3)).astype(F)
    parts = []
    # 1 shared edges and vertices: a corner of a triangle, or a point of one of its edges, from anywhere in the room
    pick, corner = rng.integers(0, len(tris), n), rng.integers(0, 3, n)
    v0, v1 = tris[pick, corner].astype(np.float64), tris[pick, (corner + 1) % 3].astype(np.float64)
    s = np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0, 1, n))[:, None]
    target = (v0 + s * (v1 - v0)).astype(F)
    o = inside(n)
    parts.append((o, _directions(rng, target.astype(np.float64) - o)))
    # 2 grazing inside a wall's plane: the origin in the plane or up to 3 ulp off it, the direction in the plane exactly (a zero component:
    #   the exact walk takes those) or leaving it by a hair
    P, nrm, ax = surface(n)
    rows = np.arange(n)
    P[rows, ax] = _off_by_ulps(P[rows, ax], rng.integers(-3, 4, n))
    d = tangent(nrm, n) + nrm * (rng.choice([0.0, 1e-30, 1e-12, 1e-7, 1e-5, 1e-3], n) * rng.choice([-1.0, 1.0], n))[:, None]
    parts.append((P, _directions(rng, d, 0.5, 2.0)))
    # 3 starting on a surface, 1e-4 off it along the normal or not at all: into it, along it, and away from it
    P, nrm, ax = surface(n)
    o = (P + np.where(rng.random((n, 1)) < 0.5, 1e-4 * L, 0.0) * nrm).astype(F)
    lean = np.select([rng.random(n) < 0.4, rng.random(n) < 0.7], [-rng.uniform(0.01, 1.0, n), -rng.uniform(1e-4, 0.05, n)], rng.uniform(0.01, 1.0, n))
    parts.append((o, _directions(rng, tangent(nrm, n) + lean[:, None] * nrm)))
    # 4 short rays: t from 1e-5 to 1e-2 (in the room's unit) to a surface point, unit directions and others
    P, nrm, ax = surface(n)
    d = tangent(nrm, n) * rng.uniform(0, 1.5, (n, 1)) - nrm
    d = _directions(rng, d, 0.5, 2.0)
    t = ic.log_uniform(rng, 1e-5, 1e-2, (n, 1)) * L
    parts.append(((P - t * ic.unit64(d)).astype(F), d))
    # 5 across the room at random surface points, every length of direction (some outside the fast path's 1/16 .. 16)
    P, nrm, ax = surface(n)
    o = inside(n)
    parts.append((o, _directions(rng, P.astype(np.float64) - o, 0.05, 20.0)))
    # 6 from a surface point to a surface point: both ends in faces of flat boxes
    P, nrm, ax = surface(N_RAYS - N_RAYS // 4 - 5 * n)
    Q, _, _ = surface(len(P))
    parts.append((P, _directions(rng, Q.astype(np.float64) - P + 1e-9 * L)))
    parts.append(_camera_like(sd, 8611))
    return np.concatenate([p[0] for p in parts]).astype(F), np.concatenate([p[1] for p in parts]).astype(F)


def _tripwired_rays(cos):
    sd = scene_data("tripwired", cos)
    soup, wires, blockers, centres, side = _tripwired_parts(cos)
    rng = np.random.default_rng(8620)
    k = ic.kernel_direction()
    n_cam = N_RAYS // 4
    n = (N_RAYS - n_cam) // 4
    parts = []
    which = rng.integers(0, N_WIRES, n)
    start = lambda w, m: (centres[w] + side[w] * rng.uniform(1.6, 3.0, (m, 1)) + rng.normal(size=(m, 3)) * 0.5).astype(F)
    # 1 across a wire's leaf box from the blocker's side
    lo, hi = wires.min(axis=1).astype(np.float64), wires.max(axis=1).astype(np.float64)
    o = start(which, n)
    parts.append((o, _directions(rng, rng.uniform(lo[which], hi[which]) - o, 0.5, 2.0)))
    # 2 at the wire's plane far from the wire, along the direction its test is blind in
    o = start(which, n)
    far = centres[which] + k * rng.uniform(-3.0, 3.0, (n, 1)) + rng.normal(size=(n, 3)) * 0.05
    parts.append((o, _directions(rng, far - o, 0.5, 2.0)))
    # 3 from behind the wire (no blocker in the way), and from inside its box
    o = (centres[which] - side[which] * rng.uniform(0.0, 2.0, (n, 1)) + rng.normal(size=(n, 3)) * 0.3).astype(F)
    parts.append((o, _directions(rng, rng.uniform(lo[which], hi[which]) + k * rng.uniform(-1.0, 1.0, (n, 1)) - o, 0.5, 2.0)))
    # 4 the soup's own rays
    m = N_RAYS - n_cam - 3 * n
    o, d = pin_cases.rays_for(sd, m, 8621)
    parts.append((np.clip(o, -5.9, 5.9), d))
    parts.append(_camera_like(sd, 8622))
    return np.concatenate([p[0] for p in parts]).astype(F), np.concatenate([p[1] for p in parts]).astype(F)


@functools.lru_cache(maxsize=None)
def rays(name, cos=0.0):
    o, d = _tripwired_rays(cos) if name == "tripwired" else _walls_rays(name)
    assert o.shape == d.shape == (N_RAYS, 3) and np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(axis=1).all()
    o.setflags(write=False); d.setflags(write=False)
    return o, d


# ---- the GPU's answers, once per scene -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def answers(rt):
    made = {}

    def get(name):
        if name not in made:
            scene = rt.Scene(scene_data(name))
            o, d = rays(name)
            fast, st = scene.query_closest(o, d)
            made[name] = dict(scene=scene, fast=fast, st=st)
        return made[name]
    yield get
    for a in made.values():
        a["scene"].close()


def _digest(sd):
    """n_tripwire_groups and the number of member records of the scene's preparation (rtt_prepared_digest: `tripwires` holds 8 floats per
    group and 8 per member)."""
    rt = pin_cases.rt
    hooks = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    hooks.rtt_prepared_digest.argtypes = [C.POINTER(rt.rt_scene_desc), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(8192)
    n = hooks.rtt_prepared_digest(C.byref(sd.desc), rt.RT_INTEGRATOR_HW8, 0, buf, len(buf))
    assert 0 < n < len(buf), n
    lines = {l.split()[0]: l.split() for l in buf.value.decode().splitlines()}
    groups = int(lines["n_tripwire_groups"][2], 16)
    return groups, int(lines["tripwires"][1]) // 8 - groups


def _sample(name, fast, rt, also=()):
    """1,024 rays at random and up to 1,024 of those the fast call sent to the exact walk; and up to 256 of the rays `also`."""
    rng = np.random.default_rng(8630 + SCENE_NAMES.index(name))
    exact = np.flatnonzero(fast["flags"] & rt.RT_HIT_EXACT_WALK)
    also = np.asarray(also, np.int64)
    return np.concatenate([rng.choice(N_RAYS, N_ORACLE, replace=False), rng.choice(exact, min(N_ORACLE, exact.size), replace=False),
                           rng.choice(also, min(256, also.size), replace=False)])


def _nan_records(hits):
    """Rays whose hit record holds a NaN: a hit with NaN barycentrics (den == 0: every comparison of the test is false, so it is a hit)."""
    return np.flatnonzero(np.isnan(hits["ns"]).any(axis=1) | np.isnan(hits["texcoord"]).any(axis=1) | np.isnan(hits["tangent"]).any(axis=1))


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_closest_hits_equal_the_forced_reference_walk_and_the_oracle(rt, answers, name):
    a = answers(name)
    o, d = rays(name)
    fast, st = a["fast"], a["st"]
    slow, st_ref = a["scene"].query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    n_exact = int(((fast["flags"] & rt.RT_HIT_EXACT_WALK) != 0).sum())
    differ = int(np.any(_words(rt, fast) != _words(rt, slow), axis=1).sum())
    print(f"{name}: {st.rays} rays, {N_RAYS - n_exact - int(st.invalid_rays)} decided on the fast path, {n_exact} sent to the exact walk, hits {int((fast['triangle'] != MISS).sum())}, "
          f"{differ} differ from the forced reference walk; {st.kernel_ms:.2f} ms, forced {st_ref.kernel_ms:.2f} ms")
    assert st.reference_exact == 1 and st.rays == N_RAYS and st.invalid_rays == 0 and st.exact_walks == n_exact
    assert st_ref.exact_walks == N_RAYS
    assert N_RAYS - n_exact >= 200 and n_exact >= 200                     # both sides of the gate are at work
    assert differ == 0, _first_difference(_words(rt, fast), _words(rt, slow))
    # Two of the tripwired scene's 12 triangles have den == 0 exactly: their hits carry NaN barycentrics, and the record's NaNs must have
    # the reference's signs (x86 signs a NaN it generates; `-1. * shadingNorma` for an inside hit flips that sign like any other).
    nan_hits = _nan_records(fast)
    print(f"{name}: {nan_hits.size} hit records hold a NaN, {int(((fast['flags'][nan_hits] & rt.RT_HIT_INSIDE) != 0).sum())} of them inside hits")
    if name == "tripwired":
        assert nan_hits.size >= 100 and ((fast["flags"][nan_hits] & rt.RT_HIT_INSIDE) != 0).sum() >= 20 and ((fast["flags"][nan_hits] & rt.RT_HIT_INSIDE) == 0).sum() >= 20
    pick = _sample(name, fast, rt, nan_hits)
    sd = scene_data(name)
    want = _words(rt, _expected_hits(oracle_lib.Hw8Oracle(sd), sd, o[pick], d[pick]))
    assert np.array_equal(_words(rt, fast[pick]), want), _first_difference(_words(rt, fast[pick]), want)
    if oracle_lib.ref_path("libref_hw8.so"):
        live = _words(rt, _expected_hits(oracle_lib.Ref8(sd), sd, o[pick], d[pick]))
        assert np.array_equal(_words(rt, fast[pick]), live), _first_difference(_words(rt, fast[pick]), live)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_occlusion_is_what_the_closest_hits_say(rt, answers, name):
    """tmax of +inf, t, t +- 1 ulp and 0.5 t (T = the closest hit's t; a fixed bound for a ray that misses): occluded == hit and t < tmax."""
    a = answers(name)
    o, d = rays(name)
    hit, t = a["fast"]["triangle"] != MISS, a["fast"]["t"]
    T = np.where(hit, t, F(1.0)).astype(F)
    bounds = {"inf": np.full(N_RAYS, np.inf, F), "t": T, "t + 1 ulp": ic.ulp_step(T, 1), "t - 1 ulp": ic.ulp_step(T, -1), "t / 2": (F(0.5) * T).astype(F)}
    for kind, tmax in bounds.items():
        occ, st = a["scene"].query_occluded(o, d, tmax)
        want = (hit & (t < tmax)).astype(np.uint8)
        bad = np.flatnonzero((occ & rt.RT_OCCLUSION_OCCLUDED) != want)
        print(f"{name}, tmax = {kind}: {int(want.sum())} occluded, {st.exact_walks} exact walks, {bad.size} differ from the closest hits")
        assert st.reference_exact == 1 and st.invalid_rays == 0
        assert bad.size == 0, (kind, bad[:5].tolist(), o[bad[:5]].tolist(), d[bad[:5]].tolist(), tmax[bad[:5]].tolist(), t[bad[:5]].tolist())


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_light_pdfs_equal_the_forced_reference_walk_and_the_oracle(rt, answers, name):
    a = answers(name)
    o, d = rays(name)
    fast, st = a["scene"].query_light_pdf(o, d)
    slow, st_ref = a["scene"].query_light_pdf(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    differ = np.flatnonzero(fast.view(np.uint32) != slow.view(np.uint32))
    print(f"{name}: light pdf of {st.rays} rays, {st.exact_walks} sent to the exact walk, nonzero {int((fast != 0).sum())}, {differ.size} differ from the forced reference walk")
    assert st.reference_exact == 1 and st.invalid_rays == 0 and st_ref.exact_walks == N_RAYS
    assert N_RAYS - st.exact_walks >= 200 and (fast != 0).sum() >= 200
    assert differ.size == 0, (differ[:5].tolist(), fast[differ[:5]].tolist(), slow[differ[:5]].tolist())
    nan_pdf = np.flatnonzero(np.isnan(fast))                             # a light hit with NaN barycentrics: fabs(d . NaN) makes the term a NaN without a sign
    print(f"{name}: {nan_pdf.size} light pdfs are NaN")
    if name == "tripwired":
        assert nan_pdf.size >= 100
    pick = _sample(name, a["fast"], rt, nan_pdf)
    sd = scene_data(name)
    orc = oracle_lib.Hw8Oracle(sd)
    want = np.array([orc.light_pdf(o[i], d[i]) for i in pick], F)
    assert np.array_equal(fast[pick].view(np.uint32), want.view(np.uint32)), np.flatnonzero(fast[pick].view(np.uint32) != want.view(np.uint32))[:8]
    if oracle_lib.ref_path("libref_hw8.so"):
        ref = oracle_lib.Ref8(sd)
        live = np.array([ref.light_pdf(o[i], d[i]) for i in pick], F)
        assert np.array_equal(fast[pick].view(np.uint32), live.view(np.uint32))


@pytest.mark.parametrize("pipeline", ["default", "rounds_exact"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_renders_equal_the_oracle(rt, monkeypatch, name, pipeline):
    """64 x 48 x 4 spp on the default pipeline (the persistent walkers and their 16-bit boxes, which the queries do not run) and on the
    round pipeline with exact re-walks."""
    sd = scene_data(name)
    if pipeline == "rounds_exact":
        monkeypatch.setenv("RTAMD_KERNEL", "wavefront")
        monkeypatch.setenv("RTAMD_ROUNDS_EXACT", "1")
    scene = rt.Scene(sd)
    try:
        rgb, rgb8, st = scene.render(64, 48, 4, counters=True)
    finally:
        scene.close()
    ref, ref8, _ = oracle_lib.Hw8Oracle(sd).render(64, 48, 4)
    bad = int((rgb.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    print(f"{name}, {pipeline}: pipeline {st.pipeline}, exact closest hits {st.exact_closest_hits} of {st.closest_hit_queries}, exact light sums {st.exact_light_sums} of "
          f"{st.light_pdf_queries}; {bad} of {64 * 48} pixels differ from the oracle")
    assert st.pipeline == (rt.RT_PIPELINE_ROUNDS if pipeline == "rounds_exact" else rt.RT_PIPELINE_PERSISTENT)
    assert st.reference_exact == 1
    assert np.array_equal(rgb, ref, equal_nan=True) and np.array_equal(rgb8, ref8)


def test_tripwired_scene_has_its_tripwires():
    """The 12 constructed triangles, and whatever else of the scene lies below the threshold, are the preparation's tripwire members."""
    sd = scene_data("tripwired")
    cos = float_cos(sd.positions.reshape(-1, 3, 3))
    groups, members = _digest(sd)
    print(f"tripwired: {groups} tripwire groups, {members} members; |cos| of the constructed ones {np.sort(cos[300:300 + N_WIRES]).tolist()}")
    assert (cos[300:300 + N_WIRES] < 2.0 ** -16).all()
    assert groups > 0 and members == int((cos < TRIPWIRE_COS).sum()) and members >= N_WIRES


@pytest.mark.parametrize("log2_cos", [-13, -12, -10, -8])
def test_census_of_the_band_above_the_tripwire_threshold(rt, log2_cos):
    """Recorded, not asserted: the tripwired scene with its 12 triangles at |cos| above RTAMD_TRIPWIRE_COS, where no tripwire guards them
    and the gate's window has to.  The number of rays whose fast answer differs from the forced reference walk is printed (profiles/
    r26_intersection_edges.txt holds the run's figures); replacing the threshold by a bound is a design change of its own."""
    cos = 2.0 ** log2_cos
    sd = scene_data("tripwired", cos)
    fc = float_cos(sd.positions.reshape(-1, 3, 3))[300:300 + N_WIRES]
    groups, members = _digest(sd)
    o, d = rays("tripwired", cos)
    scene = rt.Scene(sd)
    try:
        fast, st = scene.query_closest(o, d)
        slow, _ = scene.query_closest(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    finally:
        scene.close()
    differ = int(np.any(_words(rt, fast) != _words(rt, slow), axis=1).sum())
    print(f"census |cos| = 2^{log2_cos}: constructed triangles at {fc.min():.3e} .. {fc.max():.3e}, {members} tripwire members, {st.exact_walks} of {st.rays} rays "
          f"sent to the exact walk, {differ} fast answers differ from the forced reference walk")
    assert st.rays == N_RAYS and (fc >= TRIPWIRE_COS).all()

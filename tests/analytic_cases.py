"""The inputs on which the analytic figures, the light pdf and the samplers of the .txt snapshots (hw1 .. hw5: rt_kernels_txt.h,
rt_kernels_hw4.h, rt_kernels_hw5.h) are pinned at their branch points: one table for the golden generator (golden/make_goldens.py ->
pins_analytic_edges.npz), the host pin (test_analytic_pins.py) and the GPU test (test_gpu_analytic.py).  Everything is deterministic:
fixed seeds, float32 arrays, boundary inputs placed by bit arithmetic or through the oracle; numpy supplies no transcendental function.

A figure row is 24 floats: type, data 3, data2 3, data3 3, position 3, rotation 4 (x y z w, exactly as parsed), o 3, d 3, one unused.
An answer is a row of 32-bit words: flags (1 hit | 2 inside) and float bits, all 0 for a miss.

families()   quad      a, b, c                      hw2's float roots | hw3's double-then-narrow roots: 2 x (flags, t)
             slabs     s, o, d                      the slab test alone (hw5's intersectBoxAndRay without the normal): flags, t
             fig       an ELLIPSOID / PLANE / BOX figure row       Figure::intersect of hw1 | hw2 | hw3 | hw4 | hw5: 5 x (flags, t, normal)
             tri5      a TRIANGLE figure row        hw5's Figure::intersect: flags, t, normal
             lpdf      a light's figure row, x = o  hw4's FigureLight::pdf (0 for a triangle) | hw5's pdfOneFigureLight
             pone      a light's figure row, x = o, then y 3 and yn 3 of the row's own (30 floats)     pdfOne(x, d, y, yn) of hw4's BoxLight /
                       EllipsoidLight (0 for a triangle) | hw5's BoxLight / EllipsoidLight / TriangleLight
             lsample   a light's figure row, x = o, and aux = (seed, prime)     hw4's | hw5's sample(x): 2 x (direction 3, engine state,
                       the normal cache after 2, the normal cache before 2).  prime != 0: the normal_distribution the light draws from
                       (hw4: the EllipsoidLight's own, hw5: the pixel's) holds the second value of one polar round of engine(prime).
             cosine    a normal and aux             Cosine::sample of hw4 | hw5, the same 2 x 8 words

lsample: every row's rejection loop ends; the draws of a row are counted by stepping a minstd_rand from the seed to the returned state
(draws()).  Largest count over the table: 86 engine steps, 22 attempts (hw4 and hw5 alike); generation fails above 4,096.
cosine: the fallback `return n` is reached: for a seed the drawn unit vector v comes from the oracle's own normal draws, and n = -v and the
floats beside it make |v + n| <= 1e-9 or (v + n) . n <= 1e-9.
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib

F = np.float32
U = np.uint32
M31 = 2147483647
A = 48271
A_INV = 1899818559                                   # 48271^-1 mod 2^31 - 1
ELLIPSOID, PLANE, BOX, TRIANGLE = 0, 1, 2, 3
T_MAX_BITS = 0x461C4000                              # the float 1e4
FAMILIES = ("quad", "slabs", "fig", "tri5", "lpdf", "pone", "lsample", "cosine")
WIDTH = {"quad": 4, "slabs": 2, "fig": 25, "tri5": 5, "lpdf": 2, "pone": 2, "lsample": 16, "cosine": 16}
MAX_DRAWS = 4096
IDENTITY = (0.0, 0.0, 0.0, 1.0)
# the rotation exactly as parsed: identity, non-unit, zero, 180-degree turns, a third of a turn, and two of no special kind
QUATS = (IDENTITY, (0.0, 0.0, 0.0, 2.0), (0.2, 0.4, -0.6, 1.5), (0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0),
         (0.0, 0.0, 1.0, 0.0), (0.5, 0.5, 0.5, 0.5), (0.18257419, 0.36514837, 0.5477226, 0.73029674), (-0.6, 0.0, 0.8, 0.0))
UNIT_QUATS = (IDENTITY, (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5), (0.18257419, 0.36514837, 0.5477226, 0.73029674), (-0.6, 0.0, 0.8, 0.0))
# seeds whose first two uniforms u, v have float(u + v) == 1 with the exact sum above 1 (the fold `u + v > 1.` is taken on the float sum:
# no fold), the same with the exact sum at most 1, and float(u + v) within 2^-22 above 1 (fold).  They came from a scan of engine states
# that is not kept here; what stands for them is test_boundary_seeds_draw_what_they_claim, which draws u and v for every one of them.
FOLD_SEEDS = {"sum_one_exact_above": (1155666760, 163849873, 374234534, 1529901294, 538084407, 748469068, 1904135828, 2114520489),
              "sum_one_exact_below": (1366051421, 584619195, 1740285955, 958853729, 177421503, 1333088263, 551656037, 1917707458),
              "just_above": (117315085, 234630170, 1272981845, 281164958, 1319516633, 1436831718, 327699746, 445014831)}


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def from_bits(b):
    return np.ascontiguousarray(b, U).view(F)


def ulp_step(x, k):
    """The float k steps from x (x finite and positive)."""
    out = from_bits((bits(x).astype(np.int64) + k).astype(U))
    return out[0] if np.ndim(x) == 0 else out


def figrow(ftype, data, o, d, position=(0, 0, 0), rotation=IDENTITY, data2=(0, 0, 0), data3=(0, 0, 0)):
    r = np.zeros(24, F)
    r[0] = ftype
    r[1:4], r[4:7], r[7:10], r[10:13], r[13:17], r[17:20], r[20:23] = data, data2, data3, position, rotation, o, d
    return r


class Table:
    def __init__(self):
        self.rows, self.kind, self.names = [], [], {}

    def add(self, name, rows):
        rows = np.atleast_2d(np.asarray(rows, F))
        k = self.names.setdefault(name, len(self.names))
        self.rows.append(rows)
        self.kind.append(np.full(len(rows), k, np.int32))

    def done(self, **extra):
        out = {"rows": np.ascontiguousarray(np.concatenate(self.rows), F), "kind": np.concatenate(self.kind), "K": dict(self.names)}
        out.update(extra)
        out["rows"].setflags(write=False)
        return out


def seed_for_first(x1):
    """The seed whose engine's first output is x1."""
    return int(x1) * A_INV % M31


def first_outputs_for_u01(value):
    """Engine outputs x with float(x - 1) * 2^-31 == value (a float32 in (0, 1))."""
    centre = int(np.float64(value) * 2.0 ** 31)
    xs = np.arange(centre - 256, centre + 257, dtype=np.int64)
    xs = xs[(xs >= 1) & (xs < M31 - 1)]
    return (xs[(xs.astype(F) * F(2.0 ** -31)) == F(value)] + 1).tolist()


# ---- quad ----------------------------------------------------------------------------------------------------------------------------
def _quad():
    T = Table()
    rng = np.random.default_rng(2701)
    T.add("random", (rng.normal(size=(2000, 3)) * np.exp2(rng.integers(-3, 4, size=(2000, 3)))).astype(F))
    T.add("random_a_negative", np.abs(rng.normal(size=(500, 3))).astype(F) * F([-1, 1, 1]) * rng.choice(F([-1, 1]), size=(500, 3)))
    m, n = np.meshgrid(np.arange(1, 9), np.arange(1, 9))
    m, n = m.reshape(-1).astype(F), n.reshape(-1).astype(F)
    for sb in (-1, 1):
        for sa in (-1, 1):
            T.add("discriminant_zero", np.stack([sa * m * m, sb * 2 * m * n, sa * n * n], axis=1))                          # b^2 == 4ac exactly
    tiny = (rng.normal(size=(300, 3)) * np.exp2(-70.0)).astype(F)
    T.add("discriminant_denormal", tiny)
    T.add("discriminant_denormal", [[0.0, 2.0 ** -70, 1.0], [2.0 ** -149, 2.0 ** -74, -1.0], [1.0, 2.0 ** -74, 0.0], [1.0, 2.0 ** -74, -0.0]])
    nan, inf = np.nan, np.inf
    T.add("discriminant_nan", [[nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, inf, 1], [inf, 1, 0], [1, inf, inf], [-1, inf, -inf], [0, inf, 1], [1, -inf, 1], [inf, 1, -1], [-inf, 1, 1]])
    a0 = [[z, b, c] for z in (0.0, -0.0) for b in (-3.0, -1.0, 1.0, 2.5, 2.0 ** -60) for c in (-2.0, -0.0, 0.0, 1.0, 7.0)]
    T.add("a_zero", a0)
    zero_root = [[a, b, c] for a in (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0) for b in (-3.0, -1.0, 1.0, 3.0) for c in (-0.0, 0.0)]
    T.add("zero_root", zero_root)                                                                                                   # c == +-0: one root is a zero of either sign
    # x1 underflows to -0 with x2 >= 0: d = b^2 rounds up to 2^-149, sqrt(d) > |b|, (-b - sqrt(d)) / 2a below the denormals
    under = [[2.0 ** e, -1.2 * 2.0 ** -75, c] for e in (74, 75, 76, 80, 90) for c in (0.0, -0.0)]
    T.add("minus_zero_outside", under)
    return T.done()


# ---- slabs ---------------------------------------------------------------------------------------------------------------------------
def _slabs():
    T = Table()
    rng = np.random.default_rng(2702)
    n = 1500
    s = rng.uniform(0.1, 3.0, size=(n, 3))
    o = rng.uniform(-4, 4, size=(n, 3))
    target = rng.uniform(-1, 1, size=(n, 3)) * s * np.where(rng.random((n, 1)) < 0.7, 1.0, 2.5)
    T.add("random", np.concatenate([s, o, target - o], axis=1).astype(F))
    o_in = rng.uniform(-1, 1, size=(400, 3)) * s[:400]
    T.add("random_inside", np.concatenate([s[:400], o_in, rng.normal(size=(400, 3))], axis=1).astype(F))
    axis_rows = {"zero_on_low_face": [], "zero_on_high_face": [], "zero_off_face": []}
    for k in range(3):
        for z in (0.0, -0.0):
            for j in range(40):
                sj = rng.uniform(0.5, 2.0, size=3).astype(F)
                oj = (rng.uniform(-3, 3, size=3)).astype(F)
                tj = (rng.uniform(-1, 1, size=3) * sj * (1.0 if j % 2 else 2.0)).astype(F)
                dj = (tj - oj).astype(F)
                dj[k] = z
                for name, ok in (("zero_on_low_face", -sj[k]), ("zero_on_high_face", sj[k]), ("zero_off_face", F(0.25) * sj[k])):
                    oo = oj.copy()
                    oo[k] = ok
                    axis_rows[name].append(np.concatenate([sj, oo, dj]))
    for name, rows in axis_rows.items():
        T.add(name, rows)
    axis = np.repeat(np.arange(3), 80)
    # t1 == t2 (through an edge), t1 == +-0 and t2 == +-0 (the origin on a face, leaving or entering), all in exact binary values
    graze = []
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        graze.append([1, 1, 1, -2 * sx, 0, 0.25, sx, sy, 0])
        graze.append([1, 2, 4, -2 * sx, 0, 0.5, sx, 2 * sy, 0])
        graze.append([1, 1, 1, 0.25, -2 * sx, 0, 0, sx, sy])
    T.add("graze_edge", graze)
    zero_t = []
    for face in (-1.0, 1.0):
        for dx in (-1.0, 1.0, -0.5, 2.0):
            for dy in (0.0, -0.0, 0.125, -0.125):
                zero_t.append([1, 1, 1, face, 0.25, -0.5, dx, dy, 0.0625])
                zero_t.append([2, 1, 0.5, 0.25, face, 0.125, dy, dx, -0.03125])
                zero_t.append([2, 1, 0.5, 0.25, 0.5, face * 0.5, dy, 0.03125, dx])
    T.add("zero_t", zero_t)
    T.add("flat_and_extreme", [[0, 1, 1, -2, 0.3, 0.2, 1, 0, 0], [0, 1, 1, -2, 0.3, 0.2, 1, 0.01, 0], [1, 0, 1, 0.3, -2, 0.2, 0, 1, 0], [1, 1, 0, 0.3, 0.2, 3, 0, 0, -1],
                               [0, 0, 0, 0, 0, 0, 1, 1, 1], [1e-40, 1e-40, 1e-40, -1e-39, 0, 0, 1, 0, 0], [1e30, 1e30, 1e30, -3e30, 1e29, 0, 1, 0, 0],
                               [1, 1, 1, -2, 0, 0, 1e-42, 0, 0], [1, 1, 1, np.nan, 0, 0, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, -2, 0, 0, np.inf, 0, 0]])
    out = T.done()
    out["axis"] = np.full(len(out["rows"]), -1)
    for name in axis_rows:
        out["axis"][out["kind"] == out["K"][name]] = axis
    return out


# ---- fig -----------------------------------------------------------------------------------------------------------------------------
def _random_figure_rows(rng, ftype, n, quats):
    rows = []
    for i in range(n):
        data = rng.uniform(0.3, 2.0, size=3) if ftype != PLANE else rng.normal(size=3) * rng.choice([0.5, 1.0, 3.0])
        pos = rng.uniform(-2, 2, size=3) * (i % 3 != 0)
        q = quats[i % len(quats)]
        o = pos + rng.uniform(-4, 4, size=3)
        if i % 5 == 4:                                                    # from inside the figure's neighbourhood
            o = pos + rng.uniform(-0.2, 0.2, size=3)
        aim = pos + rng.uniform(-1, 1, size=3) * (0.7 if i % 2 else 2.0)
        d = (aim - o) * rng.choice([0.25, 1.0, 1.0, 7.0])
        rows.append(figrow(ftype, data, o, d, pos, q))
    return np.stack(rows)


def _fig():
    T = Table()
    rng = np.random.default_rng(2703)
    for ftype, name in ((ELLIPSOID, "ellipsoid"), (PLANE, "plane"), (BOX, "box")):
        T.add("random_" + name, _random_figure_rows(rng, ftype, 640, QUATS))
    # ellipsoid: the discriminant at 0 (tangent rays in exact binary values), NaN (a zero radius under a zero coordinate, NaN inputs) and a == 0
    e = []
    for r in ((1, 1, 1), (2, 1, 0.5), (0.5, 4, 2)):
        for sgn in (-1, 1):
            e.append(figrow(ELLIPSOID, r, (-3 * r[0], sgn * r[1], 0), (r[0], 0, 0)))
            e.append(figrow(ELLIPSOID, r, (0, -3 * r[1], sgn * r[2]), (0, 2 * r[1], 0)))
            e.append(figrow(ELLIPSOID, r, (sgn * r[0], 0, 5 * r[2]), (0, 0, -r[2])))
    T.add("ellipsoid_tangent", e)
    e = [figrow(ELLIPSOID, (0, 1, 1), (0, 0.2, -3), (0, 0, 1)), figrow(ELLIPSOID, (1, 0, 1), (0.2, 0, -3), (0, 0, 1)), figrow(ELLIPSOID, (1, 1, 0), (-3, 0.2, 0), (1, 0, 0)),
         figrow(ELLIPSOID, (1, 1, 1), (np.nan, 0, -3), (0, 0, 1)), figrow(ELLIPSOID, (1, 1, 1), (0, 0, -3), (0, np.nan, 1)), figrow(ELLIPSOID, (np.inf, 1, 1), (0, 0, -3), (0, 0, 1)),
         figrow(ELLIPSOID, (1, 1, 1), (0, 0, -3), (0, 0, 1), rotation=(np.nan, 0, 0, 1)), figrow(ELLIPSOID, (1, 1, 1), (0, 0, -3), (0, 0, 1), position=(np.inf, 0, 0)),
         figrow(ELLIPSOID, (0, 1, 1), (0, 0.2, -3), (0, 0, 1), rotation=(0, 0, 0, 2)), figrow(ELLIPSOID, (0, 0, 0), (0, 0, 0), (0, 0, 1))]
    T.add("ellipsoid_nan", e)
    e = [figrow(ELLIPSOID, (1, 1, 1), (-1024, 0, 0), (s * 2.0 ** -76, 0, 0)) for s in (-1, 1)] + \
        [figrow(ELLIPSOID, (1, 1, 1), (0, 0, -3), (0, 0, 0)), figrow(ELLIPSOID, (1, 1, 1), (0, 0, 0.5), (0, -0.0, 0)), figrow(ELLIPSOID, (1, 2, 1), (0, 1024, 0.5), (0, -2.0 ** -76, 2.0 ** -80))]
    T.add("ellipsoid_a_zero", e)
    # plane: dn == +-0 (t is +-inf or NaN), t on the float 1e4 and its neighbours, t == +0, a normal that is not unit
    p = []
    for n in ((0, 1, 0), (0, 3, 0), (0, 0.25, 0)):
        for dd in ((1, 0, 0), (-1, -0.0, -1), (0, 0, 0.5), (-0.0, -0.0, -0.0), (0, 0, 0)):
            for h in (2.0, -2.0, 0.0, -0.0):
                p.append(figrow(PLANE, n, (0.5, h, -0.25), dd))
    T.add("plane_dn_zero", p)
    tmax = from_bits(U(T_MAX_BITS))[0]
    p = []
    for k in (-2, -1, 0, 1, 2):
        h = ulp_step(tmax, k)
        p.append(figrow(PLANE, (0, 1, 0), (0.5, h, 0.25), (0, -1, 0)))
        p.append(figrow(PLANE, (0, -2, 0), (0.5, h, 0.25), (0, -1, 0)))
        p.append(figrow(PLANE, (0, 0, 4), (3, 1, -2 * h), (0.5, 0, 2)))
        p.append(figrow(PLANE, (1, 0, 0), (h + 1, 0, 0), (-1, 0, 0), position=(1, 0, 0), rotation=(0, 0, 0, 1)))
    T.add("plane_t_max", p)
    p = [figrow(PLANE, (0, 1, 0), (0.5, z, 0.25), (0, s, 0)) for z in (0.0, -0.0, 2.0 ** -149, -2.0 ** -149) for s in (-1, 1)]
    T.add("plane_t_zero", p)
    # box: edges and corners (two and three components of the normal survive), a zero half-size, 0/0 on each axis
    b = []
    for s in ((1, 1, 1), (1, 2, 4), (0.5, 0.25, 2)):
        s = np.asarray(s, np.float64)
        for sx in (-1, 1):
            for sy in (-1, 1):
                b.append(figrow(BOX, s, (-2 * sx * s[0], -2 * sy * s[1], 0.25 * s[2]), (sx * s[0], sy * s[1], 0)))
                b.append(figrow(BOX, s, (0.25 * s[0], -2 * sx * s[1], -2 * sy * s[2]), (0, sx * s[1], sy * s[2])))
                b.append(figrow(BOX, s, (-2 * sx * s[0], 0.5 * s[1], -2 * sy * s[2]), (sx * s[0], 0, sy * s[2])))
                b.append(figrow(BOX, s, (0.5 * sx * s[0], 0.5 * sy * s[1], 0), (sx * s[0], sy * s[1], 0)))                       # from inside to an edge
    T.add("box_edge", b)
    b = []
    for s in ((1, 1, 1), (1, 2, 4), (0.5, 0.25, 2)):
        s = np.asarray(s, np.float64)
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    sg = np.array([sx, sy, sz])
                    b.append(figrow(BOX, s, -2 * sg * s, sg * s))
                    b.append(figrow(BOX, s, 0.5 * sg * s, sg * s))                                                               # from inside to a corner
                    b.append(figrow(BOX, s, -2 * sg * s, sg * s, position=(0, 0, 0), rotation=(0, 0, 0, 2)))
    T.add("box_corner", b)
    b = [figrow(BOX, (0, 1, 1), (-2, 0.3, 0.2), (1, 0, 0)), figrow(BOX, (1, 0, 1), (0.3, -2, 0.2), (0, 1, 0)), figrow(BOX, (1, 1, 0), (0.3, 0.2, 3), (0, 0, -1)),
         figrow(BOX, (0, 1, 1), (-2, 0.3, 0.2), (1, 0.01, 0)), figrow(BOX, (0, 0, 1), (0, 0, 3), (0, 0, -1)), figrow(BOX, (0, 0, 0), (0, 0, 0), (1, 1, 1))]
    T.add("box_zero_size", b)
    sl = _slabs()
    zero = np.isin(sl["kind"], [sl["K"]["zero_on_low_face"], sl["K"]["zero_on_high_face"], sl["K"]["zero_t"], sl["K"]["graze_edge"]])
    zr = sl["rows"][zero]
    T.add("box_slab_edges", np.stack([figrow(BOX, r[0:3], r[3:6], r[6:9]) for r in zr]))
    T.add("box_slab_edges_moved", np.stack([figrow(BOX, r[0:3], r[3:6] + F([1, -2, 0.5]), r[6:9], position=(1, -2, 0.5)) for r in zr[::3]]))
    return T.done()


# ---- tri5 ----------------------------------------------------------------------------------------------------------------------------
def trirow(data, data2, a, o, d, position=(0, 0, 0), rotation=IDENTITY):
    return figrow(TRIANGLE, data, o, d, position, rotation, data2=data2, data3=a)


def _tri5():
    T = Table()
    rng = np.random.default_rng(2705)
    rows = []
    for i in range(2000):
        a, p1, p2 = rng.uniform(-2, 2, size=(3, 3))
        pos = rng.uniform(-2, 2, size=3) * (i % 3 != 0)
        q = QUATS[i % len(QUATS)]
        w = rng.dirichlet((1, 1, 1)) if i % 4 else rng.uniform(-0.5, 1.5, size=3)
        aim = w[0] * a + w[1] * p1 + w[2] * p2 + pos
        o = aim + rng.normal(size=3) * 3
        rows.append(trirow(p1, p2, a, o, (aim - o) * rng.choice([0.5, 1.0, 4.0]), pos, q))
    T.add("random", np.stack(rows))
    # p exactly on each edge, and a step beside it: the unit right triangle in z = 0, rays along z, everything exact
    grid = [-2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 2.0 ** -24, 0.25, 0.5, 0.75, float(ulp_step(F(1), -1)), 1.0, float(ulp_step(F(1), 1))]
    edge = []
    for px in grid:
        for py in grid:
            for dz in (-1.0, 1.0):
                edge.append(trirow((1, 0, 0), (0, 1, 0), (0, 0, 0), (px, py, -dz), (0, 0, dz)))
                edge.append(trirow((0, 1, 0), (1, 0, 0), (0, 0, 0), (px, py, -dz), (0, 0, dz)))                                 # the other winding: n negated
    T.add("edge_grid", edge)
    moved = [trirow((3, 1, 0.5), (2, 2, 0.5), (2, 1, 0.5), (px + 2, py + 1, 0.5 - dz), (0, 0, dz)) for px in grid[4:] for py in grid[4:] for dz in (-1.0, 1.0)]
    T.add("edge_grid_moved", moved)
    T.add("degenerate", [trirow((1, 0, 0), (1, 0, 0), (0, 0, 0), (0.2, 0.2, 1), (0, 0, -1)), trirow((1, 1, 1), (2, 2, 2), (0, 0, 0), (0.2, 0.2, 1), (0, 0, -1)),
                         trirow((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 1), (0, 0, -1)), trirow((1, 0, 0), (0, 1, 0), (0, 0, 0), (0.2, 0.2, 1), (1, 0, 0)),
                         trirow((1, 0, 0), (0, 1, 0), (0, 0, 0), (0.2, 0.2, 0), (1, 0, 0)), trirow((1, 0, 0), (0, 1, 0), (0, 0, 0), (0.2, 0.2, 0.0), (0, 0, -1)),
                         trirow((1, 0, 0), (0, 1, 0), (0, 0, 0), (0.2, 0.2, -0.0), (0, 0, 1)), trirow((np.nan, 0, 0), (0, 1, 0), (0, 0, 0), (0.2, 0.2, 1), (0, 0, -1))])
    tmax = from_bits(U(T_MAX_BITS))[0]
    far = []
    big = 32768.0                                                       # n = (0, 0, +-2^30): t = h exactly
    for k in (-2, -1, 0, 1, 2):
        h = float(ulp_step(tmax, k))
        for dz in (-1.0, 1.0):
            far.append(trirow((big - 100, -100, 0), (-100, big - 100, 0), (-100, -100, 0), (0.25, 0.5, -dz * h), (0, 0, dz)))
            far.append(trirow((-100, big - 100, 0), (big - 100, -100, 0), (-100, -100, 0), (0.25, 0.5, -dz * h), (0, 0, dz)))
    T.add("t_max", far)
    return T.done()


# ---- lpdf ----------------------------------------------------------------------------------------------------------------------------
def _light_figure(rng, ftype, i, quats):
    pos = rng.uniform(-2, 2, size=3) * (i % 3 != 0)
    q = quats[i % len(quats)]
    if ftype == TRIANGLE:
        a, p1, p2 = rng.uniform(-1.5, 1.5, size=(3, 3))
        return dict(data=p1, data2=p2, data3=a, position=pos, rotation=q), a, p1, p2
    return dict(data=rng.uniform(0.3, 1.5, size=3), position=pos, rotation=q), None, None, None


def _lpdf():
    T = Table()
    rng = np.random.default_rng(2706)
    for ftype, name in ((BOX, "box"), (ELLIPSOID, "ellipsoid"), (TRIANGLE, "triangle")):
        rows, inside = [], []
        for i in range(1300 if ftype != TRIANGLE else 700):
            fig, a, p1, p2 = _light_figure(rng, ftype, i, QUATS)
            pos = fig["position"]
            if ftype == TRIANGLE:
                w = rng.dirichlet((1, 1, 1)) if i % 4 else rng.uniform(-0.5, 1.5, size=3)
                aim = w[0] * a + w[1] * p1 + w[2] * p2 + pos
            else:
                aim = pos + rng.uniform(-1, 1, size=3) * fig["data"] * (0.6 if i % 4 else 1.6)
            x = aim + rng.normal(size=3) * 3
            d = aim - x
            d = d / np.sqrt((d * d).sum()) if i % 2 else d * rng.choice([0.5, 3.0])
            rows.append(figrow(ftype, o=x, d=d, **fig))
            if ftype != TRIANGLE and i % 4 == 0 and fig["rotation"] in UNIT_QUATS:
                inside.append(figrow(ftype, o=pos + rng.uniform(-0.1, 0.1, size=3), d=rng.normal(size=3), **fig))
        T.add("random_" + name, np.stack(rows))
        if inside:
            T.add("inside_" + name, np.stack(inside))
    # a first hit at a t far below eps: the second ray starts at float(t + eps), where eps is 1e-4 in double (hw4), in 80 bits (hw5), and
    # where the float 1e-4 in its place would round differently on every third row
    near = []
    for k in range(1, 41):
        step = k * 2.0 ** -34 * (1 + (k % 7))
        near.append(figrow(BOX, (2.0 ** -10, 0.5, 0.5), (-2.0 ** -10 - step, 0.1, 0.05), (1, 0.01, 0.02)))
        near.append(figrow(ELLIPSOID, (2.0 ** -10, 0.5, 0.25), (-2.0 ** -10 - step, 0, 0), (1, 2.0 ** -12, 0)))
        near.append(figrow(BOX, (0.25, 2.0 ** -10, 0.5), (0.1, 2.0 ** -10 - step, 0.05), (0.01, -1, 0.02)))                    # from just inside: the exit first
    T.add("tiny_first_t", near)
    # the same on a figure of the size of eps itself, where one step of float(t + eps) moves the second origin and with it t2 and y2
    small = []
    for k in range(1, 101):
        step = k * 2.0 ** -40 * (1 + (k % 5))
        small.append(figrow(BOX, (2.0 ** -14, 2.0 ** -14, 2.0 ** -14), (-2.0 ** -14 - step, 2.0 ** -16, 2.0 ** -17), (1.3, 2.0 ** -6, 2.0 ** -7)))
        small.append(figrow(ELLIPSOID, (2.0 ** -14, 2.0 ** -13, 2.0 ** -14), (-2.0 ** -14 - step, 2.0 ** -18, 0), (0.7, 2.0 ** -6, 0)))
    T.add("tiny_figure", small)
    # d . yn == 0: through an edge of a box, where the two-component normal is perpendicular to the ray
    edge = [figrow(BOX, (1, 1, 1), (-2 * sx, 0, 0.25), (sx, sy, 0)) for sx in (-1, 1) for sy in (-1, 1)] + \
           [figrow(BOX, (1, 1, 1), (0.25, -2 * sx, 0), (0, sx, sy)) for sx in (-1, 1) for sy in (-1, 1)]
    T.add("perpendicular_normal", edge)
    # t == NaN with the figure hit: the INFINITY return
    nan = [figrow(ELLIPSOID, (0, 1, 1), (0, 0.2, -3), (0, 0, 1)), figrow(ELLIPSOID, (1, 0, 1), (0.2, 0, -3), (0, 0, 1)), figrow(ELLIPSOID, (1, 1, 1), (np.nan, 0, -3), (0, 0, 1)),
           figrow(ELLIPSOID, (1, 1, 1), (0, 0, -3), (0, np.nan, 1)), figrow(ELLIPSOID, (1, 1, 1), (-1024, 0, 0), (-2.0 ** -76, 0, 0))]
    sl = _slabs()
    low_x = sl["rows"][(sl["kind"] == sl["K"]["zero_on_low_face"]) & (sl["axis"] == 0)]
    nan += [figrow(BOX, r[0:3], r[3:6], r[6:9]) for r in low_x[:30]]
    T.add("nan_t", nan)
    return T.done()


# ---- pone ----------------------------------------------------------------------------------------------------------------------------
def ponerow(fig, y, yn):
    return np.concatenate([fig, np.asarray(y, F), np.asarray(yn, F)]).astype(F)


def _pone():
    """pdfOne on a y and yn that no hit produced: the light pdf only ever hands it the point and normal of a hit of its own ray."""
    T = Table()
    rng = np.random.default_rng(2709)
    for ftype, name in ((BOX, "box"), (ELLIPSOID, "ellipsoid"), (TRIANGLE, "triangle")):
        rows = []
        for i in range(400):
            fig, _, _, _ = _light_figure(rng, ftype, i, QUATS)
            pos = fig["position"]
            x = pos + rng.normal(size=3) * 3
            y = pos + rng.uniform(-1.5, 1.5, size=3)
            d = (y - x) * rng.choice([0.25, 1.0, 3.0]) if i % 2 else rng.normal(size=3)
            yn = rng.normal(size=3) * rng.choice([0.5, 1.0, 2.0])
            rows.append(ponerow(figrow(ftype, o=x, d=d, **fig), y, yn))
        T.add("random_" + name, np.stack(rows))
    box = dict(data=(0.5, 1, 2), position=(1, -2, 0.5), rotation=(0.5, 0.5, 0.5, 0.5))
    ell = dict(data=(0.5, 1, 2), position=(1, -2, 0.5), rotation=(0.2, 0.4, -0.6, 1.5))
    tri = dict(data=(1, 0.5, 0), data2=(-0.5, 1, 0.25), data3=(0.25, -0.5, 0), position=(0.5, 0.25, -1), rotation=(0.5, 0.5, 0.5, 0.5))
    lights = ((BOX, box), (ELLIPSOID, ell), (TRIANGLE, tri))
    x = (3.0, 0.5, -1.25)
    # y == x: the squared distance is 0, and 0 / 0 where the ray also lies in the surface
    T.add("y_equals_x", [ponerow(figrow(t, o=x, d=d, **f), x, (0, 1, 0)) for t, f in lights for d in ((0, 1, 0), (0, -2, 0), (1, 0, 0), (0, 0, 0))])
    # d . yn == +0 and -0 (|.| makes both +0: the density is inf), products that underflow to 0 or to a denormal under which the quotient
    # overflows on narrowing, and two small ones beside them
    perp = [((1, 0, 0), (0, 1, 0)), ((1, 1, 1), (-0.0, -0.0, -0.0)), ((1, -0.0, -0.0), (-0.0, 1, 1)), ((1, 2, 0), (2, -1, 0)), ((0, 0, 0), (1, 1, 1)),
            ((2.0 ** -75, 0, 0), (2.0 ** -75, 0, 0)), ((2.0 ** -74, 0, 0), (-2.0 ** -75, 0, 0)), ((1, 0, 0), (2.0 ** -149, 1, 0)),
            ((2.0 ** -60, 0, 0), (2.0 ** -60, 0, 0)), ((1, 0, 0), (-2.0 ** -100, 1, 0))]           # the last two: a quotient that still fits a float
    T.add("dot_zero", [ponerow(figrow(t, o=x, d=d, **f), (1.5, -1.5, 0.25), yn) for t, f in lights for d, yn in perp])
    # y at the ellipsoid's centre: n == 0, the point density is 1 / 0; with y == x as well, inf * 0
    centre = [ponerow(figrow(ELLIPSOID, o=x, d=(1, 0, 0), **ell), ell["position"], (1, 0, 0)), ponerow(figrow(ELLIPSOID, o=ell["position"], d=(1, 0, 0), **ell), ell["position"], (1, 0, 0)),
              ponerow(figrow(ELLIPSOID, o=x, d=(1, 0, 0), **ell), ell["position"], (0, 1, 0)), ponerow(figrow(ELLIPSOID, (1, 1, 1), x, (0, 0, 1)), (0, 0, 0), (0, 0, -1)),
              ponerow(figrow(ELLIPSOID, (1, 1, 1), x, (0, 0, 1)), (-0.0, -0.0, -0.0), (0, 0, 2))]
    T.add("ellipsoid_centre", centre)
    # figures without an area: a box with two zero half-sizes (sTotal == 0), a degenerate triangle (1 / 0), a zero radius (0 / 0 in n)
    flat = [ponerow(figrow(BOX, (0, 0, 1), x, (0, 0, 1)), (0, 0, 0.5), (0, 0, 1)), ponerow(figrow(BOX, (0, 0, 0), x, (0, 0, 1)), (0, 0, 0), (0, 0, 1)),
            ponerow(figrow(BOX, (0, 0, 1), x, (0, 0, 1)), x, (0, 0, 1)), ponerow(figrow(BOX, (-1, 1, 1), x, (0, 0, 1)), (0, 0, 1), (0, 0, 1)),
            ponerow(trirow((1, 0, 0), (1, 0, 0), (0, 0, 0), x, (0, 0, 1)), (0.5, 0, 0), (0, 0, 1)), ponerow(trirow((1, 1, 1), (2, 2, 2), (0, 0, 0), x, (0, 0, 1)), (0.5, 0.5, 0.5), (0, 0, 1)),
            ponerow(trirow((0, 0, 0), (0, 0, 0), (0, 0, 0), x, (0, 0, 1)), x, (0, 0, 1)),
            ponerow(figrow(ELLIPSOID, (0, 1, 1), x, (0, 0, 1)), (0, 0.5, 0.5), (0, 0, 1)), ponerow(figrow(ELLIPSOID, (0, 0, 0), x, (0, 0, 1)), (0, 0, 0), (0, 0, 1)),
            ponerow(figrow(ELLIPSOID, (1, 1, 1), x, (0, 0, 1), rotation=(0, 0, 0, 0)), (0.5, 0.5, 0.5), (0, 0, 1))]
    T.add("no_area", flat)
    nan, inf = np.nan, np.inf
    odd = []
    for t, f in lights:
        odd += [ponerow(figrow(t, o=x, d=(0, 0, 1), **f), (1, -2, 1), (nan, 0, 1)), ponerow(figrow(t, o=x, d=(0, 0, 1), **f), (1, -2, 1), (0, 0, inf)),
                ponerow(figrow(t, o=x, d=(0, 0, 1), **f), (1, -2, 1), (inf, 0, 1)), ponerow(figrow(t, o=x, d=(0, 0, 1), **f), (nan, -2, 1), (0, 0, 1)),
                ponerow(figrow(t, o=x, d=(0, 0, 1), **f), (inf, -2, 1), (0, 0, 1)), ponerow(figrow(t, o=x, d=(nan, 0, 1), **f), (1, -2, 1), (0, 0, 1)),
                ponerow(figrow(t, o=(1e20, 0, 0), d=(0, 0, 1), **f), (-1e20, -2, 1), (0, 0, 1)), ponerow(figrow(t, o=x, d=(0, 0, 2.0 ** -140), **f), (1, -2, 1), (0, 0, 2.0 ** -9))]
    T.add("nan_and_inf", odd)
    return T.done()


# ---- lsample -------------------------------------------------------------------------------------------------------------------------
def _lsample():
    T = Table()
    aux = []
    rng = np.random.default_rng(2707)

    def add(name, rows, seeds, primes):
        T.add(name, rows)
        aux.append(np.stack([np.asarray(seeds, np.uint64).astype(U), np.asarray(primes, np.uint64).astype(U)], axis=1))

    for ftype, name, n in ((BOX, "box", 400), (ELLIPSOID, "ellipsoid", 400), (TRIANGLE, "triangle", 200)):
        rows = []
        for i in range(n):
            fig, _, _, _ = _light_figure(rng, ftype, i, UNIT_QUATS)
            x = fig["position"] + rng.normal(size=3) * (4.0 if i % 3 else 1.2)
            rows.append(figrow(ftype, o=x, d=(0, 0, 0), **fig))
        seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        seeds[:4] = (0, 1, M31, 2 ** 32 - 1)
        add("random_" + name, np.stack(rows), seeds, np.where(np.arange(n) % 2, rng.integers(1, 2 ** 31, size=n), 0))
    # x in the plane of a box face, beside the face: the points drawn on that face (and on its opposite) are reached along the plane
    rows = []
    for i in range(300):
        s = rng.uniform(0.3, 1.5, size=3).astype(F)
        k = i % 3
        x = (rng.uniform(1.2, 3.0, size=3) * s * rng.choice([-1, 1], size=3)).astype(F)
        x[k] = s[k] * (1 if i % 2 else -1)
        q = IDENTITY if i % 4 else (0.0, 0.0, 1.0, 0.0)
        rows.append(figrow(BOX, s, x, (0, 0, 0), rotation=q))
    add("box_in_face_plane", np.stack(rows), rng.integers(1, 2 ** 31, size=300), np.zeros(300))
    # x on and just off the surface of an ellipsoid: rays that graze it
    rows = []
    for i in range(300):
        r = rng.uniform(0.3, 1.5, size=3)
        v = rng.normal(size=3)
        v = v / np.sqrt((v * v).sum())
        x = r * v * (1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, 1.001)[i % 4]
        rows.append(figrow(ELLIPSOID, r, x, (0, 0, 0)))
    add("ellipsoid_grazing", np.stack(rows), rng.integers(1, 2 ** 31, size=300), np.where(np.arange(300) % 2, rng.integers(1, 2 ** 31, size=300), 0))
    # an ellipsoid seen from far away: b^2 and 4ac are of the size of the distance squared and their difference, a few units, drowns in
    # their rounding: about every other point drawn is missed
    rows = []
    for i in range(200):
        r = rng.uniform(0.5, 1.5, size=3)
        v = rng.normal(size=3)
        x = v / np.sqrt((v * v).sum()) * (1e3, 3e3, 1e4, 1e5)[i % 4]
        rows.append(figrow(ELLIPSOID, r, x, (0, 0, 0), rotation=IDENTITY if i % 2 else (0.5, 0.5, 0.5, 0.5)))
    add("ellipsoid_far", np.stack(rows), rng.integers(1, 2 ** 31, size=200), np.where(np.arange(200) % 2, rng.integers(1, 2 ** 31, size=200), 0))
    # the face choice at its boundaries: the unit cube's u = 3 u01 on 1 (wx) and 2 (wx + wy) and a step below each; flip on u01 == 0.5
    third, two_thirds = F(1) / F(3), F(2) / F(3)
    xs = []
    for value in (third, ulp_step(third, -1), two_thirds, ulp_step(two_thirds, -1), ulp_step(third, 1), ulp_step(two_thirds, 1)):
        xs += first_outputs_for_u01(F(value))[:3]
    seeds = [seed_for_first(x) for x in xs]
    cube = figrow(BOX, (1, 1, 1), (3.5, -2.25, 1.75), (0, 0, 0))
    add("box_u_boundary", np.tile(cube, (len(seeds), 1)), seeds, np.zeros(len(seeds)))
    add("box_u_zero", np.stack([figrow(BOX, s, (3.5, -2.25, 1.75), (0, 0, 0)) for s in ((1, 1, 1), (0.5, 1, 2))]), [seed_for_first(1)] * 2, [0, 0])
    x2s = []
    for value in (F(0.5), ulp_step(F(0.5), -1), ulp_step(F(0.5), 1)):
        x2s += first_outputs_for_u01(F(value))[:4]
    seeds = [seed_for_first(seed_for_first(x)) for x in x2s]
    add("box_flip_half", np.tile(cube, (len(seeds), 1)), seeds, np.zeros(len(seeds)))
    tri = trirow((1, 0.5, 0), (-0.5, 1, 0.25), (0.25, -0.5, 0), (2.0, 1.5, 3.0), (0, 0, 0), position=(0.5, 0.25, -1), rotation=(0.5, 0.5, 0.5, 0.5))
    for name, seeds in FOLD_SEEDS.items():
        add("fold_" + name, np.tile(tri, (len(seeds), 1)), seeds, np.zeros(len(seeds)))
    return T.done(aux=np.ascontiguousarray(np.concatenate(aux), U))


# ---- the box's face point -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def face_point_cases():
    """Half-sizes and seeds for one round's point of BoxLight::sample, which the reference keeps in a local of its loop: no entry of the
    compiled reference can return it, so these cases are answered by the oracle alone (rto_box_face_point, the lines its sampler runs)
    and are not in the fixture.  The reference's say on the same lines is the lsample family, whose directions come from these points.
    Returns s (n x 3), seeds (n), and the kind of each row."""
    rng = np.random.default_rng(2710)
    fam = families()["lsample"]
    edge = np.isin(fam["kind"], [fam["K"][k] for k in ("box_u_boundary", "box_u_zero", "box_flip_half")])
    edge_seeds = fam["aux"][edge, 0]
    n = 600
    s = np.concatenate([rng.uniform(0.3, 2.0, size=(n, 3)), np.ones((len(edge_seeds), 3)), np.tile([[0.5, 1, 2]], (len(edge_seeds), 1)),
                        [[0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, 1], [0, 0, 0], [np.inf, 1, 1], [np.nan, 1, 1]]]).astype(F)
    seeds = np.concatenate([rng.integers(0, 2 ** 32, size=n, dtype=np.uint64), edge_seeds, edge_seeds, np.arange(11, 18)]).astype(U)
    kind = np.concatenate([np.zeros(n, int), np.ones(len(edge_seeds), int), np.full(len(edge_seeds), 2), np.full(7, 3)])
    for a in (s, seeds, kind):
        a.setflags(write=False)
    return s, seeds, kind


def face_point_oracle():
    s, seeds, _ = face_point_cases()
    out = np.zeros((len(s), 4), U)
    _call(oracle_lib.lib(), "rto_box_face_point", np.ascontiguousarray(s), np.ascontiguousarray(seeds), len(s), out)
    return out


# ---- cosine --------------------------------------------------------------------------------------------------------------------------
def drawn_unit_vector(seed):
    """The unit vector Cosine::sample draws first with engine(seed) and a fresh normal_distribution, through the oracle's own draws; the
    norm and the scaling are float32 operations that numpy rounds as the reference does (one root, one division, three products)."""
    L = oracle_lib.lib()
    abc = np.zeros(3, F)
    L.rto_rng_kat_normals_first(int(seed), 3, 0, abc.ctypes.data)
    l2 = (abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2]
    return (F(1.0 / np.float64(np.sqrt(np.float64(l2)).astype(F)))) * abc


def _cosine():
    T = Table()
    aux = []
    rng = np.random.default_rng(2708)
    n = 900
    v = rng.normal(size=(n, 3))
    normals = (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(F)
    normals[::7] *= F(2.5)
    normals[3::11] = F([0, 0, 1])
    T.add("random", normals)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    seeds[:4] = (0, 1, M31, 2 ** 32 - 1)
    aux.append(np.stack([seeds.astype(U), np.where(np.arange(n) % 2, rng.integers(1, 2 ** 31, size=n), 0).astype(U)], axis=1))
    back, back_seeds = [], []
    for seed in (1, 7, 4242, 12345, 99991, 2147483646, 31337, 271828):
        w = drawn_unit_vector(seed)
        for k in range(-1, 3):
            for c in range(3):
                nn = -w
                if k:
                    nn = nn.copy()
                    nn[c] = from_bits(U(int(bits(nn[c:c + 1])[0]) + (k if k < 2 else 64)))[0]
                back.append(nn)
                back_seeds.append(seed)
    T.add("opposite", np.stack(back))
    aux.append(np.stack([np.asarray(back_seeds, U), np.zeros(len(back), U)], axis=1))
    odd = [[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [1e-30, 0, 0], [0, -1e20, 0], [1e20, 1e20, 1e20], [-0.0, -0.0, -0.0]]
    T.add("odd_normals", odd)
    aux.append(np.stack([np.arange(5, 5 + len(odd), dtype=U), np.zeros(len(odd), U)], axis=1))
    return T.done(aux=np.ascontiguousarray(np.concatenate(aux), U))


@functools.lru_cache(maxsize=None)
def families():
    fam = {"quad": _quad(), "slabs": _slabs(), "fig": _fig(), "tri5": _tri5(), "lpdf": _lpdf(), "pone": _pone(), "lsample": _lsample(), "cosine": _cosine()}
    assert sum(len(f["rows"]) for f in fam.values()) <= 40000
    return fam


def rows(name):
    return families()[name]["rows"]


def aux(name):
    return families()[name]["aux"]


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
def _call(lib, fn, *args):
    f = getattr(lib, fn)
    f.argtypes = [C.c_size_t if isinstance(a, int) else (type(a) if isinstance(a, C.c_uint32) else C.c_void_p) for a in args]
    f.restype = C.c_int
    return f(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])


def _not_triangle(r):
    return np.flatnonzero(r[:, 0] != TRIANGLE)


@functools.lru_cache(maxsize=None)
def _ref_lib(hw):
    p = oracle_lib.ref_path(f"libref_funcs_hw{hw}.so")
    return C.CDLL(p) if p else None


def reference_built():
    return all(_ref_lib(hw) is not None and hasattr(_ref_lib(hw), "reff_quad") for hw in range(1, 6)) and hasattr(_ref_lib(5), "reff_pdf_one")


def evaluate(which):
    """The answers of every family through the oracle (`oracle`) or the compiled reference's harnesses (`reference`): name -> n x WIDTH
    uint32.  With the reference, the sampler rows first go through the oracle under a bound on the figure tests: the reference itself
    would loop for ever on a row whose light cannot be hit."""
    ref = which == "reference"
    assert which in ("oracle", "reference")
    O = oracle_lib.lib()
    out = {k: np.zeros((len(rows(k)), WIDTH[k]), U) for k in FAMILIES}

    def run(hw, fn, name, cols, r, *more, only=None):
        """One entry point on the rows `only` of a family into the columns `cols` of its answers."""
        idx = np.arange(len(r)) if only is None else only
        sub = np.ascontiguousarray(r[idx])
        extra = [np.ascontiguousarray(m[idx]) for m in more]
        ans = np.zeros((len(idx), cols.stop - cols.start), U)
        if ref:
            args = [sub, len(idx), ans] if not extra else [sub] + extra + [len(idx), ans]
            _call(_ref_lib(hw), "reff_" + fn, *args)
        elif fn == "lsample":
            over = _call(O, f"rto_hw{hw}_lsample", sub, extra[0], len(idx), C.c_uint32(MAX_DRAWS), ans, None)
            assert over == 0, (name, hw, over)
        else:
            args = [sub, len(idx), ans] if not extra else [sub] + extra + [len(idx), ans]
            _call(O, f"rto_hw{hw}_{fn}", *args)
        out[name][idx, cols] = ans

    run(2, "quad", "quad", slice(0, 2), rows("quad"))
    run(3, "quad", "quad", slice(2, 4), rows("quad"))
    run(5 if ref else 3, "slabs", "slabs", slice(0, 2), rows("slabs"))
    for hw in range(1, 6):
        run(hw, "fig", "fig", slice(5 * (hw - 1), 5 * hw), rows("fig"))
    run(5, "fig", "tri5", slice(0, 5), rows("tri5"))
    r = rows("lpdf")
    run(4, "lpdf", "lpdf", slice(0, 1), r, only=_not_triangle(r))
    run(5, "lpdf", "lpdf", slice(1, 2), r)
    r = rows("pone")
    run(4, "pdf_one", "pone", slice(0, 1), r, only=_not_triangle(r))
    run(5, "pdf_one", "pone", slice(1, 2), r)
    r, a = rows("lsample"), aux("lsample")
    if ref:
        evaluate("oracle")                                              # asserts that every row's loop ends
    run(4, "lsample", "lsample", slice(0, 8), r, a, only=_not_triangle(r))
    run(5, "lsample", "lsample", slice(8, 16), r, a)
    r, a = rows("cosine"), aux("cosine")
    run(4, "cosine", "cosine", slice(0, 8), r, a)
    run(5, "cosine", "cosine", slice(8, 16), r, a)
    return out


@functools.lru_cache(maxsize=None)
def oracle_answers():
    out = evaluate("oracle")
    for v in out.values():
        v.setflags(write=False)
    return out


def attempts():
    """The figure tests of every lsample row (hw4's for boxes and ellipsoids, hw5's for all), from the oracle: n x 2."""
    O = oracle_lib.lib()
    r, a = rows("lsample"), aux("lsample")
    out = np.zeros((len(r), 2), U)
    for col, hw, idx in ((0, 4, _not_triangle(r)), (1, 5, np.arange(len(r)))):
        ans, att = np.zeros((len(idx), 8), U), np.zeros(len(idx), U)
        assert _call(O, f"rto_hw{hw}_lsample", np.ascontiguousarray(r[idx]), np.ascontiguousarray(a[idx]), len(idx), C.c_uint32(MAX_DRAWS), ans, att) == 0
        out[idx, col] = att
    return out


def draws(seeds, states):
    """Engine steps from minstd_rand(seed) to `state`, per row; fails beyond MAX_DRAWS."""
    s = np.asarray(seeds, np.uint64) % np.uint64(M31)
    s[s == 0] = 1
    target = np.asarray(states, np.uint64)
    count = np.full(len(s), -1, np.int64)
    for k in range(MAX_DRAWS + 1):
        count[(count < 0) & (s == target)] = k
        if (count >= 0).all():
            break
        s = s * np.uint64(A) % np.uint64(M31)
    assert (count >= 0).all(), f"{int((count < 0).sum())} sampler rows did not reach their state within {MAX_DRAWS} draws"
    return count


def light_hits(r):
    """For every lpdf row, whether the light pdf's first query hits the figure (with a t that is no NaN) and whether its second one, from
    x + float(t + 1e-4) d, does: by the oracle's hw5 figure test (the sum in double, as hw4 forms it; one float product and sum per axis)."""
    O = oracle_lib.lib()
    h1 = np.zeros((len(r), 5), U)
    _call(O, "rto_hw5_fig", np.ascontiguousarray(r), len(r), h1)
    t1 = _f(h1[:, 1])
    first = ((h1[:, 0] & 1) != 0) & ~np.isnan(t1)
    r2 = np.array(r, F)
    with np.errstate(all="ignore"):
        r2[:, 17:20] = r[:, 17:20] + (t1.astype(np.float64) + 1e-4).astype(F)[:, None] * r[:, 20:23]
    h2 = np.zeros((len(r), 5), U)
    _call(O, "rto_hw5_fig", np.ascontiguousarray(r2), len(r), h2)
    return first, first & ((h2[:, 0] & 1) != 0) & (r[:, 0] != TRIANGLE)


def differing(got, want):
    """Indices of the rows on which two answers differ: other than equal words, or NaN in the same float on both sides (a flag word or
    an engine state read as a float is never a NaN: both are below 2^31 - 1 < 0x7f800001)."""
    got, want = np.ascontiguousarray(got, U), np.ascontiguousarray(want, U)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = (got == want) | (np.isnan(got.view(F)) & np.isnan(want.view(F)))
    return np.flatnonzero(~same.all(axis=1))


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def _f(col):
    return np.ascontiguousarray(col, U).view(F)


def reaches(name, answers):
    """Counts, over the reference's answers, of the branches the family claims to reach (test_analytic_pins.py asserts on them)."""
    fam, a = families()[name], np.asarray(answers[name])
    kind, K = fam["kind"], fam["K"]
    of = lambda k: kind == K[k]
    hit = lambda c: (a[:, c] & 1) != 0
    inside = lambda c: (a[:, c] & 2) != 0
    r = {"rows": len(a)}
    if name == "quad":
        t2, t3 = _f(a[:, 1]), _f(a[:, 3])
        r.update(hit=int(hit(2).sum()), miss=int((~hit(2)).sum()), inside=int(inside(2).sum()), outside=int((hit(2) & ~inside(2)).sum()),
                 discriminant_zero_rejected=int((of("discriminant_zero") & ~hit(0) & ~hit(2)).sum()), discriminant_zero_rows=int(of("discriminant_zero").sum()),
                 discriminant_denormal_hit=int((of("discriminant_denormal") & hit(2)).sum()),
                 nan_t_outside=int((hit(2) & np.isnan(t3) & ~inside(2)).sum()), nan_t_inside=int((hit(2) & np.isnan(t3) & inside(2)).sum()),
                 a_zero_hit=int((of("a_zero") & hit(2)).sum()), a_zero_miss=int((of("a_zero") & ~hit(2)).sum()),
                 a_negative_hit=int((fam["rows"][:, 0] < 0)[hit(2)].sum()),
                 minus_zero_outside=(int((hit(0) & ~inside(0) & (a[:, 1] == 0x80000000)).sum()), int((hit(2) & ~inside(2) & (a[:, 3] == 0x80000000)).sum())),
                 minus_zero_inside=int((hit(2) & inside(2) & (a[:, 3] == 0x80000000)).sum()), plus_zero=int((hit(2) & (a[:, 3] == 0)).sum()),
                 forms_differ_in_t=int((hit(0) & hit(2) & (a[:, 1] != a[:, 3]) & ~np.isnan(t2) & ~np.isnan(t3)).sum()),
                 forms_differ_in_flags=int((a[:, 0] != a[:, 2]).sum()))
    elif name == "slabs":
        t = _f(a[:, 1])
        axis = fam["axis"]
        low, high = of("zero_on_low_face"), of("zero_on_high_face")
        r.update(accepted=int(hit(0).sum()), rejected=int((~hit(0)).sum()), inside=int(inside(0).sum()),
                 nan_accepted_per_axis=[int((hit(0) & low & (axis == k)).sum()) for k in range(3)], nan_rejected_per_axis=[int((~hit(0) & low & (axis == k)).sum()) for k in range(3)],
                 nan_t_per_axis=[int((np.isnan(t) & low & (axis == k)).sum()) for k in range(3)], high_face_accepted=int((hit(0) & high).sum()),
                 graze_accepted=int((of("graze_edge") & hit(0)).sum()),
                 zero_t=(int((hit(0) & ~inside(0) & (a[:, 1] == 0)).sum()), int((hit(0) & ~inside(0) & (a[:, 1] == 0x80000000)).sum()),
                         int((hit(0) & inside(0) & (a[:, 1] == 0)).sum()), int((hit(0) & inside(0) & (a[:, 1] == 0x80000000)).sum())))
    elif name == "fig":
        ftype = fam["rows"][:, 0].astype(int)
        t3, t4 = _f(a[:, 11]), _f(a[:, 16])
        n3 = _f(a[:, 12:15])
        ncomp = (n3 != 0).sum(axis=1)
        tmax = from_bits(U(T_MAX_BITS))[0]
        plane = ftype == PLANE
        r.update(hit_per_type=[int((hit(10) & (ftype == k)).sum()) for k in range(3)], miss_per_type=[int((~hit(10) & (ftype == k)).sum()) for k in range(3)],
                 inside_per_type=[int((inside(10) & (ftype == k)).sum()) for k in range(3)],
                 ellipsoid_tangent_miss=int((of("ellipsoid_tangent") & ~hit(10)).sum()),
                 nan_t_hit_outside=int((hit(10) & np.isnan(t3) & ~inside(10)).sum()), ellipsoid_a_zero_rows=int(of("ellipsoid_a_zero").sum()),
                 box_two_components=int((of("box_edge") & hit(10) & (ncomp == 2)).sum()), box_three_components=int((of("box_corner") & hit(10) & (ncomp == 3)).sum()),
                 box_zero_size_nan_normal=int((of("box_zero_size") & hit(10) & np.isnan(n3).any(axis=1)).sum()),
                 plane_inf_t_hw3_only=int((plane & hit(10) & np.isinf(t3) & ~hit(15)).sum()), plane_dn_zero_nan_miss=int((of("plane_dn_zero") & ~hit(10)).sum()),
                 plane_t_below_tmax=int((of("plane_t_max") & hit(15) & (t4 < tmax)).sum()),
                 plane_t_at_or_above_tmax_hw3_only=(int((of("plane_t_max") & hit(10) & ~hit(15) & (t3 == tmax)).sum()), int((of("plane_t_max") & hit(10) & ~hit(15) & (t3 > tmax)).sum())),
                 plane_t_zero_miss=int((of("plane_t_zero") & ~hit(10)).sum()), plane_t_zero_hit=int((of("plane_t_zero") & hit(10)).sum()),
                 hw1_differs_from_hw2_in_t=int((hit(0) & hit(5) & (a[:, 1] != a[:, 6])).sum()),
                 hw1_plane_normal_not_unit_hit=int((plane & hit(0) & (np.abs((fam["rows"][:, 1:4].astype(np.float64) ** 2).sum(axis=1) - 1) > 0.1)).sum()),
                 hw2_differs_from_hw3=int((a[:, 5:10] != a[:, 10:15]).any(axis=1).sum()), hw3_differs_from_hw4=int((a[:, 10:15] != a[:, 15:20]).any(axis=1).sum()),
                 hw4_differs_from_hw5=int(differing(a[:, 15:20], a[:, 20:25]).size),
                 quaternions={str(q): int((fam["rows"][:, 13:17] == F(q)).all(axis=1).sum()) for q in QUATS})
    elif name == "tri5":
        t = _f(a[:, 1])
        rw = fam["rows"]
        tmax = from_bits(U(T_MAX_BITS))[0]
        g = np.flatnonzero(of("edge_grid"))
        # the edge grid is exact: p = (px, py, 0) and the three tests are on py (along b), px (along c) and 1 - px - py (the third edge)
        px, py = rw[g, 17], rw[g, 18]
        on = lambda cond: (int((cond & hit(0)[g]).sum()), int((cond & ~hit(0)[g]).sum()))
        body = (px > 0) & (py > 0) & (px + py < 1)
        r.update(hit=int(hit(0).sum()), miss=int((~hit(0)).sum()), inside=int(inside(0).sum()), outside=int((hit(0) & ~inside(0)).sum()),
                 edge_b_plus_zero=on((bits(py) == 0) & (px > 0) & (px < 1)), edge_b_minus_zero=on((bits(py) == 0x80000000) & (px > 0) & (px < 1)),
                 edge_c_plus_zero=on((bits(px) == 0) & (py > 0) & (py < 1)), edge_c_minus_zero=on((bits(px) == 0x80000000) & (py > 0) & (py < 1)),
                 edge_third=on((px > 0) & (py > 0) & (px.astype(np.float64) + py.astype(np.float64) == 1)),
                 beside_edges=on(((np.abs(px) == F(2.0 ** -149)) | (np.abs(py) == F(2.0 ** -149))) & (px < 1) & (py < 1)), body=on(body),
                 degenerate_miss=int((of("degenerate") & ~hit(0)).sum()),
                 t_below_tmax=int((of("t_max") & hit(0) & (t < tmax)).sum()), t_max_miss=int((of("t_max") & ~hit(0)).sum()),
                 windings=(int((of("edge_grid") & hit(0) & inside(0)).sum()), int((of("edge_grid") & hit(0) & ~inside(0)).sum())))
    elif name == "lpdf":
        p4, p5 = _f(a[:, 0]), _f(a[:, 1])
        ftype = fam["rows"][:, 0].astype(int)
        first, second = light_hits(fam["rows"])
        one, two = first & ~second & np.isfinite(p5), first & second & np.isfinite(p5)
        r.update(first_hit_only_per_type=[int((one & (ftype == k)).sum()) for k in (BOX, ELLIPSOID)], second_hit_per_type=[int((two & (ftype == k)).sum()) for k in (BOX, ELLIPSOID)],
                 inside_rows_first_hit_only=int(((of("inside_box") | of("inside_ellipsoid")) & one).sum()),
                 tiny_first_t_rows=int(of("tiny_first_t").sum()), tiny_figure_rows=int(of("tiny_figure").sum()),
                 tiny_first_t_second_hit=int((of("tiny_first_t") & two).sum()), tiny_figure_second_hit=int((of("tiny_figure") & two).sum()),
                 zero=int((a[:, 1] == 0).sum()), positive_per_type=[int(((p5 > 0) & (ftype == k)).sum()) for k in (BOX, ELLIPSOID, TRIANGLE)],
                 infinite_from_nan_t=int((of("nan_t") & np.isinf(p5)).sum()), infinite_from_nan_t_hw4=int((of("nan_t") & np.isinf(p4)).sum()),
                 infinite_from_perpendicular_normal=int((of("perpendicular_normal") & np.isinf(p5)).sum()),
                 inside_rows_positive=int(((of("inside_box") | of("inside_ellipsoid")) & (p5 > 0) & np.isfinite(p5)).sum()),
                 triangle_positive=int(((ftype == TRIANGLE) & (p5 > 0)).sum()), hw4_differs_from_hw5=int(differing(a[ftype != TRIANGLE, 0:1], a[ftype != TRIANGLE, 1:2]).size))
    elif name == "pone":
        p4, p5 = _f(a[:, 0]), _f(a[:, 1])
        ftype = fam["rows"][:, 0].astype(int)
        finite = np.isfinite(p5) & (p5 > 0)
        r.update(positive_finite_per_type=[int((finite & (ftype == k)).sum()) for k in (BOX, ELLIPSOID, TRIANGLE)],
                 y_equals_x_zero=int((of("y_equals_x") & (a[:, 1] == 0)).sum()), y_equals_x_nan=int((of("y_equals_x") & np.isnan(p5)).sum()),
                 dot_zero_infinite=int((of("dot_zero") & np.isinf(p5)).sum()), dot_zero_finite=int((of("dot_zero") & finite).sum()),
                 ellipsoid_centre_infinite=int((of("ellipsoid_centre") & np.isinf(p5)).sum()), ellipsoid_centre_nan=int((of("ellipsoid_centre") & np.isnan(p5)).sum()),
                 no_area_not_finite=int((of("no_area") & ~np.isfinite(p5)).sum()), nan=int(np.isnan(p5).sum()), infinite=int(np.isinf(p5).sum()),
                 hw4_differs_from_hw5=int(differing(a[ftype != TRIANGLE, 0:1], a[ftype != TRIANGLE, 1:2]).size), kinds={k: int(of(k).sum()) for k in K})
    elif name == "lsample":
        ftype = fam["rows"][:, 0].astype(int)
        n4 = draws(fam["aux"][ftype != TRIANGLE, 0], a[ftype != TRIANGLE, 3])
        n5 = draws(fam["aux"][:, 0], a[:, 11])
        box = ftype == BOX
        r.update(max_draws=(int(n4.max()), int(n5.max())), box_rejecting=int((n5[box] > 4).sum()), box_draws_not_multiple_of_4=int((n5[box] % 4 != 0).sum()),
                 box_in_face_plane_rejecting=int((n5[of("box_in_face_plane")] > 4).sum()), triangle_draws_not_2=int((n5[ftype == TRIANGLE] != 2).sum()),
                 cache_used=int(((a[:, 14] == 1) & (a[:, 12] == 0)).sum()), cache_left=int(((a[:, 14] == 0) & (a[:, 12] == 1)).sum()),
                 hw4_cache_changed=int(((ftype == ELLIPSOID) & (a[:, 4:6] != a[:, 6:8]).any(axis=1)).sum()),
                 box_cache_untouched=int((box & (a[:, 12:14] == a[:, 14:16]).all(axis=1) & (a[:, 4:6] == a[:, 6:8]).all(axis=1)).sum()), box_rows=int(box.sum()),
                 hw4_differs_from_hw5=int((a[ftype != TRIANGLE, 0:6] != a[ftype != TRIANGLE, 8:14]).any(axis=1).sum()),
                 kinds={k: int(of(k).sum()) for k in K})
    elif name == "cosine":
        n = fam["rows"]
        fell_back = (a[:, 8:11] == bits(n)).all(axis=1)
        r.update(fallback=int(fell_back.sum()), fallback_opposite=int((fell_back & of("opposite")).sum()), opposite_not_fallback=int((~fell_back & of("opposite")).sum()),
                 cache_used=int(((a[:, 14] == 1)).sum()), hw4_differs_from_hw5=int(differing(a[:, 0:8], a[:, 8:16]).size))
    return r

"""The inputs on which the intersection layer is pinned and its exactness gate is checked: one table for the golden generator
(golden/make_goldens.py -> pins_intersection_edges.npz), the host pins (test_intersection_pins.py) and the GPU tests
(test_gpu_intersection.py).  hw8's tests only.  Everything is deterministic: fixed seeds, float32 rows.

families()   box    mn, mx, o, d            AABB::intersect: accepted, is_inside, t                       (primitives.cpp:163-165,29-53)
             tri    positions[9], o, d      Figure::intersect of a triangle: hit, is_inside, t, u, v      (primitives.cpp:76-125)
A family is a dict: rows (n x 12 or n x 15 float32), kind (a small integer per row: which edge the row was built for, KINDS[family] names
them), axis (the axis a `box` row's special direction component lies on, -1 for none), scale (the row's M).

u and v are read from the reference as the texcoords of a figure whose corners carry (1,0), (0,1), (0,0): 0 + u * 1 + v * 0 and
0 + u * 0 + v * 1 in float.  That is u and v bit for bit, except that a -0 becomes +0 and a NaN in one reaches the other; `as_texcoords`
applies the same two sums to a (u, v) pair from elsewhere (the device), so the comparison stays one of bits.

gate_rows(M, n, seed)     the soundness cases of the gate: lo hi o d t gap c2 cull_k, what rtt_hit_stands takes (gap filled by the test)
grown_boxes(rows, M, seed)  per row the triangle's own box and three grown copies of it
box_rows(M, n, seed)      the `box` family's random part at any size, no direction component below 1e-30: the padded slab test's cases
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib

F = np.float32
SCALES = (1.0, 10.0, 1000.0)
T_MAX = F(1e4)
MAGIC1 = F([0.239, 0.419, 0.533])
MAGIC2 = F([0.35743, 0.66682, 0.69695])
KINDS = {
    "box": ("face", "edge", "corner", "origin_inside", "on_entry_face", "on_exit_face", "behind", "graze", "odd_direction", "far_origin",
            "zero_inside_slab", "zero_outside_low", "zero_outside_high", "zero_on_low_face", "zero_on_high_face"),
    "tri": ("inside", "outside", "vertex", "edge_u0", "edge_v0", "edge_uv1", "in_plane", "t_near_zero", "t_near_tmax", "two_equal", "collinear",
            "zero_area", "a2_zero", "den_zero", "near_singular"),
}
K = {fam: {name: i for i, name in enumerate(names)} for fam, names in KINDS.items()}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulp_step(x, k):
    """x moved by k units in the last place (x > 0, finite)."""
    return (bits(x).astype(np.int64) + k).astype(np.uint32).view(F)


def log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def unit64(a):
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        return a / np.linalg.norm(a, axis=-1, keepdims=True)


def lattice(M):
    """A power of two no larger than M / 64: coordinates that are small integers times it add, subtract and halve exactly."""
    return 2.0 ** np.floor(np.log2(M / 64.0))


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------
def random_boxes(rng, M, n, flat=(0.4, 0.3, 0.2, 0.1)):
    """Boxes inside [-M, M]^3, each side log-uniform from 1e-6 M to M; `flat`: the shares of boxes with 0, 1, 2, 3 flat axes."""
    size = log_uniform(rng, 1e-6 * M, M, (n, 3))
    n_flat = rng.choice(4, n, p=flat)
    order = np.argsort(rng.random((n, 3)), axis=1)                       # a random choice of which axes are flat
    size[order < n_flat[:, None]] = 0.0
    lo = (rng.uniform(-M, M - size)).astype(F)
    hi = np.minimum((lo.astype(np.float64) + size).astype(F), F(M))
    hi = np.where(size == 0, lo, hi)
    return lo, hi


def aimed(rng, o, target, n):
    """d from o towards target, of a length between 0.07 and 15 (float32)."""
    length = log_uniform(rng, 0.07, 15.0, (n, 1))
    with np.errstate(all="ignore"):
        d = unit64(np.asarray(target, np.float64) - np.asarray(o, np.float64)) * length
    return np.nan_to_num(d, nan=0.3).astype(F)


def floor_direction(d):
    """No component below 1e-30 in magnitude (the sign is kept, +0 counts as positive)."""
    d = np.asarray(d, F).copy()
    small = np.abs(d) < F(1e-30)
    d[small] = np.copysign(F(1e-30), d[small])
    return d


def _point_in_box(rng, lo, hi, pin):
    """A point of each box; pin[:, k] = -1 / +1 puts coordinate k on the low / high face, 0 leaves it uniform inside."""
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    p = rng.uniform(lo64, np.maximum(hi64, lo64))
    return np.where(pin < 0, lo64, np.where(pin > 0, hi64, p))


def box_rows(M, n, seed):
    """The random part of the `box` family: rays aimed at faces, edges and corners of random boxes (hits and near misses alike), origins
    inside, boxes behind the ray, origins far away.  No direction component below 1e-30.  Returns rows (n x 12) and kind (n)."""
    rng = np.random.default_rng(seed)
    lo, hi = random_boxes(rng, M, n)
    kind = rng.choice([K["box"][k] for k in ("face", "edge", "corner", "origin_inside", "behind", "far_origin")], n, p=(0.3, 0.2, 0.15, 0.15, 0.1, 0.1))
    n_pinned = np.select([kind == K["box"]["edge"], kind == K["box"]["corner"]], [2, 3], 1)
    order = np.argsort(rng.random((n, 3)), axis=1)
    pin = np.where(order < n_pinned[:, None], rng.choice([-1, 1], (n, 3)), 0)
    target = _point_in_box(rng, lo, hi, pin)
    # a third of the aimed rays pass the target by up to a box size: near misses of the face, edge or corner
    off = rng.random(n) < 0.33
    size = np.maximum((hi - lo).astype(np.float64).max(axis=1), 1e-6 * M)
    target = target + np.where(off[:, None], rng.normal(size=(n, 3)) * (size * log_uniform(rng, 1e-7, 1.0, n))[:, None], 0.0)
    o = rng.uniform(-M, M, (n, 3))
    inside = kind == K["box"]["origin_inside"]
    o = np.where(inside[:, None], _point_in_box(rng, lo, hi, np.zeros((n, 3), int)), o)
    far = kind == K["box"]["far_origin"]
    o = np.where(far[:, None], target + unit64(rng.normal(size=(n, 3))) * log_uniform(rng, 10 * M, 1e4 * M, (n, 1)), o)
    o = o.astype(F)
    d = aimed(rng, o, np.where(inside[:, None], o + rng.normal(size=(n, 3)), target), n)
    d = np.where((kind == K["box"]["behind"])[:, None], -d, d)
    return np.concatenate([lo, hi, o, floor_direction(d)], axis=1).astype(F), kind


def _box_exact(M, seed, n):
    """Boxes and rays on a lattice, so that the slab distances are exact: origins on the entry and on the exit face (t1 == 0, t2 == 0, of
    either sign of zero: the sign is the direction component's), and rays that touch an edge or a corner only (t1 == t2)."""
    rng = np.random.default_rng(seed)
    q = lattice(M)
    lo = rng.integers(-30, 20, (n, 3)) * 2
    size = rng.integers(1, 6, (n, 3)) * 2
    size[rng.random((n, 3)) < 0.15] = 0                                  # some flat axes
    hi = lo + size
    kind = rng.choice([K["box"]["on_entry_face"], K["box"]["on_exit_face"], K["box"]["graze"]], n)
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)
    d = rng.choice([-4, -2, -1, 1, 2, 4], (n, 3)).astype(np.float64)
    o = lo + rng.integers(0, 2, (n, 3)) * (size // 2)                    # inside or on a face, a lattice point
    side = rng.integers(0, 2, n)                                         # which face of `axis` the origin lies on
    face = np.where(side == 0, lo[rows, axis], hi[rows, axis])
    o[rows, axis] = face
    sign = np.where(side == 0, 1.0, -1.0)                                # pointing into the box from that face
    sign = np.where(kind == K["box"]["on_exit_face"], -sign, sign)
    d[rows, axis] = sign * np.abs(d[rows, axis])
    # grazing: the ray meets the box in one point of an edge: it enters on `axis` where it leaves on the next axis
    g = kind == K["box"]["graze"]
    nxt = (axis + 1) % 3
    touch = o.astype(np.float64)                                         # on the face of `axis`; put it on the far face of `nxt` in d's sense too
    d_n = d[rows, nxt]
    touch[rows, nxt] = np.where(g, np.where(d_n > 0, hi[rows, nxt], lo[rows, nxt]), touch[rows, nxt])
    steps = rng.choice([1, 2, 4, 8], n)
    o64 = np.where(g[:, None], touch - d * steps[:, None], o)
    mn, mx = (lo * q).astype(F), (hi * q).astype(F)
    return np.concatenate([mn, mx, (o64 * q).astype(F), (d * rng.choice([0.25, 1.0, 2.0], (n, 1))).astype(F)], axis=1).astype(F), kind, np.full(n, -1)


def _box_odd_directions(M, seed, n):
    """Direction components of +-0, +-1e-30, denormals and 1e30 on one axis (the others ordinary), the origin anywhere."""
    rng = np.random.default_rng(seed)
    rows, kind = box_rows(M, n, seed + 1)
    axis = rng.integers(0, 3, n)
    odd = F([0.0, -0.0, 1e-30, -1e-30, 1e-45, -1e-45, 3e-39, -3e-39, 1e30, -1e30])
    rows[np.arange(n), 9 + axis] = odd[rng.integers(0, len(odd), n)]
    return rows, np.full(n, K["box"]["odd_direction"]), axis


def _box_zero_component(M, seed, n_each):
    """For every axis on its own: d_k = +-0 with the origin inside the slab, outside it on either side, and exactly on either face (0/0:
    the reference forms a NaN there, and std::max's operand order decides which axis's NaN swallows the others).  The other two axes are
    aimed through the box's inside for half of the rows and past the box for the rest."""
    rng = np.random.default_rng(seed)
    q = lattice(M)
    out_rows, out_kind, out_axis = [], [], []
    places = ("zero_inside_slab", "zero_outside_low", "zero_outside_high", "zero_on_low_face", "zero_on_high_face")
    for axis in range(3):
        for place in places:
            n = n_each
            lo = rng.integers(-30, 20, (n, 3)) * 2
            size = rng.integers(1, 6, (n, 3)) * 2
            hi = lo + size
            target = lo + size / 2.0 + rng.uniform(-0.45, 0.45, (n, 3)) * size
            miss = rng.random(n) < 0.5
            other = (axis + 1 + rng.integers(0, 2, n)) % 3
            target[np.arange(n), other] += np.where(miss, size[np.arange(n), other] * rng.choice([-1.5, 1.5], n), 0.0)
            o = target + rng.normal(size=(n, 3)) * 8.0
            where = {"zero_inside_slab": lo[:, axis] + size[:, axis] / 2.0, "zero_outside_low": lo[:, axis] - 3.0, "zero_outside_high": hi[:, axis] + 3.0,
                     "zero_on_low_face": lo[:, axis].astype(np.float64), "zero_on_high_face": hi[:, axis].astype(np.float64)}[place]
            o[:, axis] = where
            o32 = (o * q).astype(F)
            o32[:, axis] = (where * q).astype(F)                         # exact: a lattice point
            d = aimed(rng, o32, target * q, n)
            d[:, axis] = np.where(rng.random(n) < 0.5, F(0.0), F(-0.0))
            out_rows.append(np.concatenate([(lo * q).astype(F), (hi * q).astype(F), o32, d], axis=1))
            out_kind.append(np.full(n, K["box"][place]))
            out_axis.append(np.full(n, axis))
    return np.concatenate(out_rows).astype(F), np.concatenate(out_kind), np.concatenate(out_axis)


def _box():
    rows, kind, axis, scale = [], [], [], []
    for i, M in enumerate(SCALES):
        r, k = box_rows(M, 1800, 8200 + i)
        parts = [(r, k, np.full(len(k), -1)), _box_exact(M, 8210 + i, 600), _box_odd_directions(M, 8220 + i, 300), _box_zero_component(M, 8230 + i, 40)]
        for r, k, a in parts:
            rows.append(r); kind.append(k); axis.append(a); scale.append(np.full(len(k), M))
    return dict(rows=np.ascontiguousarray(np.concatenate(rows), F), kind=np.concatenate(kind).astype(np.int32), axis=np.concatenate(axis).astype(np.int32),
                scale=np.concatenate(scale).astype(F))


# ---- triangles ------------------------------------------------------------------------------------------------------------------------
def kernel_direction():
    """magic1 x magic2: the direction the reference's barycentric solve projects along."""
    return unit64(np.cross(MAGIC1.astype(np.float64), MAGIC2.astype(np.float64)))


def float_dot3(m, b):
    """m[0] * b.x + m[1] * b.y + m[2] * b.z in float32, left to right (primitives.cpp:97-103)."""
    b = np.asarray(b, F)
    with np.errstate(all="ignore"):
        return (m[0] * b[..., 0] + m[1] * b[..., 1]) + m[2] * b[..., 2]


def _random_triangles(rng, M, n):
    """Corners data, data2, data3: data3 anywhere in [-M, M]^3 (shrunk so that the triangle fits), edges of a length log-uniform from 1e-4 M to M."""
    size = log_uniform(rng, 1e-4 * M, 0.5 * M, (n, 1))
    a = rng.uniform(-0.5 * M, 0.5 * M, (n, 3))
    b = unit64(rng.normal(size=(n, 3))) * size * rng.uniform(0.3, 1.0, (n, 1))
    c = unit64(rng.normal(size=(n, 3))) * size * rng.uniform(0.3, 1.0, (n, 1))
    return (a + b).astype(F), (a + c).astype(F), a.astype(F)


def _tri_rows(rng, p1, p2, p3, u, v, n, origin=None, far=None):
    """Rays aimed at the point a + u b + v c of each triangle (a = data3, b = data - a, c = data2 - a) from origins around it."""
    a, b, c = p3.astype(np.float64), p1.astype(np.float64) - p3, p2.astype(np.float64) - p3
    target = a + u[:, None] * b + v[:, None] * c
    reach = np.maximum(np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1))[:, None]
    if origin is None:
        origin = target + unit64(rng.normal(size=(n, 3))) * reach * log_uniform(rng, 0.05, 20.0, (n, 1))
    o = origin.astype(F)
    d = aimed(rng, o, target, n)
    return np.concatenate([p1, p2, p3, o, d], axis=1).astype(F)


def _tri_random(M, seed, n):
    rng = np.random.default_rng(seed)
    p1, p2, p3 = _random_triangles(rng, M, n)
    kind = rng.choice([K["tri"]["inside"], K["tri"]["outside"], K["tri"]["t_near_zero"], K["tri"]["t_near_tmax"]], n, p=(0.5, 0.2, 0.15, 0.15))
    u = rng.uniform(0.02, 0.96, n)
    v = rng.uniform(0.02, 0.98, n) * (1 - u)
    outside = kind == K["tri"]["outside"]
    past = log_uniform(rng, 1e-7, 2.0, n)                                 # how far beyond one of the three edges, in barycentric units
    edge = rng.integers(0, 3, n)
    u = np.where(outside, np.select([edge == 0, edge == 1], [-past, u], u + past * 0.5), u)
    v = np.where(outside, np.select([edge == 0, edge == 1], [v, -past], 1 - u + past * 0.5), v)
    rows = _tri_rows(rng, p1, p2, p3, u, v, n)
    # t on both sides of 0: the origin within a few ulp of the plane, on either side of it, or behind the ray's start
    a, b, c = p3.astype(np.float64), p1.astype(np.float64) - p3, p2.astype(np.float64) - p3
    target = a + u[:, None] * b + v[:, None] * c
    d64 = rows[:, 12:15].astype(np.float64)
    tz = kind == K["tri"]["t_near_zero"]
    t_want = np.where(rng.random(n) < 0.5, 1.0, -1.0) * log_uniform(rng, 1e-9, 1e-3, n)
    rows[:, 9:12] = np.where(tz[:, None], (target - t_want[:, None] * d64).astype(F), rows[:, 9:12])
    # t on both sides of RT_T_MAX: the origin 1e4 direction lengths away, give or take up to a thousandth
    tm = kind == K["tri"]["t_near_tmax"]
    t_want = 1e4 * (1.0 + rng.choice([-1.0, 1.0], n) * log_uniform(rng, 1e-8, 1e-3, n))
    short = unit64(d64) * log_uniform(rng, 0.07, 0.07 * max(1.0, M / 10.0), (n, 1))    # t d stays within reach of float coordinates
    rows[:, 12:15] = np.where(tm[:, None], short.astype(F), rows[:, 12:15])
    rows[:, 9:12] = np.where(tm[:, None], (target - t_want[:, None] * rows[:, 12:15].astype(np.float64)).astype(F), rows[:, 9:12])
    return rows, kind


def _tri_lattice(M, seed, n):
    """Triangles, origins and directions on a lattice, so that a ray through a vertex, along an edge or in the plane is so exactly: p is
    a power of two times b or c (v == 0 or u == 0 to the bit: the solve's products cancel exactly), on the third edge (u + v about 1), or
    d is a combination of b and c (dn == 0)."""
    rng = np.random.default_rng(seed)
    q = lattice(M)
    a = rng.integers(-16, 16, (n, 3)).astype(np.float64)
    b = rng.integers(-8, 9, (n, 3)).astype(np.float64) * 2
    c = rng.integers(-8, 9, (n, 3)).astype(np.float64) * 2
    flat = np.linalg.norm(np.cross(b, c), axis=1) == 0
    c[flat] = np.roll(b[flat], 1, axis=1) + np.array([2.0, 0.0, -2.0])    # keep the triangles proper
    kind = rng.choice([K["tri"][k] for k in ("vertex", "edge_u0", "edge_v0", "edge_uv1", "in_plane")], n, p=(0.2, 0.2, 0.2, 0.25, 0.15))
    half = rng.choice([0.5, 0.25, 0.125], n)
    corner = rng.integers(0, 3, n)
    u = np.select([kind == K["tri"]["vertex"], kind == K["tri"]["edge_u0"], kind == K["tri"]["edge_v0"]], [(corner == 1) * 1.0, 0.0, half], 0.0)
    v = np.select([kind == K["tri"]["vertex"], kind == K["tri"]["edge_u0"], kind == K["tri"]["edge_v0"]], [(corner == 2) * 1.0, half, 0.0], 0.0)
    s = rng.integers(1, 8, n) / 8.0
    uv1 = kind == K["tri"]["edge_uv1"]
    u, v = np.where(uv1, s, u), np.where(uv1, 1.0 - s, v)
    target = a + u[:, None] * b + v[:, None] * c
    step = rng.integers(-6, 7, (n, 3)).astype(np.float64)
    step[(step == 0).all(axis=1)] = (1.0, 2.0, -3.0)
    in_plane = kind == K["tri"]["in_plane"]
    step = np.where(in_plane[:, None], rng.integers(-3, 4, (n, 1)) * b + rng.integers(1, 4, (n, 1)) * c, step)
    back = rng.choice([1.0, 2.0, 4.0, 8.0], n)
    o = target - step * back[:, None]
    o = np.where((in_plane & (rng.random(n) < 0.5))[:, None], o + np.cross(b, c) / 4.0, o)     # in-plane rays beside the plane as well as in it
    d = step * rng.choice([0.125, 0.25, 0.5], (n, 1))
    # the third edge: also a hair inside and outside it, where u + v rounds to either side of 1
    nudge = np.where(uv1 & (rng.random(n) < 0.6), rng.choice([-1.0, 1.0], n) * log_uniform(rng, 1e-8, 1e-6, n), 0.0)
    o = o + nudge[:, None] * (b + c)
    rows = np.concatenate([(a + b) * q, (a + c) * q, a * q, o * q, d], axis=1).astype(F)
    return rows, kind


def _tri_degenerate(M, seed, n):
    rng = np.random.default_rng(seed)
    p1, p2, p3 = _random_triangles(rng, M, n)
    kind = rng.choice([K["tri"]["two_equal"], K["tri"]["collinear"], K["tri"]["zero_area"]], n)
    two = kind == K["tri"]["two_equal"]
    which = rng.integers(0, 3, n)
    p2 = np.where((two & (which == 0))[:, None], p1, p2)
    p3 = np.where((two & (which == 1))[:, None], p1, p3)
    p3 = np.where((two & (which == 2))[:, None], p2, p3)
    col = kind == K["tri"]["collinear"]                                  # data2 on the line data3 - data, as nearly as floats allow: n is rounding noise
    s = rng.uniform(-1.0, 2.0, (n, 1))
    p2 = np.where(col[:, None], (p3.astype(np.float64) + s * (p1.astype(np.float64) - p3)).astype(F), p2)
    zero = kind == K["tri"]["zero_area"]                                 # all three corners equal
    p1, p2 = np.where(zero[:, None], p3, p1), np.where(zero[:, None], p3, p2)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return _tri_rows(rng, p1, p2, p3, u, v, n), kind


def a2_zero_edges(M, rng, n, pick=None):
    """Edge vectors b whose float magic2 . b is exactly 0: k (m1, -m0, 0), k (0, m2, -m1), k (m2, 0, -m0) for the float magic2 = (m0, m1, m2)
    and k a power of two: the two products are the same two floats multiplied in either order, and the third term is 0."""
    m = MAGIC2.astype(np.float64)
    base = np.array([[m[1], -m[0], 0.0], [0.0, m[2], -m[1]], [m[2], 0.0, -m[0]]])
    k = 2.0 ** rng.integers(-6, 2, n) * lattice(M) * 16 * rng.choice([-1.0, 1.0], n)
    if pick is None:
        pick = rng.integers(0, 3, n)
    return base[pick] * k[:, None], pick


def _tri_a2_den(M, seed, n):
    """The `a2 == 0` branch of the solve (b with magic2 . b == 0 exactly, c ordinary) and den == 0 exactly (b and c both so, and not
    parallel: the triangle is a proper one, in a plane that holds the solve's kernel direction as nearly as floats allow).  data3 is the
    origin for most rows, so that data - data3 gives b back exactly; the rest carry a lattice corner (a2 is then only nearly 0)."""
    rng = np.random.default_rng(seed)
    b, pick = a2_zero_edges(M, rng, n)
    assert (float_dot3(MAGIC2, b.astype(F)) == 0).all()
    kind = rng.choice([K["tri"]["a2_zero"], K["tri"]["den_zero"]], n, p=(0.7, 0.3))
    size = np.linalg.norm(b, axis=1, keepdims=True)
    c = unit64(rng.normal(size=(n, 3))) * size * rng.uniform(0.3, 1.5, (n, 1))
    c2, _ = a2_zero_edges(M, rng, n, (pick + 1 + rng.integers(0, 2, n)) % 3)
    c = np.where((kind == K["tri"]["den_zero"])[:, None], c2, c)
    a = np.where(rng.random((n, 1)) < 0.8, 0.0, rng.integers(-16, 16, (n, 3)) * lattice(M))
    p1, p2, p3 = (a + b).astype(F), (a + c).astype(F), a.astype(F)
    u = rng.uniform(-0.2, 1.0, n)
    v = rng.uniform(-0.2, 1.0, n) * (1 - np.clip(u, 0, 1))
    return _tri_rows(rng, p1, p2, p3, u, v, n), kind


def _tri_near_singular(M, seed, n):
    """Triangles whose normal is perpendicular to magic1 x magic2 within |cos| from 2^-24 to 2^-6: the solve's two equations are nearly
    dependent, and the test accepts points of the plane far from the triangle.  Rays at the triangle and at the plane beside it."""
    rng = np.random.default_rng(seed)
    k = kernel_direction()
    cos = log_uniform(rng, 2.0 ** -24, 2.0 ** -6, n) * rng.choice([-1.0, 1.0], n)
    e = unit64(np.cross(k, rng.normal(size=(n, 3))))
    normal = cos[:, None] * k + np.sqrt(1 - cos * cos)[:, None] * e
    t1 = unit64(k - (normal @ k)[:, None] * normal)                       # in the plane, as nearly along k as the plane allows
    t2 = np.cross(normal, t1)
    size = log_uniform(rng, 1e-3 * M, 0.3 * M, (n, 1))
    ang = rng.uniform(0, 2 * np.pi, (n, 2))
    b = size * (np.cos(ang[:, :1]) * t1 + np.sin(ang[:, :1]) * t2)
    c = size * rng.uniform(0.3, 1.0, (n, 1)) * (np.cos(ang[:, 1:]) * t1 + np.sin(ang[:, 1:]) * t2)
    a = rng.uniform(-0.5 * M, 0.5 * M, (n, 3))
    u = rng.uniform(0.05, 0.9, n)
    v = rng.uniform(0.05, 0.95, n) * (1 - u)
    beside = rng.random(n) < 0.5
    u = np.where(beside, u + rng.normal(size=n) * 3.0, u)
    return _tri_rows(rng, (a + b).astype(F), (a + c).astype(F), a.astype(F), u, v, n), np.full(n, K["tri"]["near_singular"])


def _tri():
    rows, kind, scale = [], [], []
    for i, M in enumerate(SCALES):
        for r, k in (_tri_random(M, 8300 + i, 1400), _tri_lattice(M, 8310 + i, 900), _tri_degenerate(M, 8320 + i, 150), _tri_a2_den(M, 8330 + i, 300),
                     _tri_near_singular(M, 8340 + i, 400)):
            rows.append(r); kind.append(k); scale.append(np.full(len(k), M))
    return dict(rows=np.ascontiguousarray(np.concatenate(rows), F), kind=np.concatenate(kind).astype(np.int32), scale=np.concatenate(scale).astype(F))


@functools.lru_cache(maxsize=None)
def families():
    """Built once and shared (read it, do not change it)."""
    out = dict(box=_box(), tri=_tri())
    for fam in out.values():
        for a in fam.values():
            a.setflags(write=False)
    return out


def rows(name):
    return families()[name]["rows"]


FAMILIES = ("box", "tri")


def as_texcoords(u, v):
    """What a figure with corner texcoords (1,0), (0,1), (0,0) reports for (u, v): primitives.cpp:111-114 in float32."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        return (F(0) + u * F(1)) + v * F(0), (F(0) + u * F(0)) + v * F(1)


def evaluate(which):
    """Both families through the CPU oracle (which = "oracle") or the compiled reference ("reference", needs oracle/_ref with the two
    entry points).  Per family an n x 2 (box: flags, bits of t) or n x 4 (tri: flags, bits of t, tu, tv) uint32 array; flags = 1 accepted |
    2 inside, and a rejected row's other words are 0."""
    L, prefix = (C.CDLL(oracle_lib.ref_path("libref_hw8.so")), "ref8_") if which == "reference" else (oracle_lib.lib(), "rto_")
    out = {}
    for family, width in (("box", 1), ("tri", 3)):
        flags, answers = oracle_lib.intersection_test(L, f"{prefix}{family}_test", rows(family), width)
        out[family] = np.concatenate([flags[:, None], bits(answers)], axis=1)
    return out


@functools.lru_cache(maxsize=None)
def oracle_answers():
    out = evaluate("oracle")
    for a in out.values():
        a.setflags(write=False)
    return out


def tri_records(r):
    """a1, b1, a2, b2, den and n of rows' triangles as make_isect forms them (float32): which branches a row can reach."""
    r = np.asarray(r, F)
    a = r[:, 6:9]
    b, c = r[:, 0:3] - a, r[:, 3:6] - a
    with np.errstate(all="ignore"):
        n = np.stack([b[:, 2] * c[:, 1] - b[:, 1] * c[:, 2], b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0], b[:, 1] * c[:, 0] - b[:, 0] * c[:, 1]], axis=1)
        a1, b1, a2, b2 = float_dot3(MAGIC1, b), float_dot3(MAGIC1, c), float_dot3(MAGIC2, b), float_dot3(MAGIC2, c)
        den = b1 * a2 - a1 * b2
    return dict(a1=a1, b1=b1, a2=a2, b2=b2, den=den, n=n)


def reach(gold):
    """What each family claims to reach, counted over the reference's answers and, where a branch is a property of the inputs, over them."""
    fam = families()
    out = {}
    b, g = fam["box"], gold["box"]
    ok, inside, t = (g[:, 0] & 1) != 0, (g[:, 0] & 2) != 0, g[:, 1].view(F)
    kind, axis = b["kind"], b["axis"]
    kb = K["box"]
    on_face = (kind == kb["zero_on_low_face"]) | (kind == kb["zero_on_high_face"])
    out["box_rows"] = int(len(ok))
    out["box_nan_share"] = float(np.isnan(t).mean())
    out["box_accepted"], out["box_rejected"] = int(ok.sum()), int((~ok).sum())
    out["box_inside"], out["box_outside"] = int(inside.sum()), int((ok & ~inside).sum())
    out["box_nan_accepted_per_axis"] = tuple(int((on_face & ok & (axis == k)).sum()) for k in range(3))
    out["box_nan_rejected_per_axis"] = tuple(int((on_face & ~ok & (axis == k)).sum()) for k in range(3))
    out["box_zero_t_entry"] = (int((ok & ~inside & (g[:, 1] == 0)).sum()), int((ok & ~inside & (g[:, 1] == 0x80000000)).sum()))     # t1 == +0, -0
    out["box_zero_t_exit"] = (int((ok & inside & (g[:, 1] == 0)).sum()), int((ok & inside & (g[:, 1] == 0x80000000)).sum()))        # t2 == +0, -0
    out["box_graze_accepted"] = int((ok & (kind == kb["graze"])).sum())
    out["box_behind_rejected"] = int((~ok & (kind == kb["behind"])).sum())
    out["box_kinds"] = {name: (int((ok & (kind == i)).sum()), int((~ok & (kind == i)).sum())) for name, i in kb.items()}
    out["box_scales"] = {float(M): int((b["scale"] == F(M)).sum()) for M in SCALES}
    tr, g = fam["tri"], gold["tri"]
    hit, inside = (g[:, 0] & 1) != 0, (g[:, 0] & 2) != 0
    t, tu, tv = g[:, 1].view(F), g[:, 2].view(F), g[:, 3].view(F)
    kind = tr["kind"]
    kt = K["tri"]
    rec = tri_records(tr["rows"])
    with np.errstate(all="ignore"):
        s = tu + tv
    one_below = np.nextafter(F(1), F(0))
    out["tri_rows"] = int(len(hit))
    out["tri_nan_share"] = float((np.isnan(t) | np.isnan(tu) | np.isnan(tv)).mean())
    out["tri_hit"], out["tri_miss"] = int(hit.sum()), int((~hit).sum())
    out["tri_facing"] = (int((hit & inside).sum()), int((hit & ~inside).sum()))
    out["tri_u_zero"], out["tri_v_zero"] = int((hit & (tu == 0)).sum()), int((hit & (tv == 0)).sum())
    out["tri_uv_one"] = (int((hit & (s == one_below)).sum()), int((hit & (s == 1)).sum()), int((~hit & (kind == kt["edge_uv1"])).sum()))
    out["tri_a2_zero"] = (int((hit & (rec["a2"] == 0)).sum()), int((~hit & (rec["a2"] == 0)).sum()))
    out["tri_a2_nonzero_hits"] = int((hit & (rec["a2"] != 0)).sum())
    out["tri_den_zero"] = int((rec["den"] == 0).sum())
    out["tri_den_zero_proper"] = int(((rec["den"] == 0) & (rec["n"] != 0).any(axis=1)).sum())
    out["tri_normal_zero"] = int((rec["n"] == 0).all(axis=1).sum())
    out["tri_nan_hits"] = int((hit & (np.isnan(tu) | np.isnan(tv))).sum())
    out["tri_kinds"] = {name: (int((hit & (kind == i)).sum()), int((~hit & (kind == i)).sum())) for name, i in kt.items()}
    # the exits that need the ray: dn == 0, t <= 0, t >= RT_T_MAX, counted on the inputs in float32 as the test forms them
    r = tr["rows"]
    with np.errstate(all="ignore"):
        ro = r[:, 9:12] - r[:, 6:9]
        dot = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]
        dn = dot(r[:, 12:15], rec["n"])
        tt = -dot(ro, rec["n"]) / dn
    out["tri_dn"] = (int((dn > 0).sum()), int((dn < 0).sum()), int((dn == 0).sum()))
    out["tri_t_exits"] = dict(nonpositive=int((tt <= 0).sum()), beyond=int((tt >= T_MAX).sum()), nan=int(np.isnan(tt).sum()),
                              near_zero=(int(((tt > 0) & (tt < 1e-3)).sum()), int(((tt <= 0) & (tt > -1e-3)).sum())),
                              near_tmax=(int(((tt < T_MAX) & (tt > 9990)).sum()), int(((tt >= T_MAX) & (tt < 10010)).sum())))
    with np.errstate(all="ignore"):
        cosk = np.abs(unit64(rec["n"].astype(np.float64)) @ kernel_direction())
    ns = kind == kt["near_singular"]
    out["tri_near_singular"] = (int((ns & hit).sum()), int((ns & (cosk < 2.0 ** -16)).sum()), int((ns & (cosk >= 2.0 ** -16)).sum()))
    out["tri_scales"] = {float(M): int((tr["scale"] == F(M)).sum()) for M in SCALES}
    return out


# ---- the gate's soundness cases --------------------------------------------------------------------------------------------------------
def gate_rows(M, n, seed):
    """lo hi o d t gap c2 cull_k per row (gap = 1e30: the test fills it in).  Boxes as the `box` family's; hit points on a face exactly,
    within 1e-9 M to 1e-3 M of one (on either side of it), or anywhere inside; origins anywhere in [-M, M]^3, 30 % of them within 1e-6 M
    to 0.1 M of the hit point; d from the origin to the point, of a length from 0.07 to 15, no component below 1e-30; t the float
    distance over that length moved by -3 .. +3 ulp; c2 = 2^-20 M, cull_k = 2^-7."""
    rng = np.random.default_rng(seed)
    lo, hi = random_boxes(rng, M, n)
    place = rng.choice(3, n, p=(0.35, 0.35, 0.3))                         # on a face, near a face, anywhere inside
    axis = rng.integers(0, 3, n)
    side = rng.choice([-1, 1], n)
    pin = np.zeros((n, 3), int)
    pin[np.arange(n), axis] = np.where(place < 2, side, 0)
    P = _point_in_box(rng, lo, hi, pin)
    near = np.where(place == 1, log_uniform(rng, 1e-9 * M, 1e-3 * M, n) * np.where(rng.random(n) < 0.8, -side, side), 0.0)      # mostly inwards
    P[np.arange(n), axis] += near
    P = P.astype(F)
    o = rng.uniform(-M, M, (n, 3))
    close = rng.random(n) < 0.3
    o = np.where(close[:, None], P + unit64(rng.normal(size=(n, 3))) * log_uniform(rng, 1e-6 * M, 0.1 * M, (n, 1)), o)
    o = np.clip(o, -M, M).astype(F)
    length = log_uniform(rng, 0.07, 15.0, n)
    diff = P.astype(np.float64) - o.astype(np.float64)
    dist = np.maximum(np.linalg.norm(diff, axis=1), 1e-30)
    d = floor_direction((diff / dist[:, None] * length[:, None]).astype(F))
    t = np.maximum((dist / length).astype(F), F(1e-30))
    t = ulp_step(t, rng.integers(-3, 4, n))
    rows = np.concatenate([lo, hi, o, d, t[:, None], np.full((n, 1), 1e30), np.full((n, 1), 2.0 ** -20 * M), np.full((n, 1), 2.0 ** -7)], axis=1)
    return np.ascontiguousarray(rows, F)


GAPS = ("none", 2.0 ** -4, 2.0 ** -10, 2.0 ** -16, 2.0 ** -20)          # the runner-up's distance behind the hit: none (1e30), or t times this


def with_gap(rows, gap):
    out = rows.copy()
    out[:, 13] = F(1e30) if gap == "none" else out[:, 12] * F(gap)
    return out


def grown_boxes(rows, M, seed):
    """Per row the triangle's own box and three copies with each face moved outward by 0 or by a log-uniform amount from 1e-8 M to M,
    clipped to [-M, M]: the boxes above the triangle in some tree.  Returns lo, hi as 4 x n x 3."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    lo, hi = [rows[:, 0:3]], [rows[:, 3:6]]
    for _ in range(3):
        g = np.where(rng.random((2, n, 3)) < 0.35, 0.0, log_uniform(rng, 1e-8 * M, M, (2, n, 3)))
        lo.append(np.maximum((rows[:, 0:3].astype(np.float64) - g[0]).astype(F), F(-M)))
        hi.append(np.minimum((rows[:, 3:6].astype(np.float64) + g[1]).astype(F), F(M)))
    return np.stack(lo), np.stack(hi)

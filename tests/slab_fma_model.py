"""NumPy float32 model of the grid walkers' box test (csrc/device/rt_device.h make_ray_grid / slab_test_q at PT_SLAB_FMA=1, the grid of
csrc/device/rt_node_grid.h), the float64 ray / box test it is held against, and the cases both tests of it run.

Every device operation is one float32 operation here, in the device's order; an FMA is the exact product-sum rounded once to float32.
The one thing the model takes as given is the reciprocal of a direction component (v_rcp_f32, 1 ulp): `rcp=None` uses the correctly
rounded one, the GPU test passes the device's own."""
import numpy as np

F = np.float32
GRID_CELLS, GRID_BORDER = 65000.0, 4        # rt_types.h RT_GRID_CELLS / RT_GRID_BORDER
SCENES = (((-10.0, -3.0, -10.0), (10.0, 5.0, 10.0)),          # a room
          ((100.0, 100.0, -0.001), (100.5, 130.0, 0.001)),    # far from the origin, thin along z
          ((-1e-3, -1e-3, -1e-3), (1e-3, 1e-3, 1e-3)),        # tiny
          ((0.0, 0.0, 0.0), (4000.0, 1.0, 0.0)))              # flat along z, long along x
T_MAX = F(3.0e38)


def node_grid(grid_box):
    """make_node_grid on the float32 box lo.xyz hi.xyz: (lo, step, istep) as float32 triples."""
    b = np.asarray(grid_box, F).astype(np.float64)
    ext = np.maximum(b[3:] - b[:3], 0.0)
    largest = ext.max() if ext.max() > 0 else 1.0
    e = np.where(ext > largest / 64.0, ext, largest / 64.0)
    step = (e / GRID_CELLS).astype(F)
    lo = (b[:3] - GRID_BORDER * step.astype(np.float64)).astype(F)
    return lo, step, (F(1.0) / step).astype(F)


def axis_cells(blo, bhi, glo, step, margin=1.0):
    """grid_axis_word: the cell below / above each bound and `margin` cells further (the device has margin = 1)."""
    a = np.floor((blo.astype(np.float64) - np.float64(glo)) / np.float64(step)) - margin
    b = np.ceil((bhi.astype(np.float64) - np.float64(glo)) / np.float64(step)) + margin
    fits = (a >= 0.0) & (b <= 65535.0) & (a <= b)
    return np.where(fits, a, 0.0), np.where(fits, b, 65535.0), fits


def fma32(a, b, c):
    """float32(a * b + c) with one rounding: the product of a cell (16 bits) and a float32 is exact in float64; the float64 sum is made
    round-to-odd from its exact error term, so that the second rounding, to float32, is the only one that shows."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                     # TwoSum: p + c = s + err exactly
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        toward_zero = fix & ((err > 0) != (s > 0))          # the exact sum lies below |s|: truncate first
        s = np.where(toward_zero, np.nextafter(s, 0.0), s)
        bits = s.view(np.int64).copy()
        bits[fix] |= 1
        return bits.view(np.float64).astype(F)


def clamp_dir(d):
    d = np.asarray(d, F)
    return np.where(np.abs(d) > F(1e-30), d, np.copysign(F(1e-30), d)).astype(F)


def grid_test(cases, grid_box, rcp=None, margin=1.0):
    """cases: n x 13 float32 (lo.xyz hi.xyz o.xyz d.xyz tbest).  Returns (entered, fits, unclamped entry distance) of slab_test_q on
    the grid box of every case."""
    cases = np.asarray(cases, F)
    glo, step, istep = node_grid(grid_box)
    d = clamp_dir(cases[:, 9:12])
    if rcp is None:
        rcp = (F(1.0) / d).astype(F)
    tmin = tmax = None
    fits = np.ones(len(cases), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(3):
            a, b, f = axis_cells(cases[:, k], cases[:, 3 + k], glo[k], step[k], margin)
            fits &= f
            o_g = ((cases[:, 6 + k] - glo[k]).astype(F) * istep[k]).astype(F)
            inv = (step[k] * rcp[:, k].astype(F)).astype(F)
            c = (-o_g * inv).astype(F)
            neg = inv < 0
            t_in = fma32(np.where(neg, b, a).astype(F), inv, c)
            t_out = fma32(np.where(neg, a, b).astype(F), inv, c)
            tmin = t_in if tmin is None else np.fmax(tmin, t_in)      # v_max / v_min pass a NaN operand over
            tmax = t_out if tmax is None else np.fmin(tmax, t_out)
        entered = np.fmax(tmin, F(0)) <= np.fmin(tmax, cases[:, 12])
    return entered, fits, tmin


def real_test(cases):
    """Whether the ray o + t d, 0 <= t <= tbest, meets the float box: float64 on the float32 inputs, a zero component meaning a ray
    that stays in its plane."""
    c = np.asarray(cases, F).astype(np.float64)
    lo, hi, o, d = c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9:12]
    zero = d == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    inside = (lo <= o) & (o <= hi)
    t0 = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    t1 = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    tmin, tmax = np.maximum(t0.max(axis=1), 0.0), np.minimum(t1.min(axis=1), c[:, 12])
    return tmin <= tmax


def make_cases(scene_lo, scene_hi, n, rng):
    """n cases (n x 13 float32) in one scene, and its grid box: where the FMA form is weakest.  Origins at the grid's far corner (the
    largest grid coordinates) and its near one, boxes one cell thick and flat ones, origins on box faces, direction components of
    either sign from the clamp (1e-30, and exact zeros) through 1e-6 to 1, directions of any length."""
    lo_s, hi_s = np.array(scene_lo), np.array(scene_hi)
    grid_box = np.concatenate([lo_s, hi_s]).astype(F)
    _, step, _ = node_grid(grid_box)
    ext = hi_s - lo_s
    c = rng.uniform(lo_s, hi_s, (n, 3))
    half = rng.uniform(0, 1, (n, 3)) ** 4 * 0.25 * ext * rng.choice([0.0, 1.0, 1.0, 1.0], (n, 3))     # some flat boxes
    thin = rng.random((n, 3)) < 0.15
    half = np.where(thin, 0.5 * step.astype(np.float64) * rng.uniform(0.2, 1.0, (n, 3)), half)        # at most one cell thick
    far = rng.random(n) < 0.1                                                                         # boxes at the far corner too
    c[far] = hi_s - rng.uniform(0, 1, (int(far.sum()), 3)) ** 4 * 0.02 * ext
    blo = np.maximum(c - half, lo_s).astype(F)
    bhi = np.maximum(np.minimum(c + half, hi_s).astype(F), blo)
    o = rng.uniform(lo_s, hi_s, (n, 3))
    o[: n // 8] = lo_s
    o[n // 8: n // 2] = hi_s                                                                          # the far corner: o' near 65,000
    o[n // 4: n // 2] -= rng.uniform(0, 1, (n // 2 - n // 4, 3)) ** 2 * 0.01 * ext                    # ... and just inside it
    face = rng.integers(0, 3, n)
    rows = np.arange(n)
    on_face = rng.random(n) < 0.2                                                                     # origins on a face of their box
    side = np.where(rng.random(n) < 0.5, blo[rows, face], bhi[rows, face])
    o[on_face, face[on_face]] = side[on_face]
    target = rng.uniform(blo, bhi)
    d = target - o + rng.normal(0, 1e-3, (n, 3)) * ext
    nz = np.linalg.norm(d, axis=1) > 0
    d[~nz] = (1.0, 0.0, 0.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # small components: the ray (all but) stays in a plane, which passes through the box or lies on one of its faces
    small = rng.random((n, 3)) < 0.25
    small[rows, np.argmax(np.abs(d), axis=1)] &= rng.random(n) < 0.1                                 # seldom all three
    mag = np.where(rng.random((n, 3)) < 0.3, 0.0, 10.0 ** rng.uniform(-30, -6, (n, 3)))
    mag[rng.random((n, 3)) < 0.1] = 1e-30
    d = np.where(small, mag * rng.choice([-1.0, 1.0], (n, 3)), d)
    pick = rng.random((n, 3))
    in_plane = np.where(pick < 0.3, blo, np.where(pick < 0.6, bhi, rng.uniform(blo, bhi)))
    o = np.where(small, in_plane, o)
    d[np.all(d == 0, axis=1)] = (0.0, 1e-30, 0.0)
    d *= 10.0 ** np.where(rng.random(n) < 0.3, rng.uniform(-6, 0, n), 0.0)[:, None]                   # directions need not be unit
    d32 = d.astype(F)
    d32 = np.where((d32 != 0) & (np.abs(d32) < F(1e-30)), np.copysign(F(1e-30), d32), d32)            # below the clamp only as exact zeros
    dn = np.maximum(np.linalg.norm(d32.astype(np.float64), axis=1), 1e-30)
    tbest = np.where(rng.random(n) < 0.5, 3.0e38, np.minimum(rng.uniform(0, 2, n) * np.linalg.norm(ext) / dn, 3.0e38)).astype(F)
    cases = np.concatenate([blo, bhi, o.astype(F), d32, tbest[:, None]], axis=1).astype(F)
    return np.ascontiguousarray(cases), grid_box

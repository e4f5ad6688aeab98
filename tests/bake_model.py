"""The baker (include/rtamd.h: rt_bake_rays, rt_bake) restated for the tests.

What is restated in numpy, float32 with one rounding per operation and no fused operation: p + eps * n, the nine SH polynomials,
the per-stream sums in sample order, the sum over a point's streams, the two scales, and the uniform direction as `normalize` of the
three normals of rto_rng_kat (a record that enters with a saved normal is handled as scatter_model._cosine_with_saved handles it).
Everything else comes from elsewhere: the cosine direction of a fresh engine is the oracle's rto_hw8_cosine_sample_pdf (an engine
state is its own seed), the engine's bookkeeping is scatter_model's, and the paths are scatter_model.trace -- `trace_counted` is that
function with one more result, each path's number of closest-hit queries, which is what the scheduling statistics are made of."""
import ctypes as C

import numpy as np

import scatter_model as model
import surface_model as sm

rt = model.rt
F = np.float32
MISS = model.MISS
EPS = model.EPS
IRRADIANCE, SH9 = 0, 1
FLOATS = {IRRADIANCE: 3, SH9: 27}
NO_RAY = np.array([0, 0, 0, 0x7FC00000, 0x7FC00000, 0x7FC00000], np.uint32)     # rq_store_no_ray


def _lib():
    L = model._lib()
    L.rto_hw8_cosine_sample_pdf.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def point_valid(point, engines, mode):
    """The rule of rt_bake_rays over all of a point's engines."""
    ok = bool(np.isfinite(point["p"]).all())
    if mode == IRRADIANCE:
        ok = ok and bool(np.isfinite(point["n"]).all() and np.abs(point["n"]).max() > 0)
    return ok and all(model.valid_state(x) for x in np.atleast_1d(engines["x"]))


def _direction(e, n, mode):
    """(d, the engine's record afterwards) for one draw of the ray maker from the engine record e."""
    x, saved, has_saved = int(e["x"]), F(e["saved"]), int(e["has_saved"] != 0)
    if has_saved:
        if mode == IRRADIANCE:
            d = model._cosine_with_saved(saved, x, n)
        else:
            p, q = model._normals(x, 2)
            with np.errstate(all="ignore"):
                d = sm.normalize(np.array([saved, p, q], F))
        after = (model._polar_round(x), F(0), 0, e["reserved"])
    else:
        if mode == IRRADIANCE:
            out = np.zeros(5, F)
            _lib().rto_hw8_cosine_sample_pdf(x, np.ascontiguousarray(n, F).ctypes.data, out.ctypes.data)
            d = out[0:3].copy()
        else:
            with np.errstate(all="ignore"):
                d = sm.normalize(model._normals(x, 3))
        after = (model._polar_round(model._polar_round(x)), model._normals(x, 4)[3], 1, e["reserved"])
    return d.astype(F), after


def expected_rays(points, rng, mode):
    """rt_bake_rays: (RAY_DTYPE records, invalid records); rng (RNG_DTYPE) advances in place."""
    rays = np.zeros(len(points), rt.RAY_DTYPE)
    invalid = 0
    for i in range(len(points)):
        if not point_valid(points[i], rng[i], mode):
            rays[i:i + 1].view(np.uint32)[:] = NO_RAY
            invalid += 1
            continue
        n = np.array(points["n"][i], F)
        d, rng[i] = _direction(rng[i], n, mode)
        with np.errstate(all="ignore"):
            rays["o"][i] = points["p"][i] + EPS * n if mode == IRRADIANCE else points["p"][i]
        rays["d"][i] = d
    return rays, invalid


def sh_basis(d):
    """Y_m(d), m = 0..8, for directions (n, 3): (n, 9) float32, the header's polynomials operation by operation."""
    d = np.asarray(d, F)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([np.full(len(d), F(0.282095)), F(0.488603) * y, F(0.488603) * z, F(0.488603) * x, F(1.092548) * (x * y),
                         F(1.092548) * (y * z), F(0.315392) * ((F(3.0) * (z * z)) - F(1.0)), F(1.092548) * (x * z),
                         F(0.546274) * ((x * x) - (y * y))], axis=1).astype(F)


def scale_of(mode, samples):
    return F((4.0 if mode == SH9 else 1.0) * 3.14159265358979323846 / float(samples))


def accumulate(acc, d, L, mode):
    """acc_k += L, or acc_k[m][c] = acc_k[m][c] + (Y_m(d) * L[c]); acc is (slots, 3) or (slots, 9, 3)."""
    with np.errstate(all="ignore"):
        if mode == IRRADIANCE:
            return (acc + L).astype(F)
        return (acc + (sh_basis(d)[:, :, None] * L[:, None, :]).astype(F)).astype(F)


def resolve(acc, valid_point, streams, mode, samples):
    """scale * (((acc_0 + acc_1) + acc_2) ...) per point; zeros for an invalid point."""
    a = acc.reshape((-1, streams) + acc.shape[1:])
    total = a[:, 0].copy()
    with np.errstate(all="ignore"):
        for k in range(1, streams):
            total = (total + a[:, k]).astype(F)
        out = (scale_of(mode, samples) * total).astype(F)
    out[~valid_point] = 0
    return out


def trace_counted(calls, o, d, rng, depth):
    """scatter_model.trace, returning (L, closest-hit queries per path) -- the rounds a path occupies a slot for."""
    n = len(o)
    o, d = np.array(o, F), np.array(d, F)
    tail = np.zeros((n, 3), F)
    E, W = np.zeros((depth, n, 3), F), np.zeros((depth, n, 3), F)
    kept = np.zeros(n, np.int64)
    queries = np.zeros(n, np.int64)
    live = np.arange(n)
    for b in range(depth):
        if not len(live):
            break
        queries[live] += 1
        hits = calls.closest(o[live], d[live])
        miss = hits["triangle"] == MISS
        if miss.any():
            tail[live[miss]] = calls.environment(o[live[miss]], d[live[miss]])
        live, hits = live[~miss], hits[~miss]
        if not len(live):
            break
        surf = calls.surface(hits)
        engines = np.ascontiguousarray(rng[live])
        sc = calls.scatter(o[live], d[live], hits, surf, engines)
        rng[live] = engines
        ended = sc["flags"] != 0
        tail[live[ended]] = surf["emission"][ended]
        live, sc, surf = live[~ended], sc[~ended], surf[~ended]
        E[b, live], W[b, live] = surf["emission"], sc["weight"]
        kept[live] = b + 1
        o[live], d[live] = sc["o"], sc["d"]
    L = tail
    with np.errstate(all="ignore"):
        for b in reversed(range(depth)):
            m = kept > b
            L[m] = E[b, m] + W[b, m] * L[m]
    return L, queries


def bake(calls, points, rng, samples, streams, mode, depth, make_rays=expected_rays, tracer=None):
    """rt_bake as the plain loop: per sample make_rays on every valid slot's engine, the paths, the sums.  rng (n_points * streams
    RNG_DTYPE records) advances in place.  tracer(o, d, rng) -> (L, queries or None) stands in for trace_counted over `calls`.
    Returns (out (n, 3) or (n, 9, 3), closest-hit queries (valid slots, q), whether each point is valid)."""
    K, q = streams, samples // streams
    assert samples == q * K
    n = len(points)
    valid = np.array([point_valid(points[i], rng[i * K:(i + 1) * K], mode) for i in range(n)], bool)
    slots = np.nonzero(np.repeat(valid, K))[0]
    slot_points = np.ascontiguousarray(np.repeat(points, K)[slots])
    acc = np.zeros((n * K, 3) if mode == IRRADIANCE else (n * K, 9, 3), F)
    queries = np.zeros((len(slots), q), np.int64)
    for j in range(q):
        engines = np.ascontiguousarray(rng[slots])
        rays, invalid = make_rays(slot_points, engines, mode)
        assert invalid == 0
        o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
        L, count = tracer(o, d, engines) if tracer else trace_counted(calls, o, d, engines, depth)
        if count is not None:
            queries[:, j] = count
        rng[slots] = engines
        acc[slots] = accumulate(acc[slots], d, L, mode)
    return resolve(acc, valid, K, mode, samples), queries, valid

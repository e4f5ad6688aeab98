"""The bounce step (include/rtamd.h: rt_rng_*, rt_query_scatter, rt_query_bsdf, rt_trace_paths) restated for the tests.

What is restated in numpy, float32 with one rounding per operation and no fused operation: the engine (std::minstd_rand and the
uniform draw on it), x + eps * ng, the component draw, the dot product in device/rt_device.h's order, k in double, the two early
returns and the zeroed fields of an ended record, the sum of the pdf's terms, and rng_n01's saved branch of the cosine sampler (the
oracle's entry points start from a seed, so a record that enters with a saved normal cannot be handed to them whole).  Everything
else is the oracle's own answer: rto_hw8_mix_sample_pdf (direction, pdf, stream position), rto_hw8_brdf, rto_hw8_cosine_pdf,
rto_hw8_vndf_pdf, rto_hw8_light_pdf, rto_rng_kat (the normal draws).

An engine state x in 1 .. 2^31-2 is its own seed (seed mod (2^31-1) == x), which is how a path's engine is carried into the oracle.

`OracleCalls` and `GpuCalls` answer the same five calls (closest, surface, environment, scatter, uniform) from the oracle and this
model, or from a Scene; `trace` and `frame` compose them into Scene::getColor and Scene::getPixel."""
import ctypes as C

import numpy as np

import oracle_lib
import surface_model as sm
import test_gpu_query as tq

rt = oracle_lib.rt
F = np.float32
M = 2147483647
MISS = 0xFFFFFFFF
EPS = F(1e-4)                       # (float)1e-4L
U01_MAX = F(0.99999994)
END_BRDF, END_CLAMP, NO_SURFACE, INVALID = 1, 2, 4, 8


def _lib():
    L = oracle_lib.lib()
    L.rto_hw8_cosine_pdf.argtypes = [C.c_void_p, C.c_void_p]
    L.rto_hw8_cosine_pdf.restype = C.c_float
    L.rto_hw8_vndf_pdf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    L.rto_hw8_vndf_pdf.restype = C.c_float
    L.rto_hw8_trace_pixel.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int]
    return L


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def seed(seeds):
    """minstd_rand::seed on an array: RNG_DTYPE records."""
    s = np.atleast_1d(np.asarray(seeds, np.uint64)) % np.uint64(M)
    rng = np.zeros(s.shape, rt.RNG_DTYPE)
    rng["x"] = np.where(s == 0, 1, s).astype(np.uint32)
    return rng


def next_state(x):
    return (np.asarray(x, np.uint64) * np.uint64(48271) % np.uint64(M)).astype(np.uint32)


def u01_of(x):
    """The uniform draw that leaves the engine in state x: float(x - 1) / 2^31, kept below 1."""
    v = (np.asarray(x, np.uint32) - np.uint32(1)).astype(F) * F(2.0 ** -31)
    return np.where(v >= F(1), U01_MAX, v).astype(F)


def uniform(rng):
    """One draw from every engine of the RNG_DTYPE array, in place."""
    rng["x"] = next_state(rng["x"])
    return u01_of(rng["x"])


def valid_state(x):
    """rq_rng_valid of device/rt_types_query.h."""
    return 1 <= int(x) <= M - 1


def _polar_round(x):
    """The engine state after one round of rng_n01's rejection loop entered in state x."""
    while True:
        x = int(next_state(x)); a = F(2) * u01_of(x) - F(1)
        x = int(next_state(x)); b = F(2) * u01_of(x) - F(1)
        r2 = a * a + b * b
        if not (r2 > F(1) or r2 == F(0)):
            return x


def _normals(x, n):
    """The first n draws of normal_distribution<float> on a fresh distribution and the engine in state x."""
    out = np.zeros(n, F)
    _lib().rto_rng_kat(int(x), 0, n, out.ctypes.data)
    return out


# ---- one record -------------------------------------------------------------------------------------------------------------------
def _nan_bits(a):
    """rq_bits: a NaN leaves with its sign bit set, as the reference's x86 build makes them."""
    w = np.ascontiguousarray(a, F).view(np.uint32).copy()
    w[np.isnan(a)] |= np.uint32(0x80000000)
    return w.view(F)


def _finite_ray(o, d):
    return bool(np.isfinite(o).all() and np.isfinite(d).all() and np.abs(d).max() > 0)


def hit_point(o, d, t, ng):
    """x + eps * ng with x = o + t * d (scene.cpp:104, :151)."""
    with np.errstate(all="ignore"):
        x = np.asarray(o, F) + F(t) * np.asarray(d, F)
        return x + EPS * np.asarray(ng, F)


def kind_of(ray_o, ray_d, hit, surf):
    if hit["triangle"] == MISS or surf["material"] == MISS:
        return NO_SURFACE
    if not _finite_ray(ray_o, ray_d) or not (np.isfinite(hit["t"]) and np.isfinite(hit["ng"]).all()):
        return INVALID
    return 0


def mix_pdf(oracle, xo, sn, d, v, alpha):
    """(cosine pdf + vndf pdf (+ light pdf)) / components, the sum in float32 in Mix::pdf's order (distributions.h:267-279)."""
    L = _lib()
    f3 = lambda a: np.ascontiguousarray(a, F)
    sn, d, v = f3(sn), f3(d), f3(v)
    lights = len(oracle.light_order()) > 0
    with np.errstate(all="ignore"):
        pdf = F(0) + F(L.rto_hw8_cosine_pdf(sn.ctypes.data, d.ctypes.data))
        pdf = pdf + F(L.rto_hw8_vndf_pdf(sn.ctypes.data, d.ctypes.data, v.ctypes.data, float(alpha)))
        if lights:
            pdf = pdf + F(oracle.light_pdf(xo, d))
        return F(pdf / F(3 if lights else 2))


def brdf_of(ray_d, surf, d):
    with np.errstate(all="ignore"):
        view = -np.asarray(ray_d, F)
    return oracle_lib.brdf(_lib(), "rto_hw8_", float(surf["base_metallic"]), surf["base_color"], d, view, surf["sn"], surf["color"],
                           float(surf["metallic"]), float(surf["alpha"]))


def _cosine_with_saved(saved, x1, n):
    """cosine_sample (oracle_common.h:96-104) entered with a saved normal: a = the saved value, b, c = the two values of one polar round."""
    p, q = _normals(x1, 2)
    with np.errstate(all="ignore"):
        d = sm.normalize(np.array([saved, p, q], F)) + n
        l = np.sqrt(sm.dot(d, d))
        if l <= F(1e-9) or sm.dot(d, n) <= F(1e-9) or np.isnan(l):
            return n.copy()
        return ((F(1) / l) * d).astype(F)


def expected_scatter(oracle, o, d, hits, surfaces, rng):
    """The rt_scatter records of the records (o[i], d[i], hits[i], surfaces[i], rng[i]); rng (RNG_DTYPE) advances in place."""
    lights = len(oracle.light_order()) > 0
    comps = 3 if lights else 2
    out = np.zeros(len(hits), rt.SCATTER_DTYPE)
    for i in range(len(hits)):
        h, s, e = hits[i], surfaces[i], rng[i]
        kind = kind_of(o[i], d[i], h, s)
        if not kind and not valid_state(e["x"]):
            kind = INVALID
        if kind:
            out[i]["flags"] = kind
            continue
        xo = hit_point(o[i], d[i], h["t"], h["ng"])
        sn, alpha = np.array(s["sn"], F), F(s["alpha"])
        x1 = int(next_state(e["x"]))
        comp = int(u01_of(x1) * F(comps))
        saved, has_saved = F(e["saved"]), int(e["has_saved"] != 0)
        if comp == 0 and has_saved:
            nd = _cosine_with_saved(saved, x1, sn)
            x_after, saved, has_saved = _polar_round(x1), F(0), 0
            pdf = mix_pdf(oracle, xo, sn, nd, d[i], alpha)
        else:
            ans = oracle.mix_sample_pdf(int(e["x"]), xo, sn, d[i], float(alpha))
            nd, pdf = ans[0:3].copy(), F(ans[3])
            if comp == 0:
                x_after, saved, has_saved = _polar_round(_polar_round(x1)), _normals(x1, 4)[3], 1
            else:
                x_after = x1
                for _ in range(2 if comp == 1 else 3):
                    x_after = int(next_state(x_after))
            assert u01_of(next_state(x_after)) == ans[4], "the model lost the oracle's stream position"
            assert np.array_equal(np.array([pdf]).view(np.uint32), np.array([mix_pdf(oracle, xo, sn, nd, d[i], alpha)]).view(np.uint32)) or np.isnan(pdf)
        rng[i] = (x_after, saved if has_saved else F(0), has_saved, e["reserved"])
        brdf = brdf_of(d[i], s, nd)
        rec = out[i]
        rec["o"], rec["d"], rec["brdf"], rec["component"] = _nan_bits(xo), _nan_bits(nd), _nan_bits(brdf), comp
        if brdf[0] <= EPS and brdf[1] <= EPS and brdf[2] <= EPS:                      # scene.cpp:154-156
            rec["flags"] = END_BRDF
            continue
        rec["pdf"] = _nan_bits(np.array([pdf], F))[0]
        with np.errstate(all="ignore"):
            k = F(np.float64(1.0) / np.float64(pdf) * np.abs(np.float64(sm.dot(nd, sn))))   # :159
            mult = (k * brdf).astype(F)
        if (mult > F(6)).any() or np.isnan(mult).any():                                # :161-163
            rec["flags"] = END_CLAMP
        else:
            rec["weight"] = mult
    return out


def expected_bsdf(oracle, o, d, hits, surfaces, dirs):
    """rt_query_bsdf: (brdf (n, 3), pdf (n,)) of the directions dirs[i]."""
    brdf, pdf = np.zeros((len(hits), 3), F), np.zeros(len(hits), F)
    for i in range(len(hits)):
        h, s = hits[i], surfaces[i]
        xo = hit_point(o[i], d[i], h["t"], h["ng"])
        if kind_of(o[i], d[i], h, s) or not _finite_ray(xo, dirs[i]):
            continue
        brdf[i] = _nan_bits(brdf_of(d[i], s, dirs[i]))
        pdf[i] = _nan_bits(np.array([mix_pdf(oracle, xo, s["sn"], dirs[i], d[i], s["alpha"])], F))[0]
    return brdf, pdf


# ---- the five calls, answered twice -------------------------------------------------------------------------------------------------
class OracleCalls:
    """The public calls answered on the CPU: the oracle's closest hit, tests/surface_model.py's surface, the scene's background
    (scenes without an environment map only) and expected_scatter."""

    def __init__(self, sd, oracle):
        assert sd.environment is None
        self.sd, self.oracle, self.tap = sd, oracle, sm.oracle_tap(sd)

    def closest(self, o, d):
        return tq._expected_hits(self.oracle, self.sd, o, d)

    def surface(self, hits):
        return sm.expected_surfaces(rt, self.sd, hits, self.tap)

    def environment(self, o, d):
        return np.broadcast_to(np.array(self.sd.bg, F), (len(o), 3)).copy()

    def scatter(self, o, d, hits, surfaces, rng):
        return expected_scatter(self.oracle, o, d, hits, surfaces, rng)

    uniform = staticmethod(uniform)


class GpuCalls:
    """The same calls on a Scene."""

    def __init__(self, scene):
        self.scene = scene

    def closest(self, o, d):
        return self.scene.query_closest(o, d)[0]

    def surface(self, hits):
        return self.scene.query_surface(hits)[0]

    def environment(self, o, d):
        return self.scene.query_environment(o, d)[0]

    def scatter(self, o, d, hits, surfaces, rng):
        return self.scene.query_scatter(o, d, hits, surfaces, rng)[0]

    uniform = staticmethod(rt.rng_uniform)


def trace(calls, o, d, rng, depth):
    """Scene::getColor(ray, depth) composed of the calls, for n rays at once: (n, 3) float32; rng advances in place.  The pairs
    (emission, weight) are kept per bounce and folded backwards, two roundings per channel (scene.cpp:164)."""
    n = len(o)
    o, d = np.array(o, F), np.array(d, F)
    tail = np.zeros((n, 3), F)
    E, W = np.zeros((depth, n, 3), F), np.zeros((depth, n, 3), F)
    kept = np.zeros(n, np.int64)
    live = np.arange(n)
    for b in range(depth):
        if not len(live):
            break
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
    return L


def frame(calls, camera_rays, w, h, samples, depth, tracer=None):
    """Scene::getPixel for every pixel of a w x h frame (scene.cpp:166-177): per pixel the engine seeded y * w + x; per sample two
    uniform draws, camera_rays(sample index, xy) -> (o, d), the path, color = color + L; then (float)(1. / samples) * color.
    tracer(o, d, rng) -> (n, 3) stands in for trace(calls, o, d, rng, depth).  Returns (frame (h, w, 3), the engines afterwards)."""
    rng = seed(np.arange(w * h))
    px, py = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    color = np.zeros((h * w, 3), F)
    for s in range(samples):
        xy = np.stack([px.reshape(-1) + calls.uniform(rng), py.reshape(-1) + calls.uniform(rng)], axis=1).astype(F)
        o, d = camera_rays(s, xy)
        with np.errstate(all="ignore"):
            color = color + (tracer(o, d, rng) if tracer else trace(calls, o, d, rng, depth))
    with np.errstate(all="ignore"):
        return (F(1.0 / samples) * color).reshape(h, w, 3), rng


def traced_paths(oracle, w, h, samples, depth):
    """rto_hw8_trace_pixel for every pixel: (camera rays per sample [(o, d)] in frame order, queries per path (h * w, samples),
    whether any query of the frame missed, whether any hit)."""
    L = _lib()
    cap = 12 * samples * depth
    o = np.zeros((samples, h * w, 3), F)
    d = np.zeros((samples, h * w, 3), F)
    lengths = np.zeros((h * w, samples), np.int64)
    any_miss = any_hit = False
    buf = np.zeros(cap, F)
    for y in range(h):
        for x in range(w):
            n = L.rto_hw8_trace_pixel(oracle._h, w, h, samples, depth, x, y, buf.ctypes.data, cap)
            rec = buf[:n].reshape(-1, 12)
            starts = np.nonzero(rec[:, 11] == depth)[0]
            assert len(starts) == samples
            o[:, y * w + x], d[:, y * w + x] = rec[starts, 0:3], rec[starts, 3:6]
            lengths[y * w + x] = np.diff(np.append(starts, len(rec)))
            any_miss |= bool((rec[:, 7] < 0).any())
            any_hit |= bool((rec[:, 7] >= 0).any())
    return o, d, lengths, any_miss, any_hit

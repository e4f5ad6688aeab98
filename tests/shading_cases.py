"""The inputs on which the shading layer of rt_device.h (BRDFs, samplers, tone-mapping) is pinned at its branch points: one table for the
golden generator (golden/make_goldens.py -> pins_shading_edges.npz), the host pin (test_shading_pins.py) and the GPU test
(test_gpu_shading.py).  Everything is deterministic: fixed seeds, float32 arrays.  A family is a dict of arrays with one row per case;
`rows(family)` packs it the way the test hooks take it.

families()   brdf         base_metallic, base_color, l, v, n, color, metallic, alpha          (hw8 MaterialModel::brdf, material.h:42-65)
             brdf_hw7     the same rows; hw7's MaterialModel(alpha, base_metallic, base_color)  (hw7 material.h:42-60)
             vndf         seed, n, v, alpha            Vndf::sample then ::pdf of the sample     (distributions.h:229-245)
             vndf_pdf     n, d, v, alpha               Vndf::pdf                                  (:239-245)
             vndf_local   t1, t2, vT, alpha            Vndf::sample_ behind its two draws (private in the reference: oracle and device only)
             cosine       seed, n                      Cosine::sample then ::pdf of the sample   (:42-57)
             cosine_pdf   n, d                         Cosine::pdf (the reference's harness has no entry for a given d: oracle and device only)
             tonemap      x                            one channel through aces, gamma and the byte (color.cpp:4-31)
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib

F = np.float32
Z = (0.0, 0.0, 1.0)
ALPHAS_BRDF = (0.0064, 0.0016, 0.25, 1.0, 0.0, 1e-20)       # hw8's floor 0.08^2, hw7's 0.04^2, ..., and two no loader produces (0/0 in distributionTerm)
METALS = ((0.0, 0.0), (1.0, 1.0), (1.0, 0.5), (0.3, 1.0), (0.0, 1.0), (1.0, 0.0))     # (base_metallic, metallic)
ALPHAS_VNDF = (0.0064, 0.0016, 0.3, 1.0)
SEEDS = (1, 7, 4242, 12345, 2147483646, 4000000007)
GATE = 0x38D1B717                                             # the float 1e-4: below the double 1e-4 that specularBrdf compares with
DENORM = 1e-45                                                # rounds to the smallest float32 denormal


def unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(F)


def tangent(n):
    """A unit vector perpendicular to n (in double, before rounding)."""
    n = np.asarray(n, np.float64)
    a = np.eye(3)[np.argmin(np.abs(n))]
    t = np.cross(n, a)
    return t / np.linalg.norm(t)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def dot32(a, b):
    """vec3.h:53-55 in float32: x*x + y*y + z*z, left to right."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def half32(l, v):
    """h = (l + v).normalize() in float32 (vec3.h:65-80: one correctly rounded root, one division, three products)."""
    s = np.asarray(l, F) + np.asarray(v, F)
    with np.errstate(all="ignore"):
        return (F(1) / np.sqrt(dot32(s, s)))[..., None] * s


def half_dots(l, v):
    """dot(h, l), dot(h, v) through the oracle's own arithmetic (rto_hw8_half_dots): (k, 2) float32."""
    l, v = np.ascontiguousarray(l, F).reshape(-1, 3), np.ascontiguousarray(v, F).reshape(-1, 3)
    out = np.zeros((l.shape[0], 2), F)
    fn = oracle_lib.lib().rto_hw8_half_dots
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn.restype = None
    fn(l.ctypes.data, v.ctypes.data, out.ctypes.data, l.shape[0])
    return out


def _normals():
    rng = np.random.default_rng(811)
    return [F(Z)] + list(unit(rng.normal(size=(5, 3))))


def _on_gate(n, t, lean, which, target):
    """(l, v) with dot(h, l) (which = 0) or dot(h, v) (1) equal to the float of bit pattern `target` and the other dot clear of the gate (above
    1.05e-4), for a normal n and a tangent t along x and y.  v = lean[0] n - lean[1] t leans against the tangent, so that h has a positive
    component along n and the distribution term is not zero by itself.  l = unit(-v + eps t) brings the dots near 1e-4, but they are
    (l.l + l.v) / |l + v| and (l.v + v.v) / |l + v| with |l + v| of a few 1e-4: one ulp of a component of l moves them by as much as their
    own size, so no bisection on eps converges, and eps is taken from a scan, the values just below the target first.  The dot itself is a
    sum of two products that cancel (a multiple of 2^-25) and a third, h.z * l.z, which is zero so far and is added last (vec3.h:53-55);
    only that one can supply the low bits of the target.  So the z component of l (of v for dot(h, v)) is stepped from 0 up, finely enough
    that its product moves by less than an ulp of the dot per step."""
    n64, t = np.asarray(n, np.float64), np.asarray(t, np.float64)
    kb = 2
    assert np.count_nonzero(n64) == 1 and np.count_nonzero(t) == 1 and n64[2] == 0 and t[2] == 0 and np.dot(n64, t) == 0
    v64 = lean[0] * n64 - lean[1] * t
    v = unit(v64)
    l_of = lambda eps: ((-v64 + eps * t) / np.linalg.norm(-v64 + eps * t)).astype(F)
    value = np.array([target], np.uint32).view(F)[0]
    if which == 0:
        at = lambda ls: half_dots(ls, np.tile(v, (len(ls), 1)))
    else:                                                   # dot(h, v): its last product is h.z * v.z, so the steps go to v.z and l stays
        at = lambda ls: half_dots(ls[:, [0, 1, 3]], ls[:, [4, 5, 2]])[:, ::-1]
    bases = np.stack([l_of(eps) for eps in np.linspace(1.5e-4, 1.2e-3, 4001)])
    if which == 1:                                          # rows l.x l.y z l.z v.x v.y with z the stepped component
        bases = np.concatenate([bases[:, :2], np.zeros((len(bases), 1), F), bases[:, 2:], np.tile(v[:2], (len(bases), 1))], axis=1)
    start = at(bases)                                       # column 0: the dot to place; 1: the other one, which must stay clear of the gate
    below = start[:, 0]
    order = [i for i in np.argsort(-below.astype(np.float64), kind="stable") if below[i] < value and start[i, 1] > 1.1e-4]     # the nearest below the target first
    steps = np.linspace(0.0, 1.2e-5, 200001).astype(F)
    for i in order[:400]:
        cand = np.tile(bases[i], (len(steps), 1))
        cand[:, kb] = steps
        dots = at(cand)
        hit = np.flatnonzero((bits(dots[:, 0]) == target) & (dots[:, 1] > 1.05e-4))
        if hit.size:
            c = cand[hit[0]]
            return (c, v) if which == 0 else (c[[0, 1, 3]], c[[4, 5, 2]])
    raise AssertionError(f"no direction with the half-vector dot on {target:#x}")


def _brdf_geometry():
    """(l, v, n) triples: the listed pairs over every normal, then the gate's threshold family and the signed zeros of v.n and l.n."""
    L, V, N = [], [], []
    add = lambda l, v, n: (L.append(np.asarray(l, F)), V.append(np.asarray(v, F)), N.append(np.asarray(n, F)))
    normals = _normals()
    for n in normals:
        n64 = np.asarray(n, np.float64)
        t = tangent(n64)
        b = np.cross(n64, t)
        v = unit(0.5 * n64 - 0.6 * t + 0.62 * b)
        v64, tf = v.astype(np.float64), t.astype(F)
        add(-v, v, n)                                       # l = -v: h = normalize(0)
        add(v, v, n)
        add(n, n, n)
        add(tf, v, n)                                       # l.n ~ 0
        add(v, tf, n)                                       # v.n ~ 0
        add(tf, -tf, n)
        add(unit(1e-4 * n64 + t), v, n)
        add(unit(-1e-4 * n64 + t), v, n)
        add(unit(2 * np.dot(v64, n64) * n64 - v64), v, n)   # the mirror direction
        add(unit(-v64 + 2e-4 * t), v, n)                    # the 1e-4 gate fires
        add(unit(-v64 + 1e-4 * t), v, n)
        add(-n, v, n)
        add(v, -n, n)
        add(n, unit(t + 1e-7 * n64), n)
    n_listed = len(L)
    X, Y = np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    # leans (v.n, -v.t) at which both searches succeed: whether l.l - v.v can hold the other dot clear of the gate depends on v's rounding
    frames = ((X, Y, (0.8, 0.6)), (X, -Y, (0.28, 0.96)), (-X, Y, (0.5, 0.8660254)), (Y, X, (0.3, 0.953939)), (Y, -X, (0.4, 0.9165)), (-Y, -X, (0.45, 0.893)))
    for n, t, lean in frames:                               # dot(h, l), then dot(h, v), on the float 1e-4 and its two neighbours
        for which in (0, 1):
            for target in (GATE - 1, GATE, GATE + 1):
                l, v = _on_gate(n, t, lean, which, target)
                add(l, v, n)
    n_gate = len(L) - n_listed
    # v.n and l.n exactly +0, -0 and the smallest denormal of either sign, n = (0, 0, 1).  -0 needs every term of the dot to be -0: negative x and y.
    for zv in (0.0, -0.0, DENORM, -DENORM):
        for zl in (0.0, -0.0, DENORM, -DENORM):
            sv = -1.0 if np.signbit(zv) else 1.0
            sl = -1.0 if np.signbit(zl) else 1.0
            add((sl * 0.8, sl * 0.6, zl), (sv * 0.6, sv * 0.8, zv), Z)
    return np.stack(L), np.stack(V), np.stack(N), n_listed, n_gate


def _brdf():
    l, v, n, n_listed, n_gate = _brdf_geometry()
    rows = []
    for g in range(len(l)):
        listed, gate = g < n_listed, n_listed <= g < n_listed + n_gate
        alphas = ALPHAS_BRDF if listed else (0.0064, 0.25)
        metals = METALS if not gate else ((0.0, 0.0), (1.0, 0.5), (0.3, 1.0))       # the gate shows in the dielectric part: l.n < 0 there
        for a in alphas:
            for bm, m in metals:
                rows.append((g, bm, m, a))
    idx = np.array([r[0] for r in rows])
    rng = np.random.default_rng(812)
    k = len(rows)
    return dict(base_metallic=F([r[1] for r in rows]), base_color=rng.uniform(0.1, 1, (k, 3)).astype(F), l=l[idx], v=v[idx], n=n[idx],
                color=rng.uniform(0.1, 1, (k, 3)).astype(F), metallic=F([r[2] for r in rows]), alpha=F([r[3] for r in rows]))


def _vndf_normals():
    rng = np.random.default_rng(813)
    out = list(unit(rng.normal(size=(3, 3))))
    for sign in (1.0, -1.0):
        for _ in range(2):                                  # within 1e-2 of +-z
            out.append(unit(np.array([0, 0, sign]) + 1e-2 * unit(rng.normal(size=3)) * rng.uniform(0.2, 1)))
        out.append(F((0, 0, sign)))
        z = np.array([0.9999], F)                           # vndf_getq compares n.z with +-0.9999 in double: the float 0.9999 and its neighbours
        for zz in (np.nextafter(z, F(0)), z, np.nextafter(z, F(1))):
            out.append(F((np.sqrt(1 - float(zz[0]) ** 2), 0, sign * zz[0])))
    u = unit(rng.normal(size=3)).astype(np.float64)
    out += [(u * (1 + 2.0 ** -20)).astype(F), (u * (1 - 2.0 ** -20)).astype(F)]
    return out


def _vndf():
    rng = np.random.default_rng(814)
    S, N, V, A = [], [], [], []
    for n in _vndf_normals():
        n64 = np.asarray(n, np.float64)
        nu = n64 / np.linalg.norm(n64)
        t = tangent(nu)
        vs = [-n, n, t.astype(F), unit(-1e-4 * nu + t), unit(1e-4 * nu + t), unit(-nu + 1e-4 * t), unit(rng.normal(size=3)),
              unit(-nu + 0.7 * unit(rng.normal(size=3)))]   # v is the incoming ray's direction (the reference's convention): -n is head-on
        for v in vs:
            for a in ALPHAS_VNDF:
                for s in SEEDS:
                    S.append(s); N.append(n); V.append(v); A.append(a)
    return dict(seed=np.array(S, np.uint32), n=np.stack(N).astype(F), v=np.stack(V).astype(F), alpha=F(A))


def _vndf_local():
    rng = np.random.default_rng(815)
    up = lambda x, k=1: (bits(F([x])) + np.uint32(k)).view(F)[0]
    pts = [(1, 0), (-1, 0), (0, 1), (0, -1), (0, 0), (1, 1e-3), (-1, -1e-3)]
    for c in (0.6, 0.28, 0.70710678, 0.96, 1e-3):           # on the circle as nearly as a float t2 allows, and one, two ulp beyond: rem < 0
        c = F(c)
        s = F(np.sqrt(1.0 - float(c) * float(c)))
        pts += [(c, s), (c, up(s)), (c, up(s, 2)), (-c, -up(s)), (up(c), s)]
    vts = [(0, 0, 1), (0, 0, -1), (1, 0, 0.0), (1, 0, -0.0), (0, -1, 0.0), (0.6, 0, 0.8), (0, 0.6, -0.8), tuple(unit(rng.normal(size=3))), (-0.6, 0.48, 0.64), tuple(unit(rng.normal(size=3))), (0, 0, 0)]
    T1, T2, VT, A = [], [], [], []
    for p in pts:
        for vt in vts:
            for a in ALPHAS_VNDF:
                T1.append(p[0]); T2.append(p[1]); VT.append(vt); A.append(a)
    return dict(t1=F(T1), t2=F(T2), vT=F(VT), alpha=F(A))


def _vndf_pdf():
    rng = np.random.default_rng(816)
    N, D, V, A = [], [], [], []
    zs = F([0.9999])
    normals = [F(Z), F((0, 0, -1)), unit(rng.normal(size=3)), F((np.sqrt(1 - float(np.nextafter(zs, F(0))[0]) ** 2), 0, np.nextafter(zs, F(0))[0]))]
    for n in normals:
        n64 = np.asarray(n, np.float64)
        t = tangent(n64)
        r = unit(-n64 + 0.5 * unit(rng.normal(size=3)))
        pairs = [(r, r),                                    # d = -(-v): normalize(0)
                 (t.astype(F), -n), (-t.astype(F), -n),     # d perpendicular to -v, exactly so for n = z
                 (unit(n64 + t), -t.astype(F)),             # vT.z = 0: G1 divides by it
                 (n, -t.astype(F)),
                 (unit(-n64 + 0.3 * t), -n),                # d below the surface
                 (-n, -n), (-n, n),
                 (unit(n64 + 0.5 * t), unit(-n64 + 0.5 * t)),     # the mirror pair: ni = n
                 (unit(rng.normal(size=3)), r)]
        pairs += [(unit(n64 + 0.6 * unit(rng.normal(size=3))), unit(-n64 + 0.6 * unit(rng.normal(size=3)))) for _ in range(40)]     # ordinary pairs, so that numbers carry the comparison
        for d, v in pairs:
            for a in ALPHAS_VNDF:
                N.append(n); D.append(d); V.append(v); A.append(a)
    return dict(n=np.stack(N).astype(F), d=np.stack(D).astype(F), v=np.stack(V).astype(F), alpha=F(A))


def _cosine():
    rng = np.random.default_rng(817)
    normals = np.concatenate([F([Z, (0, 0, -1), (1, 0, 0)]), unit(rng.normal(size=(5, 3)))])
    n = normals[np.arange(2000) % len(normals)]
    seed = np.arange(2000, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)
    u = unit(rng.normal(size=(16, 3))).astype(np.float64)
    nan = np.tile(F([0.3, -0.4, 0.8660254]), (12, 1))
    nan[np.arange(12), np.arange(12) % 3] = np.nan
    extra = [np.zeros((16, 3), F), (1e-10 * u).astype(F),     # n = 0; l <= eps
             nan,
             (1e19 * u).astype(F), (2e19 * u).astype(F)]      # len2 = 1e38 stays finite, 4e38 overflows
    extra = np.concatenate(extra)
    return dict(seed=np.concatenate([seed, np.arange(len(extra), dtype=np.uint32) + np.uint32(900001)]), n=np.concatenate([n, extra]).astype(F))


def _cosine_pdf():
    # d.n = +0, -0 (every term of the dot is -0), negative, a denormal of either sign, positive
    d = [(1, 0, 0.0), (1, 0, -0.0), (-1, -1, -0.0), (0, 0, -1), (0.6, 0, -0.8), (1, 0, DENORM), (1, 0, -DENORM), (0, 0, 1), (0.6, 0, 0.8), (np.nan, 0, 1), (0, 0, np.inf)]
    return dict(n=np.tile(F(Z), (len(d), 1)), d=F(d))


def tonemap_oracle(x):
    """The oracle's byte of every x (one channel each; rto_tonemap takes a colour).  The cases are placed with it and not with a numpy
    model: numpy's pow need not be glibc's, nor the same on every CPU, and a step found one float aside would move the inputs."""
    x = np.asarray(x, F)
    pad = np.concatenate([x, np.zeros((-len(x)) % 3, F)]).reshape(-1, 3)
    return np.stack([oracle_lib.tonemap(oracle_lib.lib(), "rto_tonemap", c) for c in pad]).reshape(-1)[: len(x)].astype(np.int64)


def _tonemap():
    lo = np.zeros(255, np.int64)                              # bit patterns: positive floats order like them
    hi = np.full(255, int(bits(F([8.0]))[0]), np.int64)
    k = np.arange(1, 256)
    assert np.all(tonemap_oracle(lo.astype(np.uint32).view(F)) < k) and np.all(tonemap_oracle(hi.astype(np.uint32).view(F)) >= k)
    while np.any(hi - lo > 1):                                # the smallest x in [0, 8] whose byte is at least k
        mid = (lo + hi) // 2
        up = tonemap_oracle(mid.astype(np.uint32).view(F)) >= k
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    around = (hi[:, None] + np.arange(-8, 41)[None, :]).ravel()
    x = np.unique(around.astype(np.uint32)).view(F)
    special = F([np.nan, np.inf, -np.inf, -0.0, -1e-3, 1e-45, 1e-38, 65504, 1e19, 1e20, 3e38])     # the reference answers 0 for the last two
    x = np.concatenate([x, special])
    return dict(x=np.concatenate([x, F([0.0, 0.5])[: (-len(x)) % 3]]))      # whole triples: the reference's entry takes a colour


@functools.lru_cache(maxsize=None)
def families():
    """Built once and shared (read it, do not change it)."""
    brdf = _brdf()
    out = dict(brdf=brdf, brdf_hw7=brdf, vndf=_vndf(), vndf_pdf=_vndf_pdf(), vndf_local=_vndf_local(), cosine=_cosine(), cosine_pdf=_cosine_pdf(),
               tonemap=_tonemap())
    for fam in out.values():
        for a in fam.values():
            a.setflags(write=False)
    return out


REFERENCE_FAMILIES = ("brdf", "brdf_hw7", "brdf_specular", "vndf", "vndf_pdf", "cosine", "tonemap")     # what pins_shading_edges.npz holds
ORACLE_ONLY_FAMILIES = ("vndf_local", "cosine_pdf")


def rows(name):
    """The family packed for the test hooks: a float32 matrix, one row per case (seeds travel beside it)."""
    f = families()[name]
    col = lambda a: a[:, None] if a.ndim == 1 else a
    order = {"brdf": ("base_metallic", "base_color", "l", "v", "n", "color", "metallic", "alpha"), "vndf": ("n", "v", "alpha"), "vndf_pdf": ("n", "d", "v", "alpha"),
             "vndf_local": ("t1", "t2", "vT", "alpha"), "cosine": ("n",), "cosine_pdf": ("n", "d"), "tonemap": ("x",)}["brdf" if name == "brdf_hw7" else name]
    return np.ascontiguousarray(np.concatenate([col(f[k]) for k in order], axis=1), F)


def _p(a):
    return np.ascontiguousarray(a, F).ctypes.data


def evaluate(which):
    """Every family through the CPU oracle (which = "oracle": all families) or the compiled reference ("reference": REFERENCE_FAMILIES,
    needs oracle/_ref).  brdf_specular is the specular term alone, read through hw7's brdf of a white metal (metallic 1, base colour 1:
    the Fresnel term is 1 and hw7 has no v.n / l.n gates), on the brdf family's geometry and alpha."""
    ref = which == "reference"
    if ref:
        L8, L7 = C.CDLL(oracle_lib.ref_path("libref_hw8.so")), C.CDLL(oracle_lib.ref_path("libref_hw7.so"))
        pre8, pre7, tone = "ref8_", "ref7_", "ref8_tonemap"
    else:
        L8 = L7 = oracle_lib.lib()
        pre8, pre7, tone = "rto_hw8_", "rto_hw7_", "rto_tonemap"
    def fn(lib, name, argtypes, restype=None):
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
        return f
    P, f32 = C.c_void_p, C.c_float
    fam = families()
    out = {}
    b = fam["brdf"]
    k = len(b["alpha"])
    brdf8 = fn(L8, pre8 + "brdf", [f32, P, P, P, P, P, f32, f32, P])
    brdf7 = fn(L7, pre7 + "brdf", [f32, f32, P, P, P, P, P])
    out["brdf"], out["brdf_hw7"], out["brdf_specular"] = np.zeros((k, 3), F), np.zeros((k, 3), F), np.zeros((k, 3), F)
    white = F([1, 1, 1])
    for i in range(k):
        brdf8(b["base_metallic"][i], _p(b["base_color"][i]), _p(b["l"][i]), _p(b["v"][i]), _p(b["n"][i]), _p(b["color"][i]), b["metallic"][i], b["alpha"][i], out["brdf"][i].ctypes.data)
        brdf7(b["alpha"][i], b["base_metallic"][i], _p(b["base_color"][i]), _p(b["l"][i]), _p(b["v"][i]), _p(b["n"][i]), out["brdf_hw7"][i].ctypes.data)
        brdf7(b["alpha"][i], 1.0, _p(white), _p(b["l"][i]), _p(b["v"][i]), _p(b["n"][i]), out["brdf_specular"][i].ctypes.data)
    v = fam["vndf"]
    sample = fn(L8, pre8 + "vndf_sample_pdf", [C.c_uint32, P, P, f32, P])
    out["vndf"] = np.zeros((len(v["alpha"]), 5), F)
    for i in range(len(v["alpha"])):
        sample(int(v["seed"][i]), _p(v["n"][i]), _p(v["v"][i]), v["alpha"][i], out["vndf"][i].ctypes.data)
    v = fam["vndf_pdf"]
    pdf = fn(L8, pre8 + "vndf_pdf", [P, P, P, f32], f32)
    out["vndf_pdf"] = F([pdf(_p(v["n"][i]), _p(v["d"][i]), _p(v["v"][i]), v["alpha"][i]) for i in range(len(v["alpha"]))])
    c = fam["cosine"]
    sample = fn(L8, pre8 + "cosine_sample_pdf", [C.c_uint32, P, P])
    out["cosine"] = np.zeros((len(c["seed"]), 5), F)
    for i in range(len(c["seed"])):
        sample(int(c["seed"][i]), _p(c["n"][i]), out["cosine"][i].ctypes.data)
    x = fam["tonemap"]["x"].reshape(-1, 3)
    fn(L8, tone, [P, P])
    out["tonemap"] = np.stack([oracle_lib.tonemap(L8, tone, x[i]) for i in range(len(x))]).reshape(-1)
    if not ref:
        v = fam["vndf_local"]
        local = fn(L8, "rto_hw8_vndf_sample_local", [f32, f32, P, f32, P])
        out["vndf_local"] = np.zeros((len(v["alpha"]), 3), F)
        for i in range(len(v["alpha"])):
            local(v["t1"][i], v["t2"][i], _p(v["vT"][i]), v["alpha"][i], out["vndf_local"][i].ctypes.data)
        c = fam["cosine_pdf"]
        cpdf = fn(L8, "rto_hw8_cosine_pdf", [P, P], f32)
        out["cosine_pdf"] = F([cpdf(_p(c["n"][i]), _p(c["d"][i])) for i in range(len(c["d"]))])
    return out


@functools.lru_cache(maxsize=None)
def oracle_answers():
    """The oracle's answers on every family, computed once and shared by the tests (read them, do not change them)."""
    out = evaluate("oracle")
    for a in out.values():
        a.setflags(write=False)
    return out


def reach(gold):
    """What each family claims to reach, counted over the reference's answers (and, where a branch is a property of the inputs, over
    the inputs of the cases the reference answers with a number)."""
    fam = families()
    nan_share = {k: float(np.isnan(gold[k].reshape(len(gold[k]), -1)).any(axis=1).mean()) for k in REFERENCE_FAMILIES if gold[k].dtype.kind == "f"}
    b = fam["brdf"]
    finite = np.isfinite(gold["brdf"]).all(axis=1)
    spec = gold["brdf_specular"][:, 0]
    vn, ln = dot32(b["v"], b["n"]), dot32(b["l"], b["n"])
    hn = dot32(half32(b["l"], b["v"]), b["n"])
    hd = half_dots(b["l"], b["v"])
    gate = (hd.astype(np.float64) < 1e-4).any(axis=1)
    nz = fam["vndf"]["n"][:, 2].astype(np.float64)
    answered = ~np.isnan(gold["vndf"]).any(axis=1)
    return dict(nan_share=nan_share,
                brdf_specular_nonzero=int((spec > 0).sum()),
                brdf_gate_zeroed=int((gate & (spec == 0) & (hn > 0)).sum()),
                brdf_gate_exact=int((bits(hd) == GATE).any(axis=1).sum()),
                brdf_vn=(int((finite & (vn >= 0)).sum()), int((finite & (vn < 0)).sum())),
                brdf_ln=(int((finite & (ln >= 0)).sum()), int((finite & (ln < 0)).sum())),
                brdf_vn_zero=int((vn == 0).sum()), brdf_ln_zero=int((ln == 0).sum()),
                vndf_getq=(int((answered & (nz > 0.9999)).sum()), int((answered & (nz < -0.9999)).sum()), int((answered & (np.abs(nz) <= 0.9999)).sum())),
                tonemap_bytes=int(np.unique(gold["tonemap"]).size),
                sizes={k: int(len(gold[k])) for k in REFERENCE_FAMILIES})

"""The surface of a hit (include/rtamd.h, rt_query_surface) restated in numpy: float32 with one rounding per operation, the operations
of the oracle's apply_normal_map and of the alpha / emission products in their order (oracle/oracle_hw8.cpp:337-343,421-431, vector
helpers oracle/oracle_common.h:34-41), so that every word of an rt_surface can be compared.  The texture taps are not restated: a
caller hands in `tap(image, tu, tv, srgb)`, which the tests bind to the oracle's rto_sample_texture.

Vectors are float32 arrays (..., 3)."""
import numpy as np

F = np.float32


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def crossr(a, o):
    """oracle_common.h:36: the reference's cross() is the negated conventional cross product."""
    return np.stack([a[..., 2] * o[..., 1] - a[..., 1] * o[..., 2], a[..., 0] * o[..., 2] - a[..., 2] * o[..., 0],
                     a[..., 1] * o[..., 0] - a[..., 0] * o[..., 1]], axis=-1)


def normalize(a):
    """(float)(1. / (double)len(a)) * a, len = the float of the double square root of the float dot product (oracle_common.h:39-41)."""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        length = np.sqrt(dot(a, a).astype(np.float64)).astype(F)
        k = (np.float64(1.0) / length.astype(np.float64)).astype(F)
        out = k[..., None] * a
    assert out.dtype == F
    return out


def apply_normal_map(sn, tan, tanw, sample):
    """oracle_hw8.cpp:337-343.  sn, tan, sample: (..., 3); tanw: (...)."""
    sn, tan, sample, tanw = np.asarray(sn, F), np.asarray(tan, F), np.asarray(sample, F), np.asarray(tanw, F)
    with np.errstate(all="ignore"):
        lx, lz = tan, sn
        ly = tanw[..., None] * crossr(lx, lz)
        ln = F(2) * sample - F(1)
        n = (ln[..., 0:1] * lx + ln[..., 1:2] * ly) + ln[..., 2:3] * lz
    assert n.dtype == F
    return normalize(n)


def alpha(roughness_factor, mr_y):
    """(float)pow((double)smax(0.08f, roughnessFactor * mr.y), 2.0) (oracle_hw8.cpp:430); smax(a, b) = (a < b) ? b : a."""
    with np.errstate(all="ignore"):
        r = np.asarray(roughness_factor, F) * np.asarray(mr_y, F)
        r = np.where(F(0.08) < r, r, F(0.08)).astype(F)
        return (r.astype(np.float64) ** 2.0).astype(F)


def emission(factor, tap=None):
    """emissiveFactor, times the emissive tap where the material has one (oracle_hw8.cpp:422-423)."""
    e = np.asarray(factor, F)
    return e if tap is None else e * np.asarray(tap, F)


def expected_surfaces(rt, sd, hits, tap):
    """The rt_surface records (rt.SURFACE_DTYPE) of the valid rt_hit records `hits` on the scene data `sd`; a miss gives the blank
    record.  tap(image_index, tu, tv, srgb) -> 3 float32."""
    out = np.zeros(len(hits), rt.SURFACE_DTYPE)
    image_of = lambda t: int(sd.texture_source[t])
    for i, h in enumerate(hits):
        if h["triangle"] == 0xFFFFFFFF:
            out[i]["material"] = 0xFFFFFFFF
            continue
        mi = int(sd.material_index[h["triangle"]])
        m = sd.materials[mi]
        tu, tv = h["texcoord"]
        color = np.ones(3, F) if m.base_color_texture < 0 else tap(image_of(m.base_color_texture), tu, tv, 1)
        em = emission(np.array(m.emission, F), None if m.emissive_texture < 0 else tap(image_of(m.emissive_texture), tu, tv, 1))
        mr = np.ones(3, F) if m.metallic_roughness_texture < 0 else tap(image_of(m.metallic_roughness_texture), tu, tv, 0)
        ns = np.array([0.5, 0.5, 1.0], F) if m.normal_texture < 0 else tap(image_of(m.normal_texture), tu, tv, 0)
        out[i]["color"], out[i]["alpha"] = color, alpha(F(m.roughness_factor), mr[1])
        out[i]["emission"], out[i]["metallic"] = em, mr[2]
        out[i]["sn"], out[i]["material"] = apply_normal_map(h["ns"], h["tangent"][:3], h["tangent"][3], ns), mi
        out[i]["base_color"], out[i]["base_metallic"] = np.array(m.base_color, F), F(m.metallic_factor)
    return out


def oracle_tap(sd):
    """tap() bound to the oracle's sample_texture over sd's images."""
    import oracle_lib
    L = oracle_lib.lib()

    def tap(image, tu, tv, srgb):
        im = sd.images[image]
        out = np.zeros(3, F)
        L.rto_sample_texture(im.shape[1], im.shape[0], im.ctypes.data, float(tu), float(tv), srgb, out.ctypes.data)
        return out
    return tap

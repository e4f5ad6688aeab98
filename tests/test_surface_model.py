"""tests/surface_model.py against the CPU oracle, without a GPU: the emission product and the taps through a one-triangle scene whose
first-hit emission is the pixel of a depth-1 render, and the fixed points of the model's own arithmetic."""
import ctypes as C

import numpy as np

import oracle_lib
import pin_cases
import surface_model as sm

rt = pin_cases.rt
F = np.float32


def _one_triangle(emissive_texture):
    rng = np.random.default_rng(41)
    m = rt.rt_material()
    m.base_color, m.emission, m.metallic_factor, m.roughness_factor = (0.7, 0.6, 0.5), (2.0, 0.5, 1.25), 0.25, 0.6
    m.base_color_texture = m.metallic_roughness_texture = m.normal_texture = -1
    m.emissive_texture = 0 if emissive_texture else -1
    tri = np.array([[-4, -3, 0], [4, -3, 0], [0, 5, 0]], F)
    uv = np.array([[-1.0, -0.75], [1.9, -0.5], [0.4, 1.95]], F)
    nrm = np.tile(F([0, 0, 1]), 3)
    tan = np.tile(F([1, 0, 0, 1]), 3)
    cam = rt.rt_camera()
    cam.position, cam.right, cam.up, cam.forward, cam.fov_y = (0.3, 0.2, 3), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.4
    images = [rng.integers(0, 256, (7, 5, 3)).astype(np.uint8)] if emissive_texture else []
    return rt.SceneData(tri.reshape(1, 9), uv.reshape(1, 6), nrm, tan, np.zeros(1, np.uint32), [m], [0] if emissive_texture else [], images,
                        camera=cam, bg=(0.1, 0.2, 0.3))


def _first_queries(orc, w, h):
    """Per pixel the oracle's first closest-hit query at one sample: (figure index or -1, tu, tv)."""
    L = oracle_lib.lib()
    L.rto_hw8_trace_pixel.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int]
    out = np.zeros((h, w, 3), F)
    buf = np.zeros(12, F)
    for y in range(h):
        for x in range(w):
            assert L.rto_hw8_trace_pixel(orc._h, w, h, 1, 1, x, y, buf.ctypes.data, buf.size) == 12
            out[y, x] = buf[7], buf[9], buf[10]
    return out


def test_emission_product_and_taps_are_the_oracles():
    for textured in (True, False):
        sd = _one_triangle(textured)
        orc = oracle_lib.Hw8Oracle(sd)
        w, h = 16, 12
        rgb, _, _ = orc.render(w, h, 1, ray_depth=1)      # depth 1: the pixel is the first hit's emission, or the background
        q = _first_queries(orc, w, h)
        tap = sm.oracle_tap(sd)
        hit = q[..., 0] >= 0
        assert hit.any() and (~hit).any()
        factor = np.array(sd.materials[0].emission, F)
        for y in range(h):
            for x in range(w):
                want = sm.emission(factor, tap(0, q[y, x, 1], q[y, x, 2], 1) if textured else None) if hit[y, x] else F(sd.bg)
                assert np.array_equal(rgb[y, x], want), (textured, x, y, rgb[y, x], want)
        if textured:
            assert len(np.unique(rgb[hit].reshape(-1, 3), axis=0)) > 20      # the taps vary: the wrap and the weights are met


def test_expected_surfaces_takes_every_field_from_its_source():
    sd = _one_triangle(True)
    hits = np.zeros(3, rt.HIT_DTYPE)
    hits["triangle"] = (0, 0xFFFFFFFF, 0)
    hits["texcoord"] = ((0.3, -0.6), (0, 0), (1.99, 0.01))
    hits["ns"], hits["tangent"] = (0, 0, 1), (1, 0, 0, -1)
    tap = sm.oracle_tap(sd)
    s = sm.expected_surfaces(rt, sd, hits, tap)
    assert s.dtype.itemsize == 64
    assert np.array_equal(s[1:2].view(np.uint32).reshape(16), [0] * 11 + [0xFFFFFFFF] + [0] * 4)
    for i in (0, 2):
        assert np.array_equal(s[i]["color"], F([1, 1, 1])) and s[i]["metallic"] == 1 and s[i]["material"] == 0
        assert np.array_equal(s[i]["emission"], F([2.0, 0.5, 1.25]) * tap(0, *hits[i]["texcoord"], 1))
        assert s[i]["alpha"] == F(F(0.6) * F(0.6)) and np.array_equal(s[i]["sn"], F([0, 0, 1]))
        assert np.array_equal(s[i]["base_color"], F([0.7, 0.6, 0.5])) and s[i]["base_metallic"] == F(0.25)


def test_model_fixed_points():
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (500, 3)).astype(F)
    n = sm.normalize(v)
    assert n.dtype == F and np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1, atol=3e-7)
    one = np.sqrt(sm.dot(v, v).astype(np.float64)).astype(F)
    assert np.array_equal(n, (np.float64(1) / one.astype(np.float64)).astype(F)[:, None] * v)
    # the flat normal-map texel (0.5, 0.5, 1) decodes to (0, 0, 1): the shading normal, normalised once more
    t = sm.normalize(rng.normal(0, 1, (500, 3)).astype(F))
    flat = sm.apply_normal_map(n, t, np.ones(500, F), np.tile(F([0.5, 0.5, 1]), (500, 1)))
    assert np.array_equal(flat, sm.normalize(F(0) * t + F(0) * sm.crossr(t, n) + n))
    # a texel along +x picks the tangent, one along +y the bitangent with the sign of tanw
    assert np.array_equal(sm.apply_normal_map(F([0, 0, 1]), F([1, 0, 0]), F(1), F([1, 0.5, 0.5])), F([1, 0, 0]))
    up = sm.apply_normal_map(F([0, 0, 1]), F([1, 0, 0]), F(1), F([0.5, 1, 0.5]))
    down = sm.apply_normal_map(F([0, 0, 1]), F([1, 0, 0]), F(-1), F([0.5, 1, 0.5]))
    assert np.array_equal(up, sm.crossr(F([1, 0, 0]), F([0, 0, 1]))) and np.array_equal(down, -up)
    # the roughness floor, its edge, and a NaN product (smax keeps its first argument)
    assert sm.alpha(F(0.01), F(1)) == F(F(0.08) * F(0.08)) and sm.alpha(F(0.08), F(1)) == F(F(0.08) * F(0.08))
    assert sm.alpha(F(0.5), F(0.5)) == F(0.0625) and sm.alpha(F(np.nan), F(1)) == F(F(0.08) * F(0.08))
    # a zero vector normalises to the x86 default NaN (0 x inf), sign bit set
    assert np.all(sm.normalize(np.zeros(3, F)).view(np.uint32) == 0xFFC00000)

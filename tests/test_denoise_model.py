"""The preview filter's model (tests/denoise_model.py, the numpy restatement of device/rt_denoise.h) on synthetic planes: what the filter
must never do -- touch a fixed pixel, mix across a normal or a depth edge, move a constant image -- and how its parts compose.  Then
the quality check on the CPU oracle's frames of the sphere scene: the filtered frame of 16 samples is closer to the 1,024-sample frame
than the noisy one.  That holds for the kernels because test_gpu_denoise.py pins them to this model bit for bit."""
import functools

import numpy as np
import pytest

import denoise_model as dm
import noise_model

F = np.float32


def planes(h, w, seed=1, normal=(0, 0, 1), depth=3.0):
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.05, 2.0, (h, w, 3)).astype(F)
    nrm = np.broadcast_to(np.array(normal, F), (h, w, 3)).copy()
    z = np.full((h, w), depth, F)
    return rgb, nrm, z


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_fixed_pixels_come_out_as_their_input_bits():
    h, w = 20, 24
    rgb, nrm, z = planes(h, w)
    alb = np.random.default_rng(2).uniform(0.0, 1.0, (h, w, 3)).astype(F)
    em = np.zeros((h, w, 3), F)
    se = np.full((h, w), 0.1, F)
    z[2:5, 3:9] = 0                      # misses
    em[10:12, 4:7, 1] = 2.5              # emitters
    rgb[15, 15, 2] = np.nan
    nrm[16, 3, 0] = np.inf
    alb[17, 20, 1] = np.nan
    se[18, 1] = np.inf
    z[19, 19] = np.inf
    rgb[2, 3] = (7.0, -0.0, 1e-30)       # any bits pass through
    want = dm.fixed_mask(rgb, nrm, z, alb, em, se)
    assert want.sum() == 18 + 6 + 5
    for kw in (dict(albedo=alb, emission=em, se=se), dict(emission=em), dict()):
        fixed = dm.fixed_mask(rgb, nrm, z, **kw)
        out, out8, n = dm.denoise(rgb, nrm, z, iterations=3, **kw)
        assert n == fixed.sum() and out.dtype == F and out8.dtype == np.uint8
        assert np.array_equal(bits(out)[fixed], bits(rgb)[fixed])
        assert np.array_equal(out8[fixed], dm.tonemap(rgb)[fixed])
        assert np.isfinite(out[~fixed]).all() and not np.array_equal(out[~fixed], rgb[~fixed])


def test_fixed_pixels_are_nobodys_neighbours():
    """A huge value in a fixed pixel leaves every other pixel as it is without that value."""
    h, w = 12, 12
    rgb, nrm, z = planes(h, w)
    em = np.zeros((h, w, 3), F)
    em[6, 6] = 1
    a, _, _ = dm.denoise(rgb, nrm, z, emission=em, iterations=3)
    rgb2 = rgb.copy()
    rgb2[6, 6] = 1e6
    b, _, _ = dm.denoise(rgb2, nrm, z, emission=em, iterations=3)
    others = np.ones((h, w), bool)
    others[6, 6] = False
    assert np.array_equal(bits(a)[others], bits(b)[others]) and b[6, 6, 0] == F(1e6)


@pytest.mark.parametrize("with_se", [False, True])
def test_opposite_normals_never_mix(with_se):
    h, w = 16, 20
    rgb, nrm, z = planes(h, w)
    rgb[:, :10] += 5                      # left: 5.05 .. 7, right: 0.05 .. 2
    nrm[:, 10:] = (0, 0, -1)
    se = np.full((h, w), 0.5, F) if with_se else None
    out, _, _ = dm.denoise(rgb, nrm, z, se=se)
    for side in (np.s_[:, :10], np.s_[:, 10:]):
        assert out[side].min() >= rgb[side].min() and out[side].max() <= rgb[side].max()
    assert out[:, :10].std() < 0.5 * rgb[:, :10].std()   # and each side is smoothed


def test_a_constant_image_stays_constant():
    h, w = 33, 70
    _, nrm, z = planes(h, w)
    z = (z + np.arange(w, dtype=F)[None, :] * F(0.01)).astype(F)   # a depth ramp: the gradient term lets it through
    rgb = np.broadcast_to(np.array([0.3, 1.7, 0.05], F), (h, w, 3)).copy()
    alb = np.random.default_rng(4).uniform(0.2, 1.0, (h, w, 3)).astype(F)
    for kw in (dict(), dict(se=np.full((h, w), 0.05, F)), dict(albedo=np.full((h, w, 3), 0.5, F))):
        out, _, _ = dm.denoise(rgb, nrm, z, iterations=5, **kw)
        assert np.abs(out / rgb - 1).max() <= 1e-6, kw.keys()
    # with a varying albedo the irradiance is what is constant
    out, _, _ = dm.denoise((rgb * alb).astype(F), nrm, z, albedo=alb, iterations=5)
    assert np.abs(out / (rgb * alb) - 1).max() <= 1e-6


def test_a_depth_step_wider_than_the_gradient_allows_does_not_mix():
    h, w = 16, 24
    rgb, nrm, z = planes(h, w)
    rgb[:, :12] += 5
    z[:, 12:] = 6.0                       # flat on both sides: the gradient is zero but in the two columns at the step
    out, _, _ = dm.denoise(rgb, nrm, z)
    inner_l, inner_r = np.s_[:, :11], np.s_[:, 13:]
    assert out[inner_l].min() >= rgb[:, :12].min() and out[inner_r].max() <= rgb[:, 12:].max()
    # one tap across the step: x = 3 / (1e-3 * 3) = 1000 >= 16, the weight is exactly zero
    assert dm.e16(F(3.0) / (dm.EPS_DEPTH_REL * F(3.0) + dm.EPS_DEPTH_ABS)) == 0


def test_without_an_error_map_no_luminance_term_enters():
    """Scaling the picture changes nothing in the weights: each pixel's output is a fixed convex combination of the inputs."""
    h, w = 12, 16
    rgb, nrm, z = planes(h, w)
    a, _, _ = dm.denoise(rgb, nrm, z, iterations=2)
    b, _, _ = dm.denoise((rgb * F(4)).astype(F), nrm, z, iterations=2)
    assert np.array_equal(bits(b), bits((a * F(4)).astype(F)))    # a power of two: exact in every product and sum
    st = dm.pack(rgb, nrm, z)
    assert not st["has_se"] and not st["v"].any()
    # with one, a bright pixel among dark ones is kept out of its neighbours where the map says the picture is quiet
    rgb2 = np.full((h, w, 3), 0.5, F)
    rgb2[6, 8] = 50
    quiet, _, _ = dm.denoise(rgb2, nrm, z, se=np.full((h, w), 1e-3, F), iterations=2)
    blind, _, _ = dm.denoise(rgb2, nrm, z, iterations=2)
    assert np.abs(quiet[6, 9] - 0.5).max() < 1e-3 and blind[6, 9, 0] > 1


@pytest.mark.parametrize("with_se", [False, True])
def test_iterations_k_is_k_applications_of_the_level_function(with_se):
    h, w = 14, 18
    rgb, nrm, z = planes(h, w, seed=9)
    z[3:5, 3:5] = 0
    se = np.random.default_rng(3).uniform(0.01, 0.3, (h, w)).astype(F) if with_se else None
    for k in (1, 2, 4, 8):
        st = dm.pack(rgb, nrm, z, se=se)
        for i in range(k):
            st["irr"], st["v"] = dm.level(st, i)
        want, want8 = dm.finish(st)
        got, got8, _ = dm.denoise(rgb, nrm, z, se=se, iterations=k)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got8, want8)
    assert np.array_equal(bits(dm.denoise(rgb, nrm, z, se=se)[0]), bits(dm.denoise(rgb, nrm, z, se=se, iterations=5, sigma_depth=1, sigma_luminance=4)[0]))


def test_tonemap_is_the_oracles():
    import oracle_lib
    import pin_cases
    x = pin_cases.tonemap_inputs()[:600]
    want = np.stack([oracle_lib.tonemap(oracle_lib.lib(), "rto_tonemap", v) for v in x])
    assert np.array_equal(dm.tonemap(x), want)
    assert np.array_equal(dm.tonemap(np.array([np.nan, np.inf, -1e-3], F)), [0, 0, 0])   # the clamp's max(0, NaN) is 0


# ---- quality on the oracle's frames ------------------------------------------------------------------------------------------------

W, H = 64, 48


@functools.lru_cache(maxsize=None)
def sphere_case():
    """The sphere scene at 64x48 on the CPU: the oracle's frames after 4, 8, 12, 16, 32, 48 and 64 samples, its 1,024-sample frame, and the guide
    planes from its closest hits at the pixel centres and the surface model."""
    import oracle_lib
    import pin_cases
    import surface_model as sm
    import test_gpu_query as tq
    sd = pin_cases.load_sphere()
    oracle = oracle_lib.Hw8Oracle(sd)
    frames = {d: oracle.render(W, H, d)[0] for d in (4, 8, 12, 16, 32, 48, 64, 1024)}
    cam = sd.camera
    xs, ys = np.meshgrid(np.arange(W, dtype=F) + F(0.5), np.arange(H, dtype=F) + F(0.5))
    tan_y = F(np.tan(np.float64(cam.fov_y) / 2))
    tan_x = F(tan_y * F(W) / F(H))
    cx, cy = tan_x * (F(2) * xs.reshape(-1) / F(W) - F(1)), tan_y * (F(2) * ys.reshape(-1) / F(H) - F(1))
    right, up, fwd = (np.array(v, F) for v in (cam.right, cam.up, cam.forward))
    d = cx[:, None] * right - cy[:, None] * up + fwd
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o = np.broadcast_to(np.array(cam.position, F), d.shape).copy()
    hits = tq._expected_hits(oracle, sd, o, d)
    surf = sm.expected_surfaces(pin_cases.rt, sd, hits, sm.oracle_tap(sd))
    hit = hits["triangle"] != tq.MISS
    guides = dict(albedo=np.where(hit[:, None], surf["base_color"] * surf["color"], F(0)).astype(F).reshape(H, W, 3),
                  normal=np.where(hit[:, None], surf["sn"], F(0)).astype(F).reshape(H, W, 3),
                  depth=np.where(hit, hits["t"], F(0)).astype(F).reshape(H, W),
                  emission=np.where(hit[:, None], surf["emission"], F(0)).astype(F).reshape(H, W, 3))
    return frames, guides


def error_map(frames, upto):
    """noise_model.Monitor fed the oracle's frames in four equal cuts up to `upto` samples (sum = frame * d)."""
    cut = upto // 4
    mon = noise_model.Monitor(np.zeros((H, W, 3), F), 0)
    for d in range(cut, upto + 1, cut):
        mon.update((frames[d] * F(d)).astype(F), d)
    return mon.estimate()[0]


def lum_rmse(a, b):
    return float(np.sqrt(np.mean((dm.luminance(a).astype(np.float64) - dm.luminance(b).astype(np.float64)) ** 2)))


def quality_table():
    frames, g = sphere_case()
    ref = frames[1024]
    rows = []
    for d in (16, 64):
        se = error_map(frames, d)
        for use_se in (True, False):
            for use_albedo in (False, True):
                out, _, fixed = dm.denoise(frames[d], g["normal"], g["depth"], albedo=g["albedo"] if use_albedo else None, emission=g["emission"],
                                           se=se if use_se else None)
                rows.append((d, use_se, use_albedo, lum_rmse(frames[d], ref), lum_rmse(out, ref), fixed))
    return rows


def test_the_filtered_frame_is_closer_to_the_converged_one():
    rows = quality_table()
    print("samples  error map  albedo  noisy RMSE  filtered RMSE  ratio  fixed pixels")
    for d, use_se, use_albedo, noisy, filtered, fixed in rows:
        print(f"{d:7d}  {str(use_se):9s}  {str(use_albedo):6s}  {noisy:10.5f}  {filtered:13.5f}  {filtered / noisy:5.3f}  {fixed}")
    d, use_se, use_albedo, noisy, filtered, _ = rows[0]
    assert (d, use_se, use_albedo) == (16, True, False)
    assert filtered < noisy

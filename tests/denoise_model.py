"""The preview filter's arithmetic (include/rtamd.h, rt_denoise) restated in numpy: float32 with one rounding per operation, exactly the
operations of device/rt_denoise.h in their order, so that the filtered floats and their bytes can be compared bit for bit.

Planes are float32 arrays: rgb, normal, albedo, emission (H, W, 3), depth and se (H, W).  A pixel is summed over its taps in the
kernel's order (dy outer, dx inner); here every tap is one shifted array, added in that same order."""
import numpy as np

F = np.float32
DEFAULT_ITERATIONS, DEFAULT_SIGMA_DEPTH, DEFAULT_SIGMA_LUMINANCE = 5, F(1), F(4)
ALBEDO_FLOOR = F(1.0 / 64.0)
EPS_DEPTH_REL, EPS_DEPTH_ABS, EPS_LUMINANCE = F(1e-3), F(1e-12), F(1e-6)
K5 = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))   # the 5-tap B3 spline, by |offset|
K3 = (F(1.0 / 2.0), F(1.0 / 4.0))                  # the 3-tap Gaussian of the variance, by |offset|


def smax(a, b):
    """(a < b) ? b : a, the kernels' max: a NaN in b gives a."""
    return np.where(np.less(a, b), b, a).astype(F)


def smin(a, b):
    """(b < a) ? b : a"""
    return np.where(np.less(b, a), b, a).astype(F)


def luminance(c):
    c = np.asarray(c, F)
    return ((F(0.2126) * c[..., 0]) + (F(0.7152) * c[..., 1])) + (F(0.0722) * c[..., 2])


def e16(x):
    """About exp(-x): max(0, 1 - x / 16) squared four times, zero from x = 16 (and for a NaN)."""
    t = smax(F(0), F(1) - x * F(0.0625))
    for _ in range(4):
        t = t * t
    return t


def tonemap(rgb):
    """The bytes of store_pixel: ACES fit, gamma 1 / 2.2 through double pow, round half away from zero."""
    x = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        q = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        q = smin(F(1), smax(F(0), q))
        g = np.power(q.astype(np.float64), np.float64(F(1.0 / 2.2))).astype(F)
        return np.floor((F(255) * g).astype(np.float64) + 0.5).astype(np.uint8)


def fixed_mask(rgb, normal, depth, albedo=None, emission=None, se=None):
    """Pixels the filter passes through and never reads as neighbours: a miss (depth not > 0), an emitter, a non-finite input."""
    with np.errstate(all="ignore"):
        fixed = ~(np.asarray(depth, F) > 0)
        fixed |= ~np.isfinite(rgb).all(axis=-1) | ~np.isfinite(normal).all(axis=-1) | ~np.isfinite(depth)
        if emission is not None:
            fixed |= (np.asarray(emission, F) != 0).any(axis=-1)
        if albedo is not None:
            fixed |= ~np.isfinite(albedo).all(axis=-1)
        if se is not None:
            fixed |= ~np.isfinite(se)
    return fixed


def _shift(a, oy, ox):
    """a[y + oy, x + ox] with the indices clamped, and where they were inside."""
    h, w = a.shape[:2]
    ys, xs = np.arange(h)[:, None] + oy, np.arange(w)[None, :] + ox
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    return a[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], inside


def pack(rgb, normal, depth, albedo=None, emission=None, se=None):
    """What the pack kernel leaves: fixed, a (H, W, 3), irr (H, W, 3), v (H, W), gx, gy (H, W); a fixed pixel's irr is its rgb as given."""
    rgb, normal, depth = np.asarray(rgb, F), np.asarray(normal, F), np.asarray(depth, F)
    h, w = depth.shape
    fixed = fixed_mask(rgb, normal, depth, albedo, emission, se)
    with np.errstate(all="ignore"):
        a = np.ones((h, w, 3), F) if albedo is None else smax(ALBEDO_FLOOR, np.asarray(albedo, F))
        irr = np.where(fixed[..., None], rgb, rgb / a).astype(F)
        if se is None:
            v = np.zeros((h, w), F)
        else:
            s = np.asarray(se, F) / luminance(a)
            v = np.where(fixed, F(0), s * s).astype(F)
        x, y = np.arange(w), np.arange(h)
        xr, xl = np.minimum(x + 1, w - 1), np.maximum(x - 1, 0)
        yr, yl = np.minimum(y + 1, h - 1), np.maximum(y - 1, 0)
        gx = np.where((xr == xl)[None, :], F(0), (depth[:, xr] - depth[:, xl]) / np.maximum(xr - xl, 1).astype(F)[None, :]).astype(F)
        gy = np.where((yr == yl)[:, None], F(0), (depth[yr, :] - depth[yl, :]) / np.maximum(yr - yl, 1).astype(F)[:, None]).astype(F)
    return dict(fixed=fixed, a=a, normal=normal, depth=depth, irr=irr, v=v, gx=gx, gy=gy, has_se=se is not None)


def level(state, i, sigma_depth=DEFAULT_SIGMA_DEPTH, sigma_luminance=DEFAULT_SIGMA_LUMINANCE):
    """One a-trous level at stride 2^i: (irr', v')."""
    fixed, n, z, irr, v, gx, gy = (state[k] for k in ("fixed", "normal", "depth", "irr", "v", "gx", "gy"))
    step = 1 << i
    sigma_depth, sigma_luminance = F(sigma_depth), F(sigma_luminance)
    with np.errstate(all="ignore"):
        if state["has_se"]:
            num, den = np.zeros_like(v), np.zeros_like(v)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, inside = _shift(v, dy, dx)
                    ok = inside & ~_shift(fixed, dy, dx)[0]
                    g = K3[abs(dy)] * K3[abs(dx)]
                    num = np.where(ok, num + g * vq, num)
                    den = np.where(ok, den + g, den)
            sd = np.sqrt(smax(F(0), num / den))
            yp = luminance(irr)
        acc, accw, accv = np.zeros_like(irr), np.zeros_like(v), np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                nq, inside = _shift(n, oy, ox)
                ok = inside & ~_shift(fixed, oy, ox)[0] & ~fixed
                zq, irrq, vq = _shift(z, oy, ox)[0], _shift(irr, oy, ox)[0], _shift(v, oy, ox)[0]
                hk = K5[abs(dy)] * K5[abs(dx)]
                wn = smax(F(0), ((n[..., 0] * nq[..., 0]) + (n[..., 1] * nq[..., 1])) + (n[..., 2] * nq[..., 2]))
                for _ in range(6):
                    wn = wn * wn
                x = np.abs(z - zq) / (((sigma_depth * np.abs((gx * F(ox)) + (gy * F(oy)))) + (EPS_DEPTH_REL * z)) + EPS_DEPTH_ABS)
                if state["has_se"]:
                    x = x + np.abs(yp - luminance(irrq)) / ((sigma_luminance * sd) + EPS_LUMINANCE)
                wt = ((hk * e16(x)) * wn).astype(F)
                acc = np.where(ok[..., None], acc + wt[..., None] * irrq, acc)
                accw = np.where(ok, accw + wt, accw)
                accv = np.where(ok, accv + (wt * wt) * vq, accv)
        keep = fixed | ~(accw > 0)
        irr2 = np.where(keep[..., None], irr, acc / accw[..., None]).astype(F)
        v2 = np.where(keep, v, accv / (accw * accw)).astype(F)
    assert irr2.dtype == F and v2.dtype == F
    return irr2, v2


def finish(state):
    """(rgb float32, rgb8): the irradiance times the albedo it was divided by; a fixed pixel's floats are its input's."""
    with np.errstate(all="ignore"):
        out = np.where(state["fixed"][..., None], state["irr"], state["irr"] * state["a"]).astype(F)
    return out, tonemap(out)


def denoise(rgb, normal, depth, albedo=None, emission=None, se=None, iterations=0, sigma_depth=0, sigma_luminance=0):
    """rt_denoise: (rgb float32 (H, W, 3), rgb8, fixed_pixels).  0 selects a default, as in rt_denoise_params."""
    iterations = iterations or DEFAULT_ITERATIONS
    sigma_depth = F(sigma_depth) if sigma_depth else DEFAULT_SIGMA_DEPTH
    sigma_luminance = F(sigma_luminance) if sigma_luminance else DEFAULT_SIGMA_LUMINANCE
    state = pack(rgb, normal, depth, albedo, emission, se)
    for i in range(iterations):
        state["irr"], state["v"] = level(state, i, sigma_depth, sigma_luminance)
    out, out8 = finish(state)
    return out, out8, int(state["fixed"].sum())

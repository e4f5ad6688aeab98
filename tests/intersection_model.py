"""Plain numpy float32 restatements of the intersection layer's arithmetic, for the soundness tests of test_gpu_intersection.py.

ref_box      AABB::intersect (primitives.cpp:163-165,29-53) with std::min's and std::max's operand order, pinned to the compiled reference
             by test_intersection_pins.py on the `box` family of intersection_cases.py
gate         pt_deep_inside / pt_box_robust / pt_hit_stands / rq_any_hit_stands of device/rt_exact.h with an IEEE reciprocal where the
             device uses v_rcp_f32 (the two differ only at knife edges), and with c1 and c2 scaled on request: what a lax gate would decide
"""
import numpy as np

F = np.float32
C1 = F(1.9073486328125e-06)        # 2^-19


def smin(a, b):
    """std::min(a, b): (b < a) ? b : a.  A NaN in `a` is returned, a NaN in `b` is dropped."""
    return np.where(b < a, b, a)


def smax(a, b):
    """std::max(a, b): (a < b) ? b : a."""
    return np.where(a < b, b, a)


def ref_box(mn, mx, o, d):
    """(ok, inside, t) of the reference's box test on rows of float32 triples; t is 0 where the box is rejected."""
    mn, mx, o, d = (np.asarray(a, F) for a in (mn, mx, o, d))
    with np.errstate(all="ignore"):
        s = F(0.5) * (mx - mn)
        oc = o - F(0.5) * (mn + mx)
        ts1 = (-s - oc) / d
        ts2 = (s - oc) / d
        lo, hi = smin(ts1, ts2), smax(ts1, ts2)
        t1 = smax(smax(lo[:, 0], lo[:, 1]), lo[:, 2])
        t2 = smin(smin(hi[:, 0], hi[:, 1]), hi[:, 2])
        ok = ~((t1 > t2) | (t2 < 0))
        inside = ok & (t1 < 0)
        t = np.where(inside, t2, t1)
    return ok, inside, np.where(ok, t, F(0)).astype(F)


class BoxesAbove:
    """The reference's answers (ref_box) on the boxes above each row's hit: lo4, hi4 are k x n x 3 (intersection_cases.grown_boxes)."""

    def __init__(self, rows16, lo4, hi4):
        r = np.asarray(rows16, F)
        res = [ref_box(lo, hi, r[:, 6:9], r[:, 9:12]) for lo, hi in zip(lo4, hi4)]
        self.ok, self.inside, self.t_box = (np.stack([x[k] for x in res]) for k in range(3))

    def rejected(self, stands):
        """(a) violated: standing rows with a box the reference rejects.  Row indices."""
        return np.flatnonzero(stands & ~self.ok.all(axis=0))

    def pruned(self, stands, bound, strict=True):
        """(b) violated: standing rows with an accepted box that the reference enters from outside behind `bound` (a float32 per row):
        bound < t_box, the pruning condition of bvh.h:118 for a best hit at `bound`; strict=False: bound <= t_box, for a tmax."""
        behind = (bound[None, :] < self.t_box) if strict else (bound[None, :] <= self.t_box)
        return np.flatnonzero(stands & (self.ok & ~self.inside & behind).any(axis=0))


def _terms(lo, hi, o, d, t, c2, scale):
    c1 = F(C1 * F(scale))
    c2 = (np.asarray(c2, F) * F(scale)).astype(F)[:, None]
    P = o + t[:, None] * d
    m = np.fmin(P - lo, hi - P).min(axis=1)
    dmax = np.abs(d).max(axis=1)
    deep = m - c2[:, 0] >= c1 * t * dmax
    inv = F(1) / np.fmax(np.abs(d), F(1e-30))
    pos = d > 0
    in_ = np.where(pos, P - lo, hi - P)
    out = np.where(pos, hi - P, P - lo)
    a = (in_ - c2) * inv
    b = (out - c2) * inv
    need = c1 * t
    pairs = [a[:, j] + b[:, k] for j in range(3) for k in range(3) if j != k]
    worst = np.minimum.reduce(pairs)          # a NaN propagates: the comparison below is false, as on the device
    exit_ = t + np.fmin(np.fmin(b[:, 0], b[:, 1]), b[:, 2])
    window = need - np.fmin(np.fmin(a[:, 0], a[:, 1]), a[:, 2])
    return deep, worst, exit_, need, window, inv, c2[:, 0]


def hit_stands(rows16, scale=1.0):
    """pt_hit_stands on rows lo hi o d t gap c2 cull_k (what rtt_hit_stands takes; c2x = 1.25 c2 as there)."""
    r = np.asarray(rows16, F)
    lo, hi, o, d, t, gap, c2, cull_k = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12], r[:, 13], r[:, 14], r[:, 15]
    with np.errstate(all="ignore"):
        deep, worst, exit_, need, window, inv, c2s = _terms(lo, hi, o, d, t, c2, scale)
        tie = (gap > 0) & (gap > F(4.8e-7) * (t + gap))
        seen = np.fmax(cull_k * t, (F(1.25) * c2s) * (F(0.9999995) * inv.max(axis=1)))
        full = (worst >= need) & (exit_ >= need) & (gap > window) & tie & (window <= seen)
    return np.where(deep, tie, full)


def box_robust(rows16, scale=1.0):
    """pt_box_robust at P = o + t d (with its pretest: the two forms decide alike except at knife edges)."""
    r = np.asarray(rows16, F)
    with np.errstate(all="ignore"):
        deep, worst, exit_, need, _, _, _ = _terms(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12], r[:, 14], scale)
    return deep | ((worst >= need) & (exit_ >= need))


def any_hit_stands(rows16, scale=1.0):
    """rq_any_hit_stands with the row's gap slot read as tmax."""
    r = np.asarray(rows16, F)
    t, tmax = r[:, 12], r[:, 13]
    with np.errstate(all="ignore"):
        deep, worst, exit_, need, window, _, _ = _terms(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], t, r[:, 14], scale)
        return deep | ((worst >= need) & (exit_ >= need) & (tmax - t > window))

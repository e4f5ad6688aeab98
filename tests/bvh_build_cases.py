"""The inputs on which the on-device tree builder is pinned to its numpy model (bvh_build_model.py): one table for the host test
(test_bvh_build_model.py) and the GPU test (test_gpu_bvh_build.py).  A case is (name, boxes (n, 8) float32, abs_pad, max_depth); the
table is built once and the model's tree of every case is kept beside it."""
import functools

import numpy as np

import bvh_build_model as model
import pin_cases

F = np.float32
THRESHOLD_CASE = "soup_6000"                      # a level of more than 1,024 open nodes, more than 4,096 builder nodes, several binning workgroups


def boxes_of(lo, hi):
    b = np.zeros((len(lo), 8), F)
    b[:, 0:3], b[:, 4:7] = lo, hi
    return b


def soup(n, seed):
    tri = pin_cases.random_triangle_scene(n, seed).positions.reshape(n, 3, 3).astype(F)
    return boxes_of(tri.min(axis=1), tri.max(axis=1))


def random_boxes(rng, n, centre=2.0, size=0.3):
    c = rng.uniform(-centre, centre, (n, 3)).astype(F)
    h = rng.uniform(0.01, size, (n, 3)).astype(F)
    return boxes_of(c - h, c + h)


def coincident(n, lo=(0.25, -1.5, 3.0), hi=(0.75, -1.0, 3.5)):
    return boxes_of(np.tile(F(lo), (n, 1)), np.tile(F(hi), (n, 1)))


def unsplittable(n_group, n_others, seed, abs_pad, max_depth):
    """n_group coincident boxes among random ones, at indices whose hash bit agrees at the depth of the node that holds just them: the
    model says which depth that is (planes do not depend on the indices), and the group then stays one leaf above the depth limit."""
    rng = np.random.default_rng(seed)
    others, group = random_boxes(rng, n_others), coincident(n_group)
    first = model.build(np.concatenate([others, group]), abs_pad, max_depth)
    want = np.arange(n_others, n_others + n_group)
    depth = next(d for d, prims, _ in first["hash_events"] if np.array_equal(prims, want))
    n = n_others + n_group
    at = np.flatnonzero(model.hash_bit(np.arange(n), depth) == 0)[1::2][:n_group]          # spread over the indices, not the first ones
    assert len(at) == n_group
    boxes = np.zeros((n, 8), F)
    boxes[at] = group
    boxes[np.setdiff1d(np.arange(n), at)] = others
    return boxes


def _table():
    rng = np.random.default_rng(2024)
    T = []
    add = lambda name, boxes, abs_pad, max_depth: T.append((name, np.ascontiguousarray(boxes, F), F(abs_pad), max_depth))
    # tiny
    add("one", random_boxes(rng, 1), 0.0, 28)
    add("two_distinct", random_boxes(rng, 2), 1e-4, 28)
    add("two_identical", coincident(2), 0.0, 28)
    # coincident boxes: the edge of BVB_MAX_LEAF, a large group beside others, a group no hash bit divides
    add("coincident_8", coincident(8), 1e-4, 28)
    add("coincident_9", coincident(9), 0.0, 28)
    add("coincident_70_beside_100", np.concatenate([random_boxes(rng, 60), coincident(70), random_boxes(rng, 40)]), 1e-4, 28)
    add("unsplittable_11", unsplittable(11, 100, 5, 0.0, 28), 0.0, 28)
    # soups: around the 32-open-node switch of the LDS paths; past 1,024 open nodes; the depth limit with and without the balance guard
    add("soup_700", soup(700, 7), 1e-4, 28)
    add(THRESHOLD_CASE, soup(6000, 11), 0.0, 28)
    add("cap8_600", soup(600, 3), 0.0, 8)
    add("cap8_2100", soup(2100, 4), 1e-4, 8)
    add("cap8_128", soup(128, 5), 0.0, 8)           # the guard's bound at the root: 4 * 128 is not above 2^6 * 8, 4 * 129 is
    add("cap8_129", soup(129, 5), 1e-4, 8)
    add("cap8_200", soup(200, 6), 0.0, 8)
    # zero-area inputs: the SAH leaf criterion
    x = np.sort(rng.uniform(-3, 3, 61)).astype(F)
    line = lambda a, b: (np.stack([a, np.full(60, F(0.5)), np.full(60, F(-2))], axis=1), np.stack([b, np.full(60, F(0.5)), np.full(60, F(-2))], axis=1))
    add("points_on_a_line", boxes_of(*line(x[:60], x[:60])), 0.0, 28)
    add("segments_on_a_line", boxes_of(*line(x[:60], x[1:])), 1e-4, 28)
    sheet = random_boxes(rng, 300)
    sheet[:, 1] = sheet[:, 5] = F(0.125)
    add("sheet_300", sheet, 0.0, 28)
    # offsets and signed zero
    moved = soup(700, 7)
    moved[:, 0:3] += F([900, -400, 250]); moved[:, 4:7] += F([900, -400, 250])
    add("soup_700_moved", moved, 1e-4, 28)
    z = soup(300, 9)
    z[0:12, 0], z[12:24, 4], z[24:36, 1], z[36:48, 5] = F(-0.0), F(0.0), F(0.0), F(-0.0)     # bounds that are exactly -0.0 / +0.0 where the box straddles
    z[0:12, 4], z[12:24, 0], z[24:36, 5], z[36:48, 1] = np.abs(z[0:12, 4]), -np.abs(z[12:24, 0]), np.abs(z[24:36, 5]), -np.abs(z[36:48, 1])
    z[48:54, 2], z[48:54, 6] = F(-0.0), F(-0.0)                                               # flat in z at -0.0 and at +0.0: centroids -0.0 and +0.0
    z[54:60, 2], z[54:60, 6] = F(0.0), F(0.0)
    z[60:64, 2], z[60:64, 6] = F(0.0), F(-0.0)                                                # lo = +0.0, hi = -0.0: equal as values
    add("soup_300_signed_zero", z, 0.0, 28)
    # costs beyond the sweeps' 3.0e38 start value: no plane is ever chosen, the hash split takes over
    c = rng.uniform(-1e19, 1e19, (40, 3)).astype(F)
    h = rng.uniform(1e18, 2e18, (40, 3)).astype(F)
    add("overflow_40", boxes_of(c - h, c + h), 1e-4, 28)
    h[:, 1] = 0
    c[:, 1] = F(3e18)
    add("overflow_flat_40", boxes_of(c - h, c + h), 0.0, 28)
    c = rng.uniform(-1.4e38, 1.4e38, (40, 3)).astype(F)                                       # doubled centroids and extents are infinite: inf * 0 and inf - inf
    h = rng.uniform(1e36, 2e36, (40, 3)).astype(F)
    h[:, 1] = 0
    c[:, 1] = F(1.0)
    add("overflow_flat_inf_40", boxes_of(c - h, c + h), 0.0, 28)
    # centroid extents of about 1e-41 on x: 16 / e is infinite.  Once with y and z to split on, once with x alone
    d = random_boxes(rng, 200)
    t = (rng.permutation(200) * 7 + 3).astype(np.uint32)                                      # denormal bit patterns: 4e-45 .. 2e-42
    d[:, 0], d[:, 4] = t.view(F), (t + np.uint32(5000)).view(F)
    add("denormal_x_200", d, 0.0, 28)
    d = random_boxes(rng, 48)
    d[:, 0:3], d[:, 4:7] = -np.abs(d[:, 4:7]), np.abs(d[:, 4:7])                              # concentric: every centroid is 0 on y and z
    t = (np.arange(48, dtype=np.uint32) % 6) * np.uint32(1200) + np.uint32(10)
    d[:, 0], d[:, 4] = t.view(F), t.view(F)
    add("denormal_x_alone_48", d, 1e-4, 28)
    return T


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_table())


NAMES = ("one", "two_distinct", "two_identical", "coincident_8", "coincident_9", "coincident_70_beside_100", "unsplittable_11", "soup_700",
         THRESHOLD_CASE, "cap8_600", "cap8_2100", "cap8_128", "cap8_129", "cap8_200", "points_on_a_line", "segments_on_a_line", "sheet_300", "soup_700_moved",
         "soup_300_signed_zero", "overflow_40", "overflow_flat_40", "overflow_flat_inf_40", "denormal_x_200", "denormal_x_alone_48")


def case(name):
    return next(c for c in table() if c[0] == name)


@functools.lru_cache(maxsize=None)
def model_tree(name):
    """The model's tree of a case, built once and shared by the tests (read it, do not change it)."""
    _, boxes, abs_pad, max_depth = case(name)
    return model.build(boxes, abs_pad, max_depth)

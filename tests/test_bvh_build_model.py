"""The numpy model of the on-device tree builder (bvh_build_model.py) and the table of cases it is compared on (bvh_build_cases.py), without a
GPU: the model's trees are valid by a check that does not use the model, the table reaches every branch and threshold of the builder,
the check can fail, and the model's trees survive the walkers' fold (csrc/host/fold_nodes.h through the test hooks) with their leaves."""
import ctypes as C
import os

import numpy as np
import pytest

import bvh_build_cases as cases
import bvh_build_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF, EMPTY = model.LEAF, model.EMPTY


def checked(name, nodes=None, order=None, last=None, depth=None):
    _, boxes, abs_pad, max_depth = cases.case(name)
    m = cases.model_tree(name)
    return model.check_tree(boxes, abs_pad, max_depth, m["nodes"] if nodes is None else nodes, m["order"] if order is None else order,
                            m["last"] if last is None else last, m["depth"] if depth is None else depth)


def test_the_table_is_what_its_names_say():
    assert tuple(c[0] for c in cases.table()) == cases.NAMES
    pads = {float(c[2]) for c in cases.table()}
    assert pads == {0.0, float(np.float32(1e-4))}
    for name, boxes, _, max_depth in cases.table():
        lo, hi = model.split_boxes(boxes)
        assert np.isfinite(boxes).all() and (lo <= hi).all() and 8 <= max_depth <= model.MAX_DEPTH, name


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_tree_is_valid(name):
    m = cases.model_tree(name)
    assert checked(name)
    assert m["nodes"].shape == (m["n_nodes"], 16) and m["nodes"].dtype == np.uint32
    print(f"{name}: {len(cases.case(name)[1])} boxes, {m['n_nodes']} nodes, depth {m['depth']}, open per level {m['open_per_level']}, {m['tally']}")


def test_the_table_reaches_every_branch():
    total = dict.fromkeys(model.TALLY, 0)
    for name in cases.NAMES:
        for k, v in cases.model_tree(name)["tally"].items():
            total[k] += v
    print(total)
    assert all(total[k] > 0 for k in model.TALLY), total
    tally = lambda name: cases.model_tree(name)["tally"]
    assert tally("points_on_a_line")["leaf_by_sah"] > 0 and tally("segments_on_a_line")["leaf_by_sah"] > 0
    assert tally("coincident_9")["hash_split"] == 1 and tally("coincident_70_beside_100")["hash_split"] > 1
    assert tally("cap8_600")["closed_by_depth"] > 0 and tally("cap8_2100")["closed_by_depth"] == 256 and tally("cap8_2100")["guard_overrode"] > 0
    assert tally("unsplittable_11")["unsplit_hash_half_empty"] == 1
    for name in ("overflow_40", "overflow_flat_40", "overflow_flat_inf_40"):      # no plane at the root: every cost is beyond 3.0e38
        depth, prims, was_split = cases.model_tree(name)["hash_events"][0]
        assert depth == 0 and len(prims) == 40 and was_split, name


def test_the_table_reaches_every_threshold():
    _, boxes, _, _ = cases.case(cases.THRESHOLD_CASE)
    m = cases.model_tree(cases.THRESHOLD_CASE)
    assert max(m["open_per_level"]) >= model.THREADS + 1          # bvb_number_kernel carries its sums into a second step
    assert m["n_builder_nodes"] > 4 * model.THREADS               # and so does bvb_layout_kernel
    assert len(boxes) > model.THREADS                             # several binning workgroups
    levels = cases.model_tree("soup_700")["open_per_level"]       # both sides of the switch between LDS and global bins / centroid keys
    assert model.LDS_NODES in levels and model.LDS_NODES + 1 <= max(levels) and min(levels) < model.LDS_NODES
    # one-primitive leaves on a soup (its exact duplicates apart), leaves above 8 only where the table means them
    sizes = lambda name: np.diff(np.concatenate([[-1], np.flatnonzero(cases.model_tree(name)["last"])]))
    assert sizes("soup_700").max() <= 2 and (sizes("soup_700") == 2).sum() <= 20
    assert sizes("cap8_2100").max() > model.MAX_LEAF and cases.model_tree("cap8_2100")["depth"] == 8
    assert sizes("unsplittable_11").max() == 11 and sizes("coincident_8").tolist() == [8] and sizes("coincident_9").max() <= 8
    assert sizes("two_identical").tolist() == [2] and sizes("two_distinct").tolist() == [1, 1] and sizes("one").tolist() == [1]
    # the centroid extents the names promise
    for name in ("denormal_x_200", "denormal_x_alone_48"):
        lo, hi = model.split_boxes(cases.case(name)[1])
        e = (lo[:, 0] + hi[:, 0]).max() - (lo[:, 0] + hi[:, 0]).min()
        with np.errstate(all="ignore"):
            assert 0 < e < 1.2e-38 and np.isinf(np.float32(16) / np.float32(e)), name
    lo, hi = model.split_boxes(cases.case("soup_300_signed_zero")[1])
    bits = np.concatenate([lo.view(np.uint32).ravel(), hi.view(np.uint32).ravel()])
    assert (bits == 0).sum() >= 24 and (bits == 0x80000000).sum() >= 24


def _damage(name, what):
    m = cases.model_tree(name)
    nodes, order, last = m["nodes"].copy(), m["order"].copy(), m["last"].copy()
    leaf_ends = np.flatnonzero(last)
    if what == "lo shrunk by an ulp":
        i = len(nodes) // 2
        f = nodes[i, 0:1].view(np.float32)
        nodes[i, 0] = np.nextafter(f, np.float32(np.inf)).view(np.uint32)[0]
    elif what == "lo grown by an ulp":                          # still contains its primitives: only the equality sees it
        i = len(nodes) // 3
        f = nodes[i, 9:10].view(np.float32)
        nodes[i, 9] = np.nextafter(f, np.float32(-np.inf)).view(np.uint32)[0]
    elif what == "hi shrunk by an ulp":
        i = len(nodes) - 1
        f = nodes[i, 14:15].view(np.float32)
        nodes[i, 14] = np.nextafter(f, np.float32(-np.inf)).view(np.uint32)[0]
    elif what == "order swapped across leaves":
        a, b = leaf_ends[3], leaf_ends[-3]
        order[a], order[b] = order[b], order[a]
    elif what == "order swapped inside a leaf":
        sizes = np.diff(np.concatenate([[-1], leaf_ends]))
        e = leaf_ends[np.flatnonzero(sizes >= 2)[0]]
        order[e - 1], order[e] = order[e], order[e - 1]
    elif what == "last mark moved":
        e = leaf_ends[np.flatnonzero(np.diff(np.concatenate([[-1], leaf_ends])) >= 2)[0]]
        last[e], last[e - 1] = 0, 1
    elif what == "child index duplicated":
        inner = [(i, o) for i in range(len(nodes)) for o in (3, 11) if not nodes[i, o] & LEAF]
        (i0, o0), (i1, o1) = inner[-1], inner[-2]
        nodes[i0, o0] = nodes[i1, o1]
    return nodes, order, last


@pytest.mark.parametrize("name", ["coincident_70_beside_100", "soup_700", "cap8_2100"])
@pytest.mark.parametrize("what", ["lo shrunk by an ulp", "lo grown by an ulp", "hi shrunk by an ulp", "order swapped across leaves", "order swapped inside a leaf",
                                  "last mark moved", "child index duplicated"])
def test_check_tree_rejects_a_damaged_tree(name, what):
    nodes, order, last = _damage(name, what)
    m = cases.model_tree(name)
    assert not (np.array_equal(nodes, m["nodes"]) and np.array_equal(order, m["order"]) and np.array_equal(last, m["last"]))
    with pytest.raises(AssertionError) as e:
        checked(name, nodes=nodes, order=order, last=last)
    print(f"{name}, {what}: {str(e.value)[:200]}")


def test_check_tree_rejects_a_wrong_depth():
    with pytest.raises(AssertionError):
        checked("soup_700", depth=cases.model_tree("soup_700")["depth"] + 1)
    _, boxes, abs_pad, _ = cases.case("cap8_600")
    m = cases.model_tree("cap8_600")
    with pytest.raises(AssertionError):
        model.check_tree(boxes, abs_pad, 7, m["nodes"], m["order"], m["last"], m["depth"])


@pytest.fixture(scope="module")
def hooks():
    path = os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so")
    if not os.path.exists(path):
        pytest.skip("test hooks not built")
    L = C.CDLL(path)
    L.rtt_fold_nodes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.rtt_fold_nodes.restype = C.c_int
    return L


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_tree_folds_with_its_leaves(hooks, name):
    """The walkers' fold keeps the leaf records of the model's tree, each exactly once."""
    words = np.ascontiguousarray(cases.model_tree(name)["nodes"])
    fl = words.view(np.float32)
    boxes = [(fl[0, 0:3], fl[0, 4:7])] + ([(fl[0, 8:11], fl[0, 12:15])] if int(words[0, 11]) != EMPTY else [])
    grid_box = np.concatenate([np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)]).astype(np.float32)
    out = np.zeros((len(words) + 2, 16), np.uint32)
    depth, grid = C.c_uint32(0), np.zeros(9, np.float32)
    n = hooks.rtt_fold_nodes(words.ctypes.data, len(words), grid_box.ctypes.data, out.ctypes.data, len(out), C.byref(depth), grid.ctypes.data)
    assert n >= 1
    seen, todo = [], [0]
    while todo:
        w = todo.pop()
        for k in range(4):
            c = int(out[w, 4 * k + 3])
            if c == EMPTY:
                continue
            if c & LEAF:
                seen.append(c)
            else:
                assert 0 < c < n
                todo.append(c)
    leaves = [int(words[i, o]) for i in range(len(words)) for o in (3, 11) if int(words[i, o]) != EMPTY and int(words[i, o]) & LEAF]
    assert sorted(seen) == sorted(leaves)
    assert depth.value <= (cases.model_tree(name)["depth"] + 1) // 2 + 1

"""The on-device tree builder (csrc/device/rt_bvh_build.h through build_tree_on_device, the function scene creation calls) read back through
the test hooks and compared on the cases of bvh_build_cases.py: first against the invariants of a valid tree (bvh_build_model.check_tree,
which does not use the model), then bit for bit against the numpy model: every node word, the leaf order, the leaf marks, the node count
and the depth.  gather_records, which brings a scene's records into the leaf order, against records[order]."""
import ctypes as C
import os

import numpy as np
import pytest

import bvh_build_cases as cases
import bvh_build_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_build_tree.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtt_build_tree.restype = C.c_int
    L.rtt_gather_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.rtt_gather_records.restype = C.c_int
    return L


def build_on_device(hooks, boxes, abs_pad, max_depth, node_cap=None, n=None):
    n = len(boxes) if n is None else n
    node_cap = len(boxes) + 1 if node_cap is None else node_cap
    nodes = np.zeros((len(boxes) + 1, 16), np.uint32)
    order, last, depth = np.zeros(len(boxes), np.uint32), np.zeros(len(boxes), np.uint8), C.c_uint32(0)
    rc = hooks.rtt_build_tree(boxes.ctypes.data, n, float(abs_pad), max_depth, nodes.ctypes.data, node_cap, order.ctypes.data, last.ctypes.data, C.byref(depth))
    return rc, nodes[:max(rc, 0)], order, last, depth.value


_built = {}


def device_tree(hooks, name):
    """The device's tree of a case, built once for the tests that read it."""
    if name not in _built:
        _, boxes, abs_pad, max_depth = cases.case(name)
        _built[name] = build_on_device(hooks, boxes, abs_pad, max_depth)
    return _built[name]


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_tree_is_valid(hooks, name):
    _, boxes, abs_pad, max_depth = cases.case(name)
    rc, nodes, order, last, depth = device_tree(hooks, name)
    assert rc >= 1
    assert model.check_tree(boxes, abs_pad, max_depth, nodes, order, last, depth)


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_tree_equals_the_model(hooks, name):
    m = cases.model_tree(name)
    rc, nodes, order, last, depth = device_tree(hooks, name)
    print(f"{name}: device {rc} nodes, depth {depth}; model {m['n_nodes']} nodes, depth {m['depth']}, open per level {m['open_per_level']}")
    assert rc == m["n_nodes"] and depth == m["depth"]
    bad = np.argwhere(nodes != m["nodes"])
    for i, w in bad[:8]:
        print(f"  node {i} word {w}: device {int(nodes[i, w]):08x} model {int(m['nodes'][i, w]):08x}")
    assert len(bad) == 0, f"{len(bad)} node words differ, the first in node {bad[0][0]}"
    assert np.array_equal(order, m["order"]), f"order differs first at slot {np.flatnonzero(order != m['order'])[:1]}"
    assert np.array_equal(last, m["last"]), f"last differs first at slot {np.flatnonzero(last != m['last'])[:1]}"


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_second_build_returns_the_same_bytes(hooks, name):
    _, boxes, abs_pad, max_depth = cases.case(name)
    first = device_tree(hooks, name)
    again = build_on_device(hooks, boxes, abs_pad, max_depth)
    assert again[0] == first[0] and again[4] == first[4]
    assert again[1].tobytes() == first[1].tobytes() and again[2].tobytes() == first[2].tobytes() and again[3].tobytes() == first[3].tobytes()


def test_refusals_are_negative_codes(hooks):
    _, boxes, abs_pad, _ = cases.case("coincident_70_beside_100")
    assert build_on_device(hooks, boxes, abs_pad, 28, n=0)[0] < 0
    assert build_on_device(hooks, boxes, abs_pad, 7)[0] < 0
    assert build_on_device(hooks, boxes, abs_pad, 29)[0] < 0
    n_nodes = cases.model_tree("coincident_70_beside_100")["n_nodes"]
    assert build_on_device(hooks, boxes, abs_pad, 28, node_cap=n_nodes - 1)[0] < 0
    assert build_on_device(hooks, boxes, abs_pad, 28, node_cap=n_nodes)[0] == n_nodes      # and the library builds on after refusing
    assert build_on_device(hooks, boxes, abs_pad, 8)[0] >= 1


@pytest.mark.parametrize("or_into_word", [0, 1])
@pytest.mark.parametrize("elem_bytes,mark_word", [(16, -1), (16, 3), (32, -1), (32, 0), (32, 7), (48, -1), (48, 5), (48, 11)])
def test_gather_records_is_records_of_order(hooks, elem_bytes, mark_word, or_into_word):
    """n = 1,501: several blocks of 256 and a partial one.  The mark word becomes 0 / 1, or keeps its upper 31 bits and gets the mark in bit 0."""
    n, words = 1501, elem_bytes // 4
    rng = np.random.default_rng(elem_bytes * 100 + mark_word * 2 + or_into_word + 7)
    records = rng.integers(0, 1 << 32, (n, words), dtype=np.uint64).astype(np.uint32)
    order = rng.permutation(n).astype(np.uint32)
    last = (rng.random(n) < 0.4).astype(np.uint8)
    out = np.zeros_like(records)
    assert hooks.rtt_gather_records(records.ctypes.data, n, elem_bytes, order.ctypes.data, last.ctypes.data, mark_word, or_into_word, out.ctypes.data) == 0
    want = records[order]
    if mark_word >= 0:
        want[:, mark_word] = ((want[:, mark_word] & np.uint32(0xFFFFFFFE)) | last) if or_into_word else last
    assert np.array_equal(out, want), f"{(out != want).any(axis=1).sum()} records differ"


@pytest.mark.parametrize("elem_bytes", [8, 20, 24, 40])
def test_gather_records_refuses_a_size_that_is_no_multiple_of_16(hooks, elem_bytes):
    n = 64
    records, out = np.arange(n * elem_bytes // 4, dtype=np.uint32), np.zeros(n * elem_bytes // 4, np.uint32)
    order, last = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint8)
    assert hooks.rtt_gather_records(records.ctypes.data, n, elem_bytes, order.ctypes.data, last.ctypes.data, -1, 0, out.ctypes.data) < 0
    assert not out.any()

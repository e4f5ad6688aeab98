"""rt_ref_walk.h frame_sum on the device (the rtt_frame_sum hook: one tree per thread over a node table of the test's own) against the model
of test_frame_sum_model.py, bit for bit, in the three forms the kernels use: 64 deep with a private stack, 64 deep with the strided LDS
view of the persistent kernel's exact role, 128 deep (two tag words, hw6) with a private stack.  Random trees of up to 40 leaves, and
left-deep and right-deep chains of MAXDEPTH - 1, MAXDEPTH and MAXDEPTH + 1 frames: the last meets the depth rule, whose answer the model
defines, and beyond 64 frames the second tag word is in use."""
import ctypes as C
import os

import numpy as np
import pytest

from test_frame_sum_model import bits, chains, frame_sum_model, random_forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
VARIANTS = {"depth64-private": (0, 64), "depth64-lds-stride16": (1, 64), "depth128-private": (2, 128)}


def load_hooks(path):
    L = C.CDLL(path)
    L.rtt_frame_sum.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.rtt_frame_sum.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def hooks():
    return load_hooks(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))


def device_sums(hooks, nodes, roots, variant):
    """-> the bits of the device's total of every root"""
    table = np.array([[k, l, r, bits(v)] for k, l, r, v in nodes], np.uint32)
    rts = np.array(roots, np.uint32)
    out = np.zeros(len(roots), np.float32)
    rc = hooks.rtt_frame_sum(table.ctypes.data, len(table), rts.ctypes.data, len(rts), variant, out.ctypes.data)
    assert rc == 0
    return out.view(np.uint32).tolist()


@pytest.fixture(scope="module")
def forest():
    nodes, roots = random_forest(29, 300)
    return nodes, roots, {d: [bits(frame_sum_model(nodes, r, d)) for r in roots] for d in (64, 128)}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_random_trees_equal_the_model(hooks, forest, name):
    variant, maxdepth = VARIANTS[name]
    nodes, roots, want = forest
    assert device_sums(hooks, nodes, roots, variant) == want[maxdepth]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_chains_at_the_depth_limit_equal_the_model(hooks, name):
    variant, maxdepth = VARIANTS[name]
    nodes, roots = chains(7, maxdepth)
    want = [bits(frame_sum_model(nodes, r, maxdepth)) for r in roots]
    assert device_sums(hooks, nodes, roots, variant) == want

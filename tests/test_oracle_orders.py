"""Pins the permutations the CPU oracle's tree builder leaves behind: the figure order after the scene's BVH is built, the light
order after the lights' BVH is built, and the two trees' node counts and depths.

They are the product of std::partition and of std::sort on tying keys inside the shared builder (oracle/oracle_bvh.h), so they
depend on the exact sequence of comparisons, and everything the oracle renders depends on them.  tests/golden/pins_oracle_orders.npz
was written by tests/golden/make_goldens.py (save_oracle_orders) from an oracle that passes tests/test_oracle_pins.py.  The hw5 oracle
exports its orders but no tree statistics, so its cases pin the two orders only."""
import importlib
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_oracle_orders.npz")
CASES = ["hw5:" + n for n in pin_cases.HW5_CASES] + ["hw6:" + n for n in sorted(pin_cases.HW6_CASES)] + ["hw8:sphere", "hw8:soup"]


def orders(case):
    """{name: uint32 array} of one case through the oracle that takes its scene."""
    hw, name = case.split(":")
    if hw == "hw5":
        rt = importlib.import_module("raytracing-course-hw_amd")
        sd = rt.load_txt(os.path.join(pin_cases.SCENES, "txt", name + ".txt"), rt.RT_INTEGRATOR_HW5)[0]
        fo, lo = oracle_lib.Hw5Oracle(sd).orders()
        return {"figure_order": fo, "light_order": lo}
    if hw == "hw6":
        orc = oracle_lib.Hw6Oracle(pin_cases.HW6_CASES[name][0]())
    else:
        orc = oracle_lib.Hw8Oracle(pin_cases.load_sphere() if name == "sphere" else pin_cases.random_triangle_scene())
    return {"figure_order": orc.figure_order(), "light_order": orc.light_order(), "bvh_stats": orc.bvh_stats()}


@pytest.mark.parametrize("case", CASES)
def test_orders_and_tree_shape_are_pinned(case):
    gold = np.load(GOLD)
    got = orders(case)
    assert len(got["figure_order"]) > 1 and len(got["light_order"]) > 0        # the cases have something to permute
    assert np.array_equal(np.sort(got["figure_order"]), np.arange(len(got["figure_order"])))
    for k, v in got.items():
        g = gold[f"{case}/{k}"]
        assert v.dtype == g.dtype and np.array_equal(v, g), f"{case}: {k} differs from the pinned one"
    assert sorted(k for k in gold.files if k.startswith(case + "/")) == sorted(f"{case}/{k}" for k in got)


def test_soup_figure_order_matches_live_reference():
    """Where the reference's hw8 builder is compiled (oracle/_ref), it leaves the same figure order on the triangle soup."""
    if oracle_lib.ref_path("libref_hw8.so") is None:
        return
    sd = pin_cases.random_triangle_scene()
    assert np.array_equal(oracle_lib.Hw8Oracle(sd).figure_order(), oracle_lib.Ref8(sd).figure_order())

"""Pins the CPU oracle's shading layer (oracle/oracle_hw8.cpp: MaterialModel, Vndf, cosine sampling; oracle_common.h: the tone-mapping)
to the compiled reference at the branch points of that code.  The cases are tests/shading_cases.py; the reference's answers are
tests/golden/pins_shading_edges.npz (golden/make_goldens.py).  The bar is equal bits, or NaN on both sides.  The same cases then hold
the device functions to the same file (test_gpu_shading.py)."""
import os

import numpy as np
import pytest

import oracle_lib
import shading_cases as sc
from test_gpu_device_math import _same_bits_or_both_nan

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_shading_edges.npz")
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def differing(got, want):
    """Indices of the cases (rows) on which the two sides differ: other than equal bits or NaN on both sides."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ok = _same_bits_or_both_nan(got, want) if got.dtype == F else got == want
    return np.flatnonzero(~ok.reshape(len(ok), -1).all(axis=1))


@pytest.mark.parametrize("family", sc.REFERENCE_FAMILIES)
def test_oracle_equals_reference_at_the_edges(gold, family):
    got, want = sc.oracle_answers()[family], gold[family]
    bad = differing(got, want)
    print(f"{family}: {len(want)} cases, {bad.size} differ from the reference")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_cases_reach_the_branches_they_claim(gold):
    """Counted over the reference's answers, so that a change of the table that loses an edge fails here and not silently."""
    r = sc.reach(gold)
    print(r)
    for family, share in r["nan_share"].items():
        assert share <= 0.10, (family, share)                # numbers carry the comparison
    assert r["brdf_specular_nonzero"] >= 200
    assert r["brdf_gate_zeroed"] >= 200                      # the specular term is 0 because a half-vector dot is below 1e-4, and for no other reason
    assert min(r["brdf_vn"]) >= 50 and min(r["brdf_ln"]) >= 50     # either side of v.n >= 0 and of l.n >= 0, among the cases answered with numbers
    assert r["brdf_vn_zero"] >= 50 and r["brdf_ln_zero"] >= 50     # and the value 0 itself, of either sign
    assert r["brdf_gate_exact"] >= 24                         # a half-vector dot equal to the float 1e-4: a float comparison and the double one part here
    assert min(r["vndf_getq"]) >= 20
    assert r["tonemap_bytes"] == 256
    # the threshold family has every target with the other dot clear of the gate: the case's answer turns on the one comparison
    b = sc.families()["brdf"]
    hd = sc.half_dots(b["l"], b["v"])
    for which in (0, 1):
        for target in (sc.GATE - 1, sc.GATE, sc.GATE + 1):
            assert ((sc.bits(hd[:, which]) == target) & (hd[:, 1 - which] > 1.05e-4)).sum() >= 6, (which, hex(target))
    # vndf_local: points beyond the unit circle (the remainder under the root is negative), at vT = +z where the sampler leaves t2 as it is
    v = sc.families()["vndf_local"]
    up = (v["vT"] == F([0, 0, 1])).all(axis=1)
    rem = (1.0 - (v["t1"] * v["t1"]).astype(np.float64) - (v["t2"] * v["t2"]).astype(np.float64)).astype(F)
    assert (up & (rem < 0)).sum() >= 8 and (up & (rem == 0)).sum() >= 8
    assert ((v["vT"][:, :2] == 0).all(axis=1)).sum() >= 50   # lensq = 0
    # cosine: every exit of the sampler's three-way fallback (l <= eps, d.n <= eps, NaN) and the ordinary one
    c = sc.families()["cosine"]
    back = (sc.bits(gold["cosine"][:, :3]) == sc.bits(c["n"])).all(axis=1) | np.isnan(gold["cosine"][:, :3]).any(axis=1)
    assert (~back).sum() >= 1900 and back.sum() >= 40


def test_golden_is_current_with_live_reference(gold):
    """Where the reference harnesses are built (and have the entry points), the file is what they answer today."""
    import ctypes as C
    p8, p7 = oracle_lib.ref_path("libref_hw8.so"), oracle_lib.ref_path("libref_hw7.so")
    if p8 is None or p7 is None or not hasattr(C.CDLL(p8), "ref8_cosine_sample_pdf") or not hasattr(C.CDLL(p7), "ref7_brdf"):
        print("oracle/_ref is not built from this tree's harnesses: pins_shading_edges.npz not re-evaluated live")
        return
    live = sc.evaluate("reference")
    for family in sc.REFERENCE_FAMILIES:
        assert differing(live[family], gold[family]).size == 0, family


def test_oracle_only_families_have_answers():
    """vndf_local and cosine_pdf have no entry in the reference (Vndf::sample_ is private; Cosine::pdf is reached through a sample): the oracle's
    answers are what the device is held to (Vndf::sample_local is the tail of Vndf::sample_, which the vndf family pins through Vndf::sample).
    Here: the answers exist, numbers carry the comparison, and max(0.f, .) answers +0 for a zero of either sign."""
    o = sc.oracle_answers()
    assert len(o["vndf_local"]) == len(sc.families()["vndf_local"]["alpha"]) and len(o["cosine_pdf"]) == len(sc.families()["cosine_pdf"]["d"])
    assert np.isnan(o["vndf_local"]).any(axis=1).mean() <= 0.10
    assert o["cosine_pdf"][:3].tolist() == [0.0, 0.0, 0.0] and not np.signbit(o["cosine_pdf"][:3]).any()     # d.n = +0, +0, -0: max(0.f, .) answers +0

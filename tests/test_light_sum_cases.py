"""The light-sum cases (tests/light_sum_cases.py) can tell associations apart, and the oracle's association on them is the reference's.

Conditions on the inputs, checked with the oracle alone: every hit count from 0 to L occurs, one- and two-hit sums are their terms
(so hit_terms' terms are the sum's terms), and a sum of three or more terms often differs in bits from the plain left fold of those
terms, so a consumer that adds them in another shape than the reference's light tree is caught.  Then Hw8Oracle.light_pdf and
Hw8Oracle.render are held bit for bit to tests/golden/pins_light_sums.npz, which tests/golden/make_goldens.py records from the compiled
reference (FiguresMix::pdf, and hw8's own scene.cpp for the frames), and to the live reference where oracle/_ref is built.

Measured with these seeds (profiles/r37_light_sums.txt): on L = 12, "through" has 25 to 133 rays per hit count 0 .. 12 and the left fold
differs in 282 of 805 sums of three or more terms (35 %), in none of 219 with at most two."""
import os

import numpy as np
import pytest

import light_sum_cases as lc
import oracle_lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_light_sums.npz")
CASES = [(L, which) for L in lc.HW8_LAYERS for which in lc.RAY_SETS]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("L", [L for L in lc.HW8_LAYERS if L >= 3])
def test_every_hit_count_occurs(L):
    k = lc.hit_counts(lc.terms_of(L, "through"))
    hist = np.bincount(k, minlength=L + 1)
    print(f"L = {L}, through: rays per hit count {hist.tolist()}")
    assert len(hist) == L + 1 and np.all(hist > 0), hist.tolist()
    k_diag = lc.hit_counts(lc.terms_of(L, "diagonal"))
    assert k_diag.max() > L                        # a ray in the plane of the shared diagonals counts some layer twice


@pytest.mark.parametrize("L", lc.HW8_LAYERS)
def test_one_and_two_hit_sums_are_their_terms(L):
    """What makes hit_terms valid: the sum is divided by the light count after the additions, so a one-light scene's pdf is the term."""
    n = np.float32(2 * L)
    seen = 0
    for which in lc.RAY_SETS:
        terms, orc = lc.terms_of(L, which), lc.oracle_pdfs(L, which)
        k = lc.hit_counts(terms)
        assert np.all(orc[k == 0] == 0) and np.all(orc[k > 0] != 0)
        plain = (terms.astype(np.float32).sum(axis=1, dtype=np.float32) / n).astype(np.float32)   # one or two terms: one rounding at most
        m = (k == 1) | (k == 2)
        assert np.array_equal(bits(plain[m]), bits(orc[m])), which
        assert np.array_equal(bits(lc.left_fold(terms)[k <= 2]), bits(orc[k <= 2])), which
        seen += int(m.sum())
    assert seen >= 100


@pytest.mark.parametrize("L", [L for L in lc.HW8_LAYERS if L >= 3])
def test_left_fold_differs_from_the_tree_sum(L):
    """At least 10 % of the sums of three or more terms differ in bits from the left fold in light order: in "through" and over all sets."""
    differs, many = [], []
    for which in lc.RAY_SETS:
        terms, orc = lc.terms_of(L, which), lc.oracle_pdfs(L, which)
        k = lc.hit_counts(terms)
        diff = bits(lc.left_fold(terms)) != bits(orc)
        print(f"L = {L}, {which}: left fold differs in {int(diff[k >= 3].sum())} of {int((k >= 3).sum())} sums of three or more terms; per hit count "
              + ", ".join(f"{kk}: {int(diff[k == kk].sum())}/{int((k == kk).sum())}" for kk in range(3, k.max() + 1)))
        differs.append(int(diff[k >= 3].sum()))
        many.append(int((k >= 3).sum()))
    assert many[0] >= 100 and differs[0] >= 0.10 * many[0]
    assert sum(differs) >= 0.10 * sum(many)


@pytest.mark.parametrize("L,which", CASES)
def test_oracle_light_pdf_is_the_references(gold, L, which):
    o, d = lc.rays(L, which)
    key = lc.fixture_key(L, which)
    assert np.array_equal(bits(gold[key + "_o"]), bits(o)) and np.array_equal(bits(gold[key + "_d"]), bits(d)), "the fixture answers other rays: regenerate it"
    orc = lc.oracle_pdfs(L, which)
    bad = np.nonzero(bits(orc) != bits(gold[key + "_pdf"]))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(o)} sums differ from the reference's, first rays {bad[:5].tolist()}, hit counts {lc.hit_counts(lc.terms_of(L, which))[bad[:5]].tolist()}"
    if oracle_lib.ref_path("libref_hw8.so"):
        live = lc.light_pdfs(oracle_lib.Ref8(lc.stack_scene(L)), o, d)
        assert np.array_equal(bits(live), bits(gold[key + "_pdf"])), "stored sums differ from the live reference"


@pytest.mark.parametrize("L", lc.FRAME_LAYERS)
def test_oracle_frame_is_the_references(gold, L):
    w, h, spp = lc.FRAME
    sd = lc.stack_scene(L)
    rgb, rgb8, cnt = oracle_lib.Hw8Oracle(sd).render(w, h, spp)
    print(f"L = {L}: {cnt.lightq} light-pdf queries in the {w}x{h}x{spp} frame")
    assert cnt.lightq > w * h * spp
    assert np.array_equal(bits(rgb), bits(gold[f"L{L}_frame_rgb"])) and np.array_equal(rgb8, gold[f"L{L}_frame_rgb8"])
    if oracle_lib.ref_path("libref_hw8_scene.so"):
        live, live8, _ = oracle_lib.Ref8Scene(sd).render(w, h, spp)
        assert np.array_equal(bits(live), bits(gold[f"L{L}_frame_rgb"])) and np.array_equal(live8, gold[f"L{L}_frame_rgb8"]), "stored frame differs from the live reference"


@pytest.mark.parametrize("L,seed", lc.HW6_FRAMES)
def test_hw6_oracle_frame_is_the_references_where_built(L, seed):
    """The hw6 frames of tests/test_gpu_light_sums_hw6.py: Hw6Oracle against the compiled hw6 scene.cpp where oracle/_ref holds it (no
    fixture: the GPU test's referee is the oracle, pinned here and by tests/test_oracle_pins.py)."""
    w, h, spp = lc.FRAME
    sd = lc.stack_scene(L, seed, hw6=True)
    rgb, rgb8, cnt = oracle_lib.Hw6Oracle(sd).render(w, h, spp)
    assert np.isfinite(rgb).all() and rgb.mean() > 0.01 and cnt.lightq > 0
    if oracle_lib.ref_path("libref_hw6.so"):
        live, live8, _ = oracle_lib.Ref6(sd).render(w, h, spp)
        assert np.array_equal(bits(rgb), bits(live)) and np.array_equal(rgb8, live8)

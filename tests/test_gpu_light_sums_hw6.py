"""Light-pdf sums on the GPU by hit count, hw6: 32x24x8 frames of the stack scenes of tests/light_sum_cases.py (hw6 flavour) through the
persistent hw6 kernel, bit for bit the oracle's pixels (Hw6Oracle, held to the compiled hw6 reference by tests/test_light_sum_cases.py on
these very frames, and here again where oracle/_ref holds it).

The hw6 kernel adds a light sum on one of five paths by its number of hits (device/rt_persistent_hw6.h): P6LightWalk::end adds three
hits and four hits inline (four: five spelled-out outcomes of the separation depths), p6_merge_hits adds 5 .. 13 (P6_MERGE_HITS) in the
lane's own column, p6_merge_hits_in 14 .. 16 (RT6_MAX_LIGHT_HITS) in a batch slice, and beyond that, or with a hit at a box boundary, the
sum is walked in the reference's order.  L = 3, 4, 13, 16, 20 layers lie on either side of each boundary.  A counting render with
RTAMD_DEBUG_COUNTERS=1 reports the hit counts that reached the slow role, which shows that the paths from five hits up ran.

The inline three- and four-hit paths have no counter.  On the L = 3 and L = 4 frames a ray meets at most three or four layers and
nothing reaches the slow role with five hits or more, so no other path can have produced those sums.  But a one-off census with a
throwaway counter (profiles/r37_light_sums.txt) showed that the 1,206 three-hit sums of the L = 3 frame all take one of the two
three-hit outcomes and the 355 four-hit sums of the L = 4 frame one of the five four-hit outcomes: the same few layers give the same
few index patterns.  light_sum_cases.HW6_OUTCOME_FRAMES adds five frames (5, 6 and 8 layers, other seeds) on which every outcome is
taken by 87 sums at least; there three and four hits still come from the inline path only, as the slow role starts at five.  The
15+ bin lumps 15 and 16 hits (p6_merge_hits_in) with 17 and more (the walk in the reference's order)."""
import re

import numpy as np
import pytest

import light_sum_cases as lc
import oracle_lib

pytestmark = pytest.mark.gpu
RMSE_TOL = 1e-3  # tests/test_gpu_parity_hw6.py: BASELINE.json north_star tolerance on linear radiance
SLOW_BINS = re.compile(r"light sums in the slow role by number of hits \(0\.\.14, 15\+\):((?: \d+){16})")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_frames():
    w, h, spp = lc.FRAME
    return {(L, seed): oracle_lib.Hw6Oracle(lc.stack_scene(L, seed, hw6=True)).render(w, h, spp) for L, seed in lc.HW6_FRAMES}


@pytest.mark.parametrize("kernel", ["persistent", "mega"])
@pytest.mark.parametrize("L,seed", lc.HW6_FRAMES)
def test_frames(rt, monkeypatch, oracle_frames, L, seed, kernel):
    """Persistent: the oracle's floats and bytes (and the live reference's where it is built); the per-lane path machine follows the rule
    of test_hw6_scene_matches_oracle."""
    w, h, spp = lc.FRAME
    monkeypatch.setenv("RTAMD_KERNEL", kernel)
    sd = lc.stack_scene(L, seed, hw6=True)
    ref, ref8, cnt = oracle_frames[L, seed]
    scene = rt.Scene(sd)
    try:
        assert np.array_equal(scene.light_order(), oracle_lib.Hw6Oracle(sd).light_order())
        rgb, rgb8, st = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW6)
    finally:
        scene.close()
    rmse = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref) ** 2)))
    bad = int((np.abs(rgb.astype(np.float64) - ref).max(axis=2) > 1e-3).sum())
    print(f"hw6 L = {L}, seed {seed}, {kernel}: rmse {rmse:.3e}, desync pixels {bad}, byte mismatches {(rgb8 != ref8).sum()}, exact {np.array_equal(bits(rgb), bits(ref))}; "
          f"the oracle asked {cnt.lightq} light pdfs")
    assert ref.mean() > 0.01
    if kernel == "mega":
        assert st.pipeline == rt.RT_PIPELINE_SINGLE and rmse < RMSE_TOL and bad <= 1
        return
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.reference_exact == 1
    assert np.array_equal(bits(rgb), bits(ref)) and np.array_equal(rgb8, ref8)
    if oracle_lib.ref_path("libref_hw6.so"):
        live, live8, _ = oracle_lib.Ref6(sd).render(w, h, spp)
        assert np.array_equal(bits(rgb), bits(live)) and np.array_equal(rgb8, live8)


@pytest.mark.parametrize("L", lc.HW6_LAYERS)
def test_slow_role_hit_counts(rt, monkeypatch, capfd, oracle_frames, L):
    """The counting render gives the plain frame's pixels, and its report shows which hit counts reached the slow role: none of five or
    more on L = 4 (so three and four hits were added inline), every count from 5 to 13 on L = 13 (p6_merge_hits), 14 and 15+ on L = 20
    (p6_merge_hits_in and the walk in the reference's order)."""
    w, h, spp = lc.FRAME
    monkeypatch.setenv("RTAMD_KERNEL", "persistent")
    monkeypatch.setenv("RTAMD_DEBUG_COUNTERS", "1")
    ref, ref8, _ = oracle_frames[L, lc.SEED]
    scene = rt.Scene(lc.stack_scene(L, hw6=True))
    try:
        plain, plain8, _ = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW6)
        capfd.readouterr()
        rgb, rgb8, st = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW6, counters=True)
        err = capfd.readouterr().err
    finally:
        scene.close()
    found = SLOW_BINS.findall(err)
    assert len(found) == 1, err
    bins = [int(x) for x in found[0].split()]
    print(f"hw6 L = {L}: slow-role light sums by hits (0..14, 15+) {bins}; {st.light_pdf_queries} light-pdf queries, exact light sums {st.exact_light_sums}")
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and st.reference_exact == 1
    assert np.array_equal(bits(rgb), bits(plain)) and np.array_equal(rgb8, plain8)
    assert np.array_equal(bits(rgb), bits(ref)) and np.array_equal(rgb8, ref8)
    if L <= 4:
        assert not any(bins[5:]), bins
    if L == 13:
        assert all(bins[5:14]), bins
    if L == 20:
        assert bins[14] > 0 and bins[15] > 0, bins

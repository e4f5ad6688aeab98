"""Pins the CPU oracle's analytic figures, light pdf and samplers of the .txt snapshots (oracle_txt_prims.h, oracle_hw2.cpp, oracle_txt.cpp,
oracle_hw4.cpp, oracle_hw5.cpp) to the compiled reference at the branch points of that code.  The cases are tests/analytic_cases.py; the
reference's answers are tests/golden/pins_analytic_edges.npz (golden/make_goldens.py, through oracle/ref/ref_txt_funcs.cpp).  The bar is
equal bits, or NaN on both sides; engine states and normal caches are words and must be equal.  The same cases then hold the device
functions to the same file (test_gpu_analytic.py)."""
import os

import numpy as np
import pytest

import analytic_cases as ac

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_analytic_edges.npz")
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_oracle_equals_reference_at_the_edges(gold, family):
    got, want = ac.oracle_answers()[family], gold[family]
    bad = ac.differing(got, want)
    print(f"{family}: {len(want)} cases, {bad.size} differ from the reference")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_quad_reaches_its_branches(gold):
    r = ac.reaches("quad", gold)
    print(r)
    assert r["hit"] >= 1000 and r["miss"] >= 1000 and r["inside"] >= 500 and r["outside"] >= 200
    assert r["discriminant_zero_rejected"] == r["discriminant_zero_rows"] >= 200            # d == 0 exactly: `d <= 0` rejects
    assert r["discriminant_denormal_hit"] >= 100
    assert r["nan_t_outside"] >= 10                                                         # a NaN discriminant or root passes every comparison: a hit, outside
    assert r["a_zero_hit"] >= 20 and r["a_zero_miss"] >= 5                                  # a == +-0: roots of +-inf and 0/0
    assert r["a_negative_hit"] >= 500                                                       # the root swap
    assert min(r["minus_zero_outside"]) >= 10                                               # x1 == -0: `x1 < 0` is false, the hit is outside with t = -0 (both root forms)
    assert r["minus_zero_inside"] >= 5 and r["plus_zero"] >= 10
    # The two root forms on the same (a, b, c): hw2 rounds the root, the difference and the quotient to float, hw3 narrows once.
    assert r["forms_differ_in_t"] >= 500


def test_slabs_reach_their_branches(gold):
    r = ac.reaches("slabs", gold)
    print(r)
    assert r["accepted"] >= 1500 and r["rejected"] >= 400 and r["inside"] >= 400
    # 0/0 with the origin on the low face: std::min / std::max hand the NaN on from their first operand only.  On x it reaches t1 and t2
    # (accepted, t = NaN); on y and z it is dropped and the other axes decide.  On the high face the interval is an infinity twice: rejected.
    assert r["nan_accepted_per_axis"][0] == r["nan_t_per_axis"][0] >= 60 and r["nan_rejected_per_axis"][0] == 0
    assert min(r["nan_accepted_per_axis"][1:]) >= 20 and min(r["nan_rejected_per_axis"][1:]) >= 5 and r["nan_t_per_axis"][1:] == [0, 0]
    assert r["high_face_accepted"] == 0
    assert r["graze_accepted"] >= 10                                                        # t1 == t2 is no rejection
    assert min(r["zero_t"]) >= 10                                                           # t1 == +0, t1 == -0 (outside), t2 == +0, t2 == -0 (inside)


def test_figures_reach_their_branches(gold):
    r = ac.reaches("fig", gold)
    print(r)
    assert min(r["hit_per_type"]) >= 300 and min(r["miss_per_type"]) >= 200 and min(r["inside_per_type"]) >= 100
    assert r["ellipsoid_tangent_miss"] >= 15                                                # the discriminant at 0 through the figure
    assert r["nan_t_hit_outside"] >= 20 and r["ellipsoid_a_zero_rows"] >= 5
    assert r["box_two_components"] >= 40 and r["box_three_components"] >= 60                # edges and corners: the normal keeps more than one component
    assert r["box_zero_size_nan_normal"] >= 3
    assert r["plane_inf_t_hw3_only"] >= 10 and r["plane_dn_zero_nan_miss"] >= 20            # dn == +-0: t = +inf is a hit without T_MAX, NaN and -inf are none
    assert r["plane_t_below_tmax"] >= 8 and min(r["plane_t_at_or_above_tmax_hw3_only"]) >= 4   # t one step below 1e4f, on it, above it
    assert r["plane_t_zero_miss"] >= 4 and r["plane_t_zero_hit"] >= 2
    # hw1 takes the plane's normal as the file has it; the rows give hw2 the same normal, and the two snapshots' float forms then agree in t
    assert r["hw1_plane_normal_not_unit_hit"] >= 300 and r["hw1_differs_from_hw2_in_t"] == 0
    assert r["hw2_differs_from_hw3"] >= 100 and r["hw3_differs_from_hw4"] >= 20 and r["hw4_differs_from_hw5"] == 0
    assert min(r["quaternions"].values()) >= 150                                            # every rotation on at least 50 rows of each figure type


def test_triangles_reach_their_branches(gold):
    r = ac.reaches("tri5", gold)
    print(r)
    assert r["hit"] >= 400 and r["miss"] >= 1000 and r["inside"] >= 200 and r["outside"] >= 200
    # p exactly on an edge makes that edge's test a zero of either sign, and `< 0` lets both through
    for name in ("edge_b_plus_zero", "edge_b_minus_zero", "edge_c_plus_zero", "edge_c_minus_zero"):
        assert r[name][0] >= 20 and r[name][1] == 0, name
    assert r["edge_third"][0] >= 20
    assert min(r["beside_edges"]) >= 50 and r["body"][0] >= 50 and r["body"][1] == 0
    assert r["degenerate_miss"] >= 6
    assert r["t_below_tmax"] >= 8 and r["t_max_miss"] >= 12                                 # t below 1e4f hits; on it and above it misses
    assert min(r["windings"]) >= 100                                                        # the negated cross product: `inside` on both sides


def test_light_pdf_reaches_its_branches(gold):
    r = ac.reaches("lpdf", gold)
    print(r)
    assert r["zero"] >= 1000 and min(r["positive_per_type"]) >= 90
    assert r["infinite_from_nan_t"] >= 30 and r["infinite_from_nan_t_hw4"] >= 30            # `if (std::isnan(t)) return INFINITY`
    assert r["infinite_from_perpendicular_normal"] >= 8                                     # d . yn == 0
    assert r["inside_rows_positive"] >= 300                                                 # x inside the light: the first hit is the exit
    assert r["triangle_positive"] >= 90                                                     # the triangle's early return
    assert min(r["first_hit_only_per_type"]) >= 150 and min(r["second_hit_per_type"]) >= 500   # one term of the sum, and two
    assert r["inside_rows_first_hit_only"] == r["inside_rows_positive"]                     # from inside, the query from t + 1e-4 misses
    # t + eps where one step of its float moves the second origin: 120 and 200 rows, the second hit present on at least a third of them
    assert r["tiny_first_t_rows"] == 120 and r["tiny_figure_rows"] == 200
    assert r["tiny_first_t_second_hit"] >= 40 and r["tiny_figure_second_hit"] >= 70
    # hw5 forms t + eps in 80 bits where hw4 (and the device) form it in double: the two may part on at most 1 row in 10,000
    print("hw4 and hw5 differ on", r["hw4_differs_from_hw5"], "rows")
    assert r["hw4_differs_from_hw5"] * 10000 <= r["rows"]


def test_pdf_one_reaches_its_branches(gold):
    r = ac.reaches("pone", gold)
    print(r)
    assert min(r["positive_finite_per_type"]) >= 350
    assert r["y_equals_x_zero"] >= 6 and r["y_equals_x_nan"] >= 3                           # |x - y|^2 == 0: 0, and 0 / 0 where d . yn == 0 too
    assert r["dot_zero_infinite"] >= 15 and r["dot_zero_finite"] >= 6                       # d . yn == +0 and -0; the smallest products beside them
    assert r["ellipsoid_centre_infinite"] >= 2 and r["ellipsoid_centre_nan"] >= 1           # n == 0: 1 / 0, and inf * 0 with y == x
    assert r["no_area_not_finite"] >= 6                                                     # sTotal == 0, a degenerate triangle, a zero radius
    assert r["nan"] >= 15 and r["infinite"] >= 25
    assert r["hw4_differs_from_hw5"] == 0                                                   # the same two lines in both snapshots


def test_light_samplers_reach_their_branches(gold):
    r = ac.reaches("lsample", gold)
    att = ac.attempts()
    ell = ac.rows("lsample")[:, 0] == ac.ELLIPSOID
    r["ellipsoid_rejecting"] = int((att[ell, 1] > 1).sum())
    r["max_attempts"] = int(att.max())
    print(r)
    assert max(r["max_draws"]) <= ac.MAX_DRAWS
    assert r["ellipsoid_rejecting"] >= 50                                                   # far away, the discriminant is rounding noise
    assert r["box_rejecting"] >= 20 and r["box_in_face_plane_rejecting"] >= 20              # more draws than the four of one attempt
    assert r["box_draws_not_multiple_of_4"] == 0 and r["triangle_draws_not_2"] == 0
    assert r["cache_used"] >= 200 and r["cache_left"] >= 200 and r["hw4_cache_changed"] >= 400
    assert r["box_cache_untouched"] == r["box_rows"]
    for kind in ("box_u_boundary", "box_u_zero", "box_flip_half", "fold_sum_one_exact_above", "fold_sum_one_exact_below", "fold_just_above"):
        assert r["kinds"][kind] >= 2, kind


def test_box_face_point_draws_in_the_reference_order():
    """One round's point of BoxLight::sample through the oracle (the reference keeps it in a local: the fixture cannot hold it) against
    the four uniforms of the row's engine put together in float32 here: u picks the face at `u < wx` and `u < wx + wy`, the second draw
    the sign at `> 0.5`, and of the two coordinates the LAST one takes the earlier draw.  Exactly four engine steps."""
    import oracle_lib
    L = oracle_lib.lib()
    s, seeds, kind = ac.face_point_cases()
    got = ac.face_point_oracle()
    assert np.array_equal(ac.draws(seeds, got[:, 3]), np.full(len(s), 4))
    want = np.zeros((len(s), 3), F)
    faces, u = np.zeros(len(s), int), np.zeros(4, F)
    on_wx = on_wxy = half = 0
    with np.errstate(all="ignore"):
        for i in range(len(s)):
            L.rto_rng_kat(int(seeds[i]), 4, 0, u.ctypes.data)
            sx, sy, sz = s[i]
            wx, wy, wz = sy * sz, sx * sz, sx * sy
            pick = u[0] * ((wx + wy) + wz)
            flip = F(1) if u[1] > 0.5 else F(-1)
            late, early = (F(2) * u[3] - F(1)), (F(2) * u[2] - F(1))
            face = 0 if pick < wx else 1 if pick < wx + wy else 2
            want[i] = [(flip * sx, late * sy, early * sz), (late * sx, flip * sy, early * sz), (late * sx, early * sy, flip * sz)][face]
            faces[i] = 2 * face + (flip > 0)
            on_wx += pick == wx
            on_wxy += pick == wx + wy
            half += u[1] == 0.5
    bad = ac.differing(got[:, 0:3], ac.bits(want))
    print(f"box face point: {len(s)} cases, {bad.size} differ; per face and sign {np.bincount(faces, minlength=6).tolist()}, u on wx {on_wx}, on wx + wy {on_wxy}, flip on 0.5 {half}")
    assert bad.size == 0, (bad[:5].tolist(), got[bad[:5]].tolist(), ac.bits(want)[bad[:5]].tolist())
    assert np.bincount(faces[kind == 0], minlength=6).min() >= 50 and on_wx >= 2 and on_wxy >= 2 and half >= 2


def test_cosine_reaches_the_fallback(gold):
    r = ac.reaches("cosine", gold)
    print(r)
    assert r["fallback_opposite"] >= 20 and r["opposite_not_fallback"] >= 20 and r["cache_used"] >= 300


def test_boundary_seeds_draw_what_they_claim(gold):
    """The seeds placed by integer arithmetic give the uniforms they were placed for, by the oracle's own engine."""
    import oracle_lib
    L = oracle_lib.lib()
    fam = ac.families()["lsample"]
    u = np.zeros(2, F)
    seen = {}
    for kind, k in fam["K"].items():
        if not (kind.startswith("box_") and kind != "box_in_face_plane") and not kind.startswith("fold_"):
            continue
        for seed in fam["aux"][fam["kind"] == k, 0]:
            L.rto_rng_kat(int(seed), 2, 0, u.ctypes.data)
            seen.setdefault(kind, []).append((float(u[0]), float(u[1]), float(F(u[0] + u[1])), float(u[0]) + float(u[1])))
    third, two_thirds = F(1) / F(3), F(2) / F(3)
    firsts = {F(v[0]) * F(3) for v in seen["box_u_boundary"]}
    assert {F(1), F(2)} <= firsts and any(x < 1 for x in firsts) and any(1 < x < 2 for x in firsts) and any(x > 2 for x in firsts)
    assert {F(v[0]) for v in seen["box_u_boundary"]} >= {third, two_thirds}
    assert all(v[0] == 0 for v in seen["box_u_zero"])
    assert {v[1] for v in seen["box_flip_half"]} >= {0.5} and any(v[1] < 0.5 for v in seen["box_flip_half"]) and any(v[1] > 0.5 for v in seen["box_flip_half"])
    assert all(v[2] == 1 and v[3] > 1 for v in seen["fold_sum_one_exact_above"])
    assert all(v[2] == 1 and v[3] <= 1 for v in seen["fold_sum_one_exact_below"])
    assert all(v[2] > 1 for v in seen["fold_just_above"])


def test_golden_is_current_with_live_reference(gold):
    """Where the reference harnesses are built, the file is what they answer today."""
    if not ac.reference_built():
        print("oracle/_ref is not built from this tree's harnesses: pins_analytic_edges.npz not re-evaluated live")
        return
    live = ac.evaluate("reference")
    for family in ac.FAMILIES:
        assert np.array_equal(live[family], gold[family]), family

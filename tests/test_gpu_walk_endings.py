"""The endings of a walk in the persistent kernels' walker loop (rt_persistent.h pt_walk_stint), on the GPU: a walk ends by an empty stack column
with or without parked leaves, in the node loop, at its head or after a leaf phase, or by a full column, and leaves only a mark in `cur` until
its end() runs.  The full column needs a deep tree and a grazing ray on real scenes; RTAMD_PT_STACK_CAP=3 makes the counting kernels take it on
nearly every walk of a small scene (the exact role then redoes those queries: same pixels, more exact walks).  RTAMD_TRACE_LEAF_BATCH=1 and =64
are the two extremes of the ballot that ends a node phase: lanes that end while leaves are parked, and lanes that end drained.
Scenes: the soup of 700 triangles (230 emissive) and the emissive sphere, as tests/test_gpu_edge_cases.py renders them; hw6_soup for the hw6 kernel."""
import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(rt, sphere_scene, name):
    """scene data, frame, and the two references (computed once): the oracle's frame and the round pipeline's"""
    if name not in _CACHE:
        sd, frame = (sphere_scene, (64, 48, 5)) if name == "sphere" else (pin_cases.random_triangle_scene(n=700, seed=21), (72, 48, 5))
        orc, orc8, _ = oracle_lib.Hw8Oracle(sd).render(*frame)
        _CACHE[name] = (sd, frame, orc, orc8)
    return _CACHE[name]


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["soup", "sphere"])
def test_hw8_walk_endings(rt, sphere_scene, monkeypatch, name):
    sd, frame, orc, orc8 = _case(rt, sphere_scene, name)
    scene = rt.Scene(sd)
    monkeypatch.setenv("RTAMD_KERNEL", "wavefront")
    rounds = scene.render(*frame)
    monkeypatch.setenv("RTAMD_KERNEL", "persistent")
    plain = scene.render(*frame)
    assert plain[2].pipeline == rt.RT_PIPELINE_PERSISTENT and rounds[2].pipeline == rt.RT_PIPELINE_ROUNDS
    assert _same(plain, (orc, orc8)) and _same(plain, rounds)

    count = scene.render(*frame, counters=True)
    monkeypatch.setenv("RTAMD_PT_STACK_CAP", "3")
    capped = scene.render(*frame, counters=True)
    knob_plain = scene.render(*frame)
    monkeypatch.delenv("RTAMD_PT_STACK_CAP")
    st, stc, stk, stp = plain[2], count[2], capped[2], knob_plain[2]
    print(f"{name}: queries {st.closest_hit_queries}+{st.light_pdf_queries}; exact walks plain {st.exact_closest_hits}+{st.exact_light_sums}, "
          f"counting {stc.exact_closest_hits}+{stc.exact_light_sums}, counting with a cap of 3 {stk.exact_closest_hits}+{stk.exact_light_sums}; "
          f"node visits {stc.node_visits} -> {stk.node_visits}")
    assert stc.pipeline == rt.RT_PIPELINE_PERSISTENT and stk.pipeline == rt.RT_PIPELINE_PERSISTENT
    assert _same(count, plain) and _same(capped, plain)
    assert stk.exact_closest_hits > stc.exact_closest_hits
    if name == "soup":
        assert stk.exact_light_sums > stc.exact_light_sums
    queries = {(s.closest_hit_queries, s.light_pdf_queries) for s in (st, stc, stk)}
    assert len(queries) == 1 and st.closest_hit_queries > frame[0] * frame[1] * frame[2]
    # the plain kernels hold the cap as an immediate: the knob changes nothing there
    assert _same(knob_plain, plain)
    assert (stp.closest_hit_queries, stp.light_pdf_queries, stp.exact_closest_hits, stp.exact_light_sums) == \
           (st.closest_hit_queries, st.light_pdf_queries, st.exact_closest_hits, st.exact_light_sums)

    for lb in ("1", "64"):
        monkeypatch.setenv("RTAMD_TRACE_LEAF_BATCH", lb)
        batch = scene.render(*frame)
        assert batch[2].pipeline == rt.RT_PIPELINE_PERSISTENT and _same(batch, plain), lb
    scene.close()


def test_hw6_walk_endings(rt, monkeypatch):
    """hw6's walkers take the same loop with immediate endings (P6Roles::DEFER = false): hw6_soup, the smallest scene of
    tests/test_gpu_parity_hw6.py, persistent against its oracle, plain, counting, and counting with the cap of 3."""
    sd = pin_cases.hw6_soup()
    w, h, spp = 64, 48, 8
    kw = dict(integrator=rt.RT_INTEGRATOR_HW6)
    ref, ref8, _ = oracle_lib.Hw6Oracle(sd).render(w, h, spp)
    monkeypatch.setenv("RTAMD_KERNEL", "persistent")
    scene = rt.Scene(sd)
    plain = scene.render(w, h, spp, **kw)
    count = scene.render(w, h, spp, counters=True, **kw)
    monkeypatch.setenv("RTAMD_PT_STACK_CAP", "3")
    capped = scene.render(w, h, spp, counters=True, **kw)
    knob_plain = scene.render(w, h, spp, **kw)
    scene.close()
    st, stc, stk = plain[2], count[2], capped[2]
    print(f"hw6_soup: queries {st.closest_hit_queries}+{st.light_pdf_queries}; exact walks counting {stc.exact_closest_hits}+{stc.exact_light_sums}, "
          f"with a cap of 3 {stk.exact_closest_hits}+{stk.exact_light_sums}")
    assert st.pipeline == rt.RT_PIPELINE_PERSISTENT and stk.pipeline == rt.RT_PIPELINE_PERSISTENT
    assert _same(plain, (ref, ref8)) and _same(count, plain) and _same(capped, plain) and _same(knob_plain, plain)
    assert stk.exact_closest_hits > stc.exact_closest_hits
    assert len({(s.closest_hit_queries, s.light_pdf_queries) for s in (st, stc, stk, knob_plain[2])}) == 1

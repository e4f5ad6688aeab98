"""Light-pdf sums on the GPU by hit count, hw8: rt_query_light_pdf and the renders on the stack scenes of tests/light_sum_cases.py, held
bit for bit to the oracle and to the compiled reference's answers in tests/golden/pins_light_sums.npz.

A sum of three or more terms has the reference's bits only if it is added in the shape of the reference's light tree.  Which consumer
adds it depends on the hit count: wf_merge_light_hits (device/rt_wavefront.h) merges 3 .. 5 (WF_MAX_LIGHT_HITS) hits in the LDS column
for the query and the round pipeline, PtLightWalk::end (device/rt_persistent.h) has its own copy for the persistent kernel, and the
sixth non-zero term sets `overflow`, which sends the sum to the exact walk (frame_sum over the reference's tree).  The ray set
"through" holds every hit count from 0 to L, so each of them is asked with a known count, and the exact-walk counters say which
consumer answered: all of the rays with six or more hits, and at most half of those with three to five (the gate may find a few of
them not robust; the merge must have served the rest).  The oracle's sums are computed once per scene and ray set and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import light_sum_cases as lc
import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pins_light_sums.npz")
RMSE_TOL = 1e-3  # tests/test_gpu_parity_hw8.py: BASELINE.json north_star tolerance on linear radiance
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(L):
        if L not in made:
            made[L] = rt.Scene(lc.stack_scene(L))
        return made[L]
    yield get
    for s in made.values():
        s.close()


def _differing(got, want):
    bad = np.nonzero(bits(got) != bits(want))[0]
    return f"{len(bad)} of {len(want)} sums differ, first rays {bad[:8].tolist()}" if len(bad) else ""


@pytest.mark.parametrize("which", lc.RAY_SETS)
@pytest.mark.parametrize("L", lc.HW8_LAYERS)
def test_light_pdfs_are_the_oracles_and_the_references_bits(rt, scenes, gold, L, which):
    scene = scenes(L)
    o, d = lc.rays(L, which)
    want, ref = lc.oracle_pdfs(L, which), gold[lc.fixture_key(L, which) + "_pdf"]
    assert np.array_equal(scene.light_order(), oracle_lib.Hw8Oracle(lc.stack_scene(L)).light_order())
    fast, st = scene.query_light_pdf(o, d)
    slow, st_ref = scene.query_light_pdf(o, d, flags=rt.RT_QUERY_REFERENCE_WALK)
    print(f"L = {L}, {which}: {st.rays} rays, {st.exact_walks} exact walks, {st.launches} launches, {st.kernel_ms:.3f} ms; nonzero {(fast != 0).sum()}")
    assert st.reference_exact == 1 and st_ref.reference_exact == 1 and st.rays == len(o) and st.invalid_rays == 0 and st_ref.exact_walks == len(o)
    assert fast.dtype == np.float32
    assert np.array_equal(bits(fast), bits(want)), _differing(fast, want)
    assert np.array_equal(bits(fast), bits(ref)), _differing(fast, ref)
    assert np.array_equal(bits(slow), bits(want)), _differing(slow, want)
    assert np.array_equal(bits(slow), bits(ref)), _differing(slow, ref)


@pytest.mark.parametrize("L", [L for L in lc.HW8_LAYERS if L >= 3])
def test_exact_walks_by_hit_count(rt, scenes, L):
    """The rays of "through" in one call per hit count.  Six or more hits: every ray takes the exact walk (the sixth non-zero term sets
    `overflow`: this follows from the code).  Three to five: at most half of them, so the merge ran and not the exact walk."""
    scene = scenes(L)
    o, d = lc.rays(L, "through")
    want = lc.oracle_pdfs(L, "through")
    k = lc.hit_counts(lc.terms_of(L, "through"))
    for kk in range(L + 1):
        m = k == kk
        assert m.any()
        got, st = scene.query_light_pdf(o[m], d[m])
        print(f"L = {L}, {kk} hits: {st.rays} rays, {st.exact_walks} exact walks")
        assert st.rays == int(m.sum()) and st.reference_exact == 1
        assert np.array_equal(bits(got), bits(want[m])), f"{kk} hits: " + _differing(got, want[m])
        if kk > 5:
            assert st.exact_walks == st.rays, kk
        elif kk >= 3:
            assert 2 * st.exact_walks <= st.rays, kk


@pytest.mark.parametrize("n", [1, 63, 65])
def test_batch_size_changes_no_answer(rt, scenes, n):
    """Partial waves and the slice rounding to 64: the first n rays alone give the first n answers (L = 12, every hit count among them)."""
    scene = scenes(12)
    o, d = lc.rays(12, "through")
    all_pdf, _ = scene.query_light_pdf(o, d)
    assert np.array_equal(bits(all_pdf), bits(lc.oracle_pdfs(12, "through")))
    pdf, st = scene.query_light_pdf(o[:n], d[:n])
    assert st.rays == n and np.array_equal(bits(pdf), bits(all_pdf[:n]))
    tail, _ = scene.query_light_pdf(o[-n:], d[-n:])
    assert np.array_equal(bits(tail), bits(all_pdf[-n:]))


DEVICE_POINTERS = """
import importlib, sys
import numpy as np
import torch
torch.zeros(1, device="cuda")   # torch first, as bench.py has it: one HIP runtime serves both
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
rt = importlib.import_module("raytracing-course-hw_amd")
import light_sum_cases as lc
scene = rt.Scene(lc.stack_scene(12))
o = np.concatenate([lc.rays(12, w)[0] for w in lc.RAY_SETS])
d = np.concatenate([lc.rays(12, w)[1] for w in lc.RAY_SETS])
for flags in (0, rt.RT_QUERY_REFERENCE_WALK):
    pdf, st = scene.query_light_pdf(o, d, flags=flags)
    rays = torch.from_numpy(rt.pack_rays(o, d).view(np.float32).reshape(-1, 6).copy()).cuda()
    out_pdf = torch.full((len(o),), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st_d = scene.query_light_pdf_device(rays.data_ptr(), len(o), out_pdf.data_ptr(), flags=flags)
    assert st_d.rays == len(o) and st_d.exact_walks == st.exact_walks
    assert np.array_equal(out_pdf.cpu().numpy().view(np.uint32), pdf.view(np.uint32))
scene.close()
print("DEVICE POINTERS EQUAL")
"""


def test_device_pointers_give_the_host_calls_bytes():
    """RT_QUERY_DEVICE_POINTERS with torch tensors as rays and output on the three ray sets of L = 12: the host-pointer call's bytes and
    exact-walk count.  In a process of its own, where torch opens the GPU before the library does (the order bench.py keeps)."""
    r = subprocess.run([sys.executable, "-c", DEVICE_POINTERS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE POINTERS EQUAL" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def oracle_frames():
    w, h, spp = lc.FRAME
    return {L: oracle_lib.Hw8Oracle(lc.stack_scene(L)).render(w, h, spp)[:2] for L in lc.FRAME_LAYERS}


@pytest.mark.parametrize("kernel", ["persistent", "wavefront", "mega"])
@pytest.mark.parametrize("L", lc.FRAME_LAYERS)
def test_frames(rt, monkeypatch, gold, oracle_frames, L, kernel):
    """A 32x24x8 frame (24,242 to 34,491 light-pdf queries, every hit count among them).  The persistent kernel (PtLightWalk::end) and the
    round pipeline with its exact kernels on (wf_merge_light_hits, wf_light_exact_kernel) give the oracle's and the reference's pixels,
    floats and bytes, with some but not all light sums through the exact walk once a ray can hit six lights; the megakernel has no gate
    and is held to the tolerance rule of tests/test_gpu_parity_hw8.py."""
    w, h, spp = lc.FRAME
    monkeypatch.setenv("RTAMD_KERNEL", kernel)
    if kernel == "wavefront":
        monkeypatch.setenv("RTAMD_ROUNDS_EXACT", "1")
    ref, ref8 = oracle_frames[L]
    scene = rt.Scene(lc.stack_scene(L))
    try:
        rgb, rgb8, st = scene.render(w, h, spp)
        rgb_c, rgb8_c, st_c = scene.render(w, h, spp, counters=True)
    finally:
        scene.close()
    rmse = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref.astype(np.float64)) ** 2)))
    bad = int((np.abs(rgb - ref).max(axis=2) > 1e-3).sum())
    print(f"L = {L}, {kernel}: rmse {rmse:.3e}, desync pixels {bad}, byte mismatches {(rgb8 != ref8).sum()}, exact {np.array_equal(bits(rgb), bits(ref))}; "
          f"exact light sums {st_c.exact_light_sums} of {st_c.light_pdf_queries} light-pdf queries")
    assert np.array_equal(bits(rgb_c), bits(rgb)) and np.array_equal(rgb8_c, rgb8)       # the counting kernels compute the same frame
    if kernel == "mega":
        assert st.reference_exact == 0 and rmse < RMSE_TOL and bad <= 1 and (rgb8 != ref8).sum() <= 3
        return
    assert st.pipeline == (rt.RT_PIPELINE_PERSISTENT if kernel == "persistent" else rt.RT_PIPELINE_ROUNDS)
    assert st.reference_exact == 1 and st_c.reference_exact == 1
    assert np.array_equal(bits(rgb), bits(ref)) and np.array_equal(rgb8, ref8)
    assert np.array_equal(bits(rgb), bits(gold[f"L{L}_frame_rgb"])) and np.array_equal(rgb8, gold[f"L{L}_frame_rgb8"])
    if L >= 6:
        assert 0 < st_c.exact_light_sums < st_c.light_pdf_queries

"""GPU parity for the hw7 snapshot (hw8's integrator before textures: ungated per-material BRDF, alpha = roughness^2,
geometric normal in the light pdf).  The expected radiance comes from the reference's own hw7 sources
(tests/golden/pins_hw7_render.npz, produced by oracle/ref/ref_hw7_scene.cpp)."""
import os

import numpy as np
import pytest

import pin_cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RMSE_TOL = 1e-3
CASES = {"practice7_1": (lambda: pin_cases.load_hw7("practice7_1"), 48, 48, 8), "practice7_4": (lambda: pin_cases.load_hw7("practice7_4"), 48, 48, 8),
         "sphere_as_hw7": (lambda: pin_cases.as_hw7(pin_cases.load_sphere()), 40, 40, 6),
         "soup_as_hw7": (lambda: pin_cases.as_hw7(pin_cases.random_triangle_scene()), 40, 32, 6)}


@pytest.mark.parametrize("kernel", ["persistent", "wavefront", "mega"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hw7_matches_the_reference_radiance(rt, monkeypatch, name, kernel):
    monkeypatch.setenv("RTAMD_KERNEL", kernel)
    mk, w, h, spp = CASES[name]
    sd = mk()
    scene = rt.Scene(sd)
    rgb, rgb8, _ = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW7)
    gold = np.load(os.path.join(GOLD, "pins_hw7_render.npz"))
    ref, ref8 = gold[name + "_rgb"], gold[name + "_rgb8"]
    rmse = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref) ** 2)))
    nbad = int((rgb.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    print(f"hw7 {name} [{kernel}]: rmse {rmse:.3e}, {nbad} of {w * h} pixels differ in any bit, byte mismatches {(rgb8 != ref8).sum()}")
    assert ref.mean() > 0.01 and rmse < RMSE_TOL and nbad <= (0 if kernel == "persistent" else 2)  # the gated default: the reference's own floats, bit for bit
    if kernel == "persistent": assert np.array_equal(rgb8, ref8)
    scene.close()


def test_hw7_and_hw8_integrators_differ_on_the_same_scene(rt):
    """Sanity: the switch does something (gated vs ungated BRDF, shading vs geometric light normal)."""
    sd = pin_cases.random_triangle_scene()
    scene = rt.Scene(sd)
    a, _, _ = scene.render(40, 32, 6, integrator=rt.RT_INTEGRATOR_HW7, want_rgb8=False)
    b, _, _ = scene.render(40, 32, 6, integrator=rt.RT_INTEGRATOR_HW8, want_rgb8=False)
    assert not np.array_equal(a, b)
    scene.close()


def test_headline_size_frame_against_the_reference_itself(rt, tmp_path):
    """1920x1080x256 on the benchmark scene with its textures stripped, rendered with RT_INTEGRATOR_HW7, against the
    reference's OWN hw7 code on six 32x32 crops: the only place where the GPU meets the reference directly at the headline size.
    The crops are the reference's, stored in tests/golden/pins_reference_crops.npz; where oracle/_ref/libref_hw7.so is built
    they are rendered live as well and must equal the stored ones."""
    import oracle_lib
    sd = pin_cases.synth_room_without_textures(str(tmp_path))
    scene = rt.Scene(sd)
    rgb, _, st = scene.render(1920, 1080, 256, integrator=rt.RT_INTEGRATOR_HW7, want_rgb8=False)
    print(f"hw7 full frame: {st.kernel_ms:.0f} ms = {1920 * 1080 * 256 / st.kernel_ms / 1e3:.1f} Msamples/s")
    gold = np.load(os.path.join(GOLD, "pins_reference_crops.npz"))
    ref7 = oracle_lib.Ref7(sd) if oracle_lib.ref_path("libref_hw7.so") else None
    worst, desync = 0.0, 0
    for (x0, y0) in pin_cases.HW7_HEADLINE_CROPS:
        ref = gold[f"hw7_headline_{x0}_{y0}_rgb"]
        if ref7 is not None:
            live, _, _ = ref7.render(1920, 1080, 256, rect=(x0, y0, 32, 32))
            assert np.array_equal(live, ref), "stored crop differs from the live reference"
        crop = rgb[y0:y0 + 32, x0:x0 + 32]
        rmse = float(np.sqrt(np.mean((crop.astype(np.float64) - ref) ** 2)))
        bad = int((np.abs(crop.astype(np.float64) - ref).max(axis=2) > 1e-3).sum())
        print(f"  crop ({x0},{y0}) vs the reference: rmse {rmse:.3e}, pixels off by > 1e-3: {bad}, bit_exact {np.array_equal(crop, ref)}")
        worst, desync = max(worst, rmse), desync + bad
        assert ref.mean() > 0.01 and np.array_equal(crop, ref)   # against the reference's own compiled integrator, bit for bit
    scene.close()

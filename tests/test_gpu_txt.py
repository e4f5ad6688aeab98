"""GPU parity for the .txt-scene snapshots: hw1 caster (BASELINE.json configs[0]) and hw3 path tracer (configs[1])."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu
TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes", "txt")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ppm(w, h, rgb8):
    return b"P6\n%d %d\n255\n" % (w, h) + rgb8.tobytes()


@pytest.mark.parametrize("name", ["hw1_sample", "hw1_sample_256"])
def test_hw1_caster_is_byte_identical_to_the_reference_program(rt, name):
    """configs[0]: the PPM the GPU path produces must carry the md5 of the reference program's file."""
    sd, w, h, _, _ = rt.load_txt(os.path.join(TXT, name + ".txt"), rt.RT_INTEGRATOR_HW1)
    scene = rt.Scene(sd)
    rgb, rgb8, _ = scene.render(w, h, 1, integrator=rt.RT_INTEGRATOR_HW1)
    gold = np.load(os.path.join(GOLD, "pins_txt_programs.npz"))
    assert hashlib.md5(_ppm(w, h, rgb8)).hexdigest() == bytes(gold[name + "_md5"]).decode()
    ref, ref8 = oracle_lib.TxtOracle(sd).render_hw1(w, h)
    assert np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    scene.close()


@pytest.mark.parametrize("name", ["hw3_practice3_5_64x48x8", "hw3_mixed_materials"])
def test_hw3_matches_oracle_with_per_pixel_seeds(rt, name):
    """Same per-pixel minstd_rand(y*W+x) streams on both sides: checks every arithmetic path (ellipsoid / plane /
    rotated box, diffuse / mirror / dielectric recursion), bit for bit: every function beneath is pinned to the reference at
    its edges (test_gpu_analytic.py), and the frame is the same arithmetic in the same order."""
    sd, w, h, spp, depth = rt.load_txt(os.path.join(TXT, name + ".txt"), rt.RT_INTEGRATOR_HW3)
    scene = rt.Scene(sd)
    rgb, rgb8, _ = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW3, ray_depth=depth)
    ref, ref8 = oracle_lib.TxtOracle(sd).render_hw3(w, h, spp, depth, per_pixel_seed=True)
    rmse = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref) ** 2)))
    print(f"hw3 {name}: rmse {rmse:.3e} bit_exact {np.array_equal(rgb, ref)} byte_mismatch {(rgb8 != ref8).sum()}")
    assert ref.mean() > 0.01 and np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    scene.close()


def test_hw3_statistical_parity_with_the_sequential_reference_stream(rt):
    """The reference's single global engine cannot be replayed in parallel, so parity with IT is statistical
    (SURVEY §8d config 2): against a converged image (sequential-stream oracle, 1024 spp) the GPU's 64-spp image must be
    unbiased and no noisier than the reference-order 64-spp image."""
    sd, _, _, _, depth = rt.load_txt(os.path.join(TXT, "hw3_practice3_5.txt"), rt.RT_INTEGRATOR_HW3)
    w, h = 64, 48
    orc = oracle_lib.TxtOracle(sd)
    converged, _ = orc.render_hw3(w, h, 1024, depth, per_pixel_seed=False)
    cpu64, _ = orc.render_hw3(w, h, 64, depth, per_pixel_seed=False)
    scene = rt.Scene(sd)
    gpu64, _, _ = scene.render(w, h, 64, integrator=rt.RT_INTEGRATOR_HW3, ray_depth=depth)
    rm = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged) ** 2)))
    bias = float(np.mean(gpu64.astype(np.float64) - converged))
    print(f"hw3 statistical: rmse_gpu {rm(gpu64):.4f} rmse_cpu {rm(cpu64):.4f} mean signed error {bias:+.5f} (image mean {converged.mean():.4f})")
    assert rm(gpu64) <= 1.15 * rm(cpu64) + 1e-3
    assert abs(bias) < 0.02 * converged.mean() + 2e-3
    scene.close()


def test_config2_800x600x64_crops(rt):
    """BASELINE.json configs[1] at full size on the GPU; crops against the oracle with the same per-pixel seeds."""
    sd, w, h, spp, depth = rt.load_txt(os.path.join(TXT, "hw3_practice3_5_800x600x64.txt"), rt.RT_INTEGRATOR_HW3)
    assert (w, h, spp, depth) == (800, 600, 64, 6)
    scene = rt.Scene(sd)
    rgb, rgb8, st = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW3, ray_depth=depth)
    print(f"config 2: {st.kernel_ms:.1f} ms kernel = {w * h * spp / st.kernel_ms / 1e3:.1f} Msamples/s")
    orc = oracle_lib.TxtOracle(sd)
    for (x0, y0) in ((380, 280), (40, 500)):
        ref, ref8 = orc.render_hw3(w, h, spp, depth, per_pixel_seed=True, rect=(x0, y0, 48, 32))
        crop = rgb[y0:y0 + 32, x0:x0 + 48]
        rmse = float(np.sqrt(np.mean((crop.astype(np.float64) - ref) ** 2)))
        print(f"  crop ({x0},{y0}): rmse {rmse:.3e} bit_exact {np.array_equal(crop, ref)}")
        assert np.array_equal(crop, ref)
    scene.close()

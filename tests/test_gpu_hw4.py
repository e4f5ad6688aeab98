"""GPU parity for the hw4 snapshot (importance-sampled path tracer over analytic primitives, box / ellipsoid lights)."""
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TXT = os.path.join(GOLD, "scenes", "txt")


@pytest.mark.parametrize("name", pin_cases.HW4_CASES)
def test_hw4_matches_oracle_with_per_pixel_seeds(rt, name):
    """Same per-pixel minstd_rand(y*W+x) streams and per-object normal caches on both sides: cosine / box-light /
    ellipsoid-light sampling, the two-hit light pdf, dielectric recursion.  Bit for bit: every function beneath is pinned to the
    reference at its edges (test_gpu_analytic.py), and the frame is the same arithmetic in the same order."""
    sd, w, h, spp, depth = rt.load_txt(os.path.join(TXT, name + ".txt"), rt.RT_INTEGRATOR_HW4)
    scene = rt.Scene(sd)
    rgb, rgb8, _ = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW4, ray_depth=depth)
    ref, ref8 = oracle_lib.Hw4Oracle(sd).render(w, h, spp, depth, per_pixel_seed=True)
    rmse = float(np.sqrt(np.mean((rgb.astype(np.float64) - ref) ** 2)))
    print(f"hw4 {name}: rmse {rmse:.3e} bit_exact {np.array_equal(rgb, ref)} byte_mismatch {(rgb8 != ref8).sum()}")
    assert ref.mean() > 0.01 and np.array_equal(rgb, ref) and np.array_equal(rgb8, ref8)
    scene.close()


def test_hw4_statistical_parity_with_the_sequential_reference_stream(rt):
    """The reference's single engine cannot be replayed in parallel: against a converged image (sequential-stream oracle,
    2048 spp) the GPU's image must be unbiased and no noisier than the reference-order image at the same spp."""
    name = "hw4_box_and_ellipsoid_lights"
    sd, w, h, spp, depth = rt.load_txt(os.path.join(TXT, name + ".txt"), rt.RT_INTEGRATOR_HW4)
    spp = 64
    orc = oracle_lib.Hw4Oracle(sd)
    converged, _ = orc.render(w, h, 2048, depth, per_pixel_seed=True)
    seq = np.load(os.path.join(GOLD, "pins_hw4_render.npz"))[name + "_rgb"]  # the reference's own stream at the file's 12 spp
    cpu64, _ = orc.render(w, h, spp, depth, per_pixel_seed=False)
    scene = rt.Scene(sd)
    gpu, _, _ = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW4, ray_depth=depth, want_rgb8=False)
    clip = lambda a: np.minimum(a, 4.0)  # fireflies of the light-sampling estimator would dominate an unclipped RMSE
    rm = lambda a: float(np.sqrt(np.mean((clip(a).astype(np.float64) - clip(converged)) ** 2)))
    bias = float(np.mean(clip(gpu).astype(np.float64) - clip(converged)))
    print(f"hw4 statistical: rmse_gpu {rm(gpu):.4f} rmse_cpu {rm(cpu64):.4f} rmse_ref12 {rm(seq):.4f} bias {bias:+.5f} mean {converged.mean():.4f}")
    assert rm(gpu) <= 1.15 * rm(cpu64)
    assert abs(bias) < 0.02 * float(clip(converged).mean()) + 2e-3
    scene.close()

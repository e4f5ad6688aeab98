"""The error budget of the walkers' FMA box test (rt_device.h, the comment above RayGrid), checked on a float32 model of it."""
import numpy as np

import slab_fma_model as M

N_PER_SCENE = 400_000      # four scenes: 1.6 M cases


def _run(margin):
    rng = np.random.default_rng(29)
    lost_total = hits_total = 0
    for scene_lo, scene_hi in M.SCENES:
        cases, grid_box = M.make_cases(scene_lo, scene_hi, N_PER_SCENE, rng)
        real = M.real_test(cases)
        entered, fits, _ = M.grid_test(cases, grid_box, margin=margin)
        lost = real & ~entered
        print(f"margin {margin}: grid over {scene_lo}..{scene_hi}: {int(real.sum())} rays enter the float box, {int(entered.sum())} the grid box, "
              f"{int(lost.sum())} lost, {int((~fits).sum())} misfits")
        assert fits.all()
        lost_total += int(lost.sum()); hits_total += int(real.sum())
        if margin == 1.0:
            assert not lost.any(), cases[lost][:5]
    return lost_total, hits_total


def test_no_box_the_real_ray_enters_is_rejected():
    """1.6 M cases where the FMA form is weakest (slab_fma_model.make_cases: origins at the grid's far corner, direction components from
    the 1e-30 clamp and exact zeros through 1e-6 to 1 with either sign, boxes one cell thick and flat boxes, origins on box faces, the
    scenes of test_gpu_device_math's grid test).  Whenever the ray, in float64 on the float box as it was before it went on the grid,
    enters the box, the model of make_ray_grid + slab_test_q enters the grid box: none lost, no allowance."""
    lost, hits = _run(1.0)
    assert lost == 0
    assert hits > 500_000          # the cases do exercise the test


def test_without_the_extra_cell_the_model_loses_boxes():
    """The same cases with the extra cell of grid_axis_word taken away (bounds only rounded outward to their cells): the rounding of the
    grid-space ray now rejects boxes that the real ray enters — the test above can fail, and what keeps it from failing is that cell."""
    lost, _ = _run(0.0)
    assert lost > 0

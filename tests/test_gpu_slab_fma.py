"""The walkers' box test on the device (rt_device.h make_ray_grid / slab_test_q through the rtt_slab_q hook) against its float32 model
(slab_fma_model), so that what test_slab_fma_budget proves of the model holds of the kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import slab_fma_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_device_decisions_equal_the_models_one_for_one():
    """The cases of test_slab_fma_budget (same generator, same seed): the device enters a grid box exactly when the model does, and
    reports the same unclamped entry distance, bit for bit.  The model is given the device's own reciprocals (v_rcp_f32 is 1 ulp, not
    correctly rounded; the budget covers any 1-ulp reciprocal).  And on the device too no box is lost that the float64 ray enters."""
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_slab_q.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtt_slab_q_entry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    rng = np.random.default_rng(29)
    n = 400_000
    for scene_lo, scene_hi in M.SCENES:
        cases, grid_box = M.make_cases(scene_lo, scene_hi, n, rng)
        out = np.zeros(n, np.uint32)
        assert L.rtt_slab_q(cases.ctypes.data, grid_box.ctypes.data, out.ctypes.data, n) == 0
        rcp, entry = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        assert L.rtt_slab_q_entry(cases.ctypes.data, grid_box.ctypes.data, rcp.ctypes.data, entry.ctypes.data, n) == 0
        entered, fits, tmin = M.grid_test(cases, grid_box, rcp=rcp)
        dev = (out & 2) != 0
        real = M.real_test(cases)
        differ = dev != entered
        t_differ = entry.view(np.uint32) != tmin.view(np.uint32)
        rcp_ulp = np.abs(rcp.view(np.int32).astype(np.int64) - (np.float32(1) / M.clamp_dir(cases[:, 9:12])).astype(np.float32).view(np.int32))
        print(f"grid over {scene_lo}..{scene_hi}: device enters {int(dev.sum())}, model {int(entered.sum())}, decisions that differ {int(differ.sum())}, "
              f"entry distances that differ {int(t_differ.sum())}, lost to the real ray {int((real & ~dev).sum())}, reciprocals off by up to {int(rcp_ulp.max())} ulp")
        assert ((out & 4) != 0).all() and fits.all()
        assert rcp_ulp.max() <= 1
        assert not differ.any(), cases[differ][:5]
        assert not t_differ.any(), cases[t_differ][:5]
        assert not (real & ~dev).any(), cases[real & ~dev][:5]

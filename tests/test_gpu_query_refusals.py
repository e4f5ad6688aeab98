"""What rt_query_closest / rt_query_light_pdf refuse, with the return code and the cause in rt_last_error(): scenes they do not serve
(hw6, .txt), a light pdf without lights, null pointers, unknown flags, a wrong struct_size; and n == 0, which is RT_OK without a launch."""
import ctypes as C
import os

import numpy as np
import pytest

import pin_cases

pytestmark = pytest.mark.gpu

QUERIES = ["rt_query_closest", "rt_query_light_pdf"]


def _stats(rt, struct_size=None):
    st = rt.rt_query_stats()
    st.struct_size = C.sizeof(st) if struct_size is None else struct_size
    return st


def _call(rt, fn, scene, n=4, flags=0, rays=True, out=True, stats=None):
    """One raw call with 4 good rays; returns (code, message)."""
    r = rt.pack_rays(np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, -1], np.float32), (4, 1)))
    o = np.zeros(4 * 16, np.uint32)
    code = getattr(rt.lib, fn)(scene._h if scene is not None else None, r.ctypes.data if rays else None, n, flags,
                               o.ctypes.data if out else None, C.byref(stats) if stats is not None else None)
    return code, rt.lib.rt_last_error().decode()


@pytest.fixture(scope="module")
def sphere(rt):
    s = rt.Scene(pin_cases.load_sphere())
    yield s
    s.close()


@pytest.mark.parametrize("fn", QUERIES)
def test_hw6_and_txt_scenes_are_unsupported(rt, fn):
    hw6 = rt.Scene(pin_cases.load_hw6("practice6_1"))
    sd, *_ = rt.load_txt(os.path.join(pin_cases.SCENES, "txt", "hw1_sample.txt"), rt.RT_INTEGRATOR_HW1)
    txt = rt.Scene(sd)
    try:
        for scene in (hw6, txt):
            code, msg = _call(rt, fn, scene)
            assert code == rt.RT_ERR_UNSUPPORTED and msg.startswith(fn + ": ") and "hw8 / hw7" in msg, (code, msg)
    finally:
        hw6.close()
        txt.close()


def test_light_pdf_needs_lights(rt):
    scene = rt.Scene(rt.load_gltf(os.path.join(pin_cases.SCENES, "hw8_sphere", "sphere.gltf")))
    try:
        assert scene.info().n_lights == 0
        code, msg = _call(rt, "rt_query_light_pdf", scene)
        assert code == rt.RT_ERR_INVALID_ARG and msg.startswith("rt_query_light_pdf: ") and "no lights" in msg, (code, msg)
        code, _ = _call(rt, "rt_query_closest", scene)
        assert code == rt.RT_OK
        with pytest.raises(rt.RtError) as e:
            scene.query_light_pdf(np.zeros((1, 3)), np.ones((1, 3)))
        assert e.value.code == rt.RT_ERR_INVALID_ARG
    finally:
        scene.close()


@pytest.mark.parametrize("fn", QUERIES)
def test_bad_arguments(rt, sphere, fn):
    code, msg = _call(rt, fn, None)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"
    code, msg = _call(rt, fn, sphere, rays=False)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"
    code, msg = _call(rt, fn, sphere, out=False)
    assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": null argument"
    for flags in (4, 8, 0x80000000, 3 | 16):
        code, msg = _call(rt, fn, sphere, flags=flags)
        assert code == rt.RT_ERR_INVALID_ARG and msg.startswith(fn + ": flags other than"), (flags, code, msg)
    for size in (0, C.sizeof(rt.rt_query_stats) - 8, C.sizeof(rt.rt_query_stats) + 8):
        code, msg = _call(rt, fn, sphere, stats=_stats(rt, size))
        assert code == rt.RT_ERR_INVALID_ARG and msg == fn + ": struct_size mismatch (ABI skew)", (size, code, msg)
    st = _stats(rt)
    code, _ = _call(rt, fn, sphere, stats=st)
    assert code == rt.RT_OK and st.rays == 4 and st.launches > 0


@pytest.mark.parametrize("fn", QUERIES)
def test_no_rays_is_ok_without_a_launch(rt, sphere, fn):
    st = _stats(rt)
    code, _ = _call(rt, fn, sphere, n=0, rays=False, out=False, stats=st)
    assert code == rt.RT_OK
    assert (st.rays, st.exact_walks, st.invalid_rays, st.launches, st.kernel_ms) == (0, 0, 0, 0, 0.0)
    assert st.reference_exact == 1
    hits, st = sphere.query_closest(np.zeros((0, 3)), np.zeros((0, 3)))
    assert hits.shape == (0,) and st.launches == 0


def test_unaligned_device_output_is_refused(rt, sphere):
    code, msg = rt.lib.rt_query_closest(sphere._h, 256, 1, rt.RT_QUERY_DEVICE_POINTERS, 260, None), rt.lib.rt_last_error().decode()
    assert code == rt.RT_ERR_INVALID_ARG and "16-byte aligned" in msg

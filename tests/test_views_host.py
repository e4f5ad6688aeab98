"""View sets, the part that needs no GPU: the header declares rt_views_* under ABI 6 with the binding's struct sizes and the library
exports them; the camera check (csrc/host/rt_views_camera.h, through the test hook rtt_views_camera_check) rejects non-finite and
oversized components, fov_y outside (0, 3] and dependent vectors, and accepts the six cameras of tests/view_cases.py; and every entry
point refuses null arguments and a wrong struct_size before it looks at a scene or a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surface_cases as sc
import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"rt_views_create", "rt_views_set_cameras", "rt_views_render", "rt_views_samples", "rt_views_resolve", "rt_views_destroy"}


@pytest.fixture(scope="module")
def check(rt):
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_views_camera_check.argtypes = [C.POINTER(rt.rt_camera), C.c_char_p, C.c_size_t]

    def run(cam):
        why = C.create_string_buffer(256)
        return L.rtt_views_camera_check(C.byref(cam) if cam is not None else None, why, 256), why.value.decode()
    return run


def test_header_declares_the_family_under_abi_6(rt):
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert re.search(r"^#define RTAMD_ABI_VERSION 6$", text, re.M)
    assert set(re.findall(r"^(?:int|void)\s+(rt_views_[a-z_]+)\(", text, re.M)) == WANT
    for name in WANT:
        assert name in rt.ABI_SYMBOLS and hasattr(rt.lib, name), name
    for words in ("checkpoints of a view set", "rt_noise, rt_denoise, guide images and rt_camera_rays", "rt_multi_*", "hw7 and hw6",
                  "adaptive sampling per view", "views of different sizes"):
        assert words in text, words                              # what is out of scope is said


def test_struct_sizes_equal_the_headers(rt):
    """The header's layout, worked out by hand (the .hip has the same static_assert): params 4 + 2*4 + 4 + 4 + 4 + 8 + 2*4, stats
    2*4 + 8 + 2*4 + 4*8 + 2*4 + 8; and field by field against the header's text."""
    assert C.sizeof(rt.rt_views_params) == 40 and C.sizeof(rt.rt_views_stats) == 72
    source = open(os.path.join(ROOT, "raytracing-course-hw_amd", "csrc", "rtamd_views.hip")).read()
    assert "static_assert(sizeof(rt_views_params) == 40 && sizeof(rt_views_stats) == 72" in source
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    for struct in (rt.rt_views_params, rt.rt_views_stats):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *").split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in struct._fields_], names
    assert rt.rt_views_params.stream.offset == 24 and rt.rt_views_stats.kernel_ms.offset == 24 and rt.rt_views_stats.exact_walks.offset == 64


def test_camera_check_accepts_the_table(rt, check):
    for scene in ("soup_a", "sphere_emissive_env"):
        for name, cam in vc.table(sc.scene_data(scene)).items():
            assert check(cam) == (0, ""), (scene, name)
    cam = vc.table(sc.scene_data("soup_a"))["inside"]
    cam.fov_x = float("nan")                                     # ignored
    assert check(cam) == (0, "")
    cam.fov_y = 3.0                                              # the interval is closed above
    assert check(cam) == (0, "")
    cam.position[0] = 2.0 ** 40                                  # and so is the bound on a component
    assert check(cam) == (0, "")


def test_camera_check_rejects(rt, check):
    bad = rt.RT_ERR_INVALID_ARG
    base = lambda: vc.table(sc.scene_data("soup_a"))["inside"]
    assert check(None)[0] == bad
    for field in ("position", "right", "up", "forward"):
        for k in range(3):
            for value in (float("nan"), float("inf"), -float("inf"), 2.0 ** 41, -2.0 ** 41, float(np.nextafter(np.float32(2.0 ** 40), np.float32(np.inf)))):
                cam = base()
                getattr(cam, field)[k] = value
                code, why = check(cam)
                assert code == bad and why.startswith("%s[%d]" % (field, k)), (field, k, value, why)
    for fov in (0.0, -0.5, 3.1, float(np.nextafter(np.float32(3.0), np.float32(4.0))), float("nan"), float("inf")):
        cam = base()
        cam.fov_y = fov
        code, why = check(cam)
        assert code == bad and why.startswith("fov_y"), (fov, why)
    coplanar = vc.camera((0, 0, 6), (1, 0, 0), (0, 1, 0), (1, 1, 0), 0.7)
    parallel = vc.camera((0, 0, 6), (1, 0, 0), (0, 1, 0), (0, 2, 0), 0.7)
    zero = vc.camera((0, 0, 6), (1, 0, 0), (0, 0, 0), (0, 0, -1), 0.7)
    nearly = vc.camera((0, 0, 6), (1, 0, 0), (0, 1, 0), (1, 1, 1e-7), 0.7)      # determinant 1e-7 against lengths of about 1.4
    big = vc.camera((0, 0, 6), (1e12, 0, 0), (0, 1e12, 0), (1e12, 1e12, 0), 0.7)  # relative, not absolute
    for cam in (coplanar, parallel, zero, nearly, big):
        code, why = check(cam)
        assert code == bad and "linearly independent" in why, why
    small = vc.camera((0, 0, 6), (1e-12, 0, 0), (0, 1e-12, 0), (0, 0, -1e-12), 0.7)  # tiny but independent: relative again
    assert check(small) == (0, "")


def test_null_arguments_and_struct_sizes(rt):
    bad = rt.RT_ERR_INVALID_ARG
    err = lambda: rt.lib.rt_last_error().decode()
    cams = (rt.rt_camera * 2)()
    p, out = rt.make_views_params(8, 8, 2), C.c_void_p(0x5a5a)
    fake = C.c_void_p(0x1000)                                    # never looked at: the refusal comes first
    for scene, pp, cc, oo in ((None, C.byref(p), cams, C.byref(out)), (fake, None, cams, C.byref(out)), (fake, C.byref(p), None, C.byref(out)),
                              (fake, C.byref(p), cams, None)):
        assert rt.lib.rt_views_create(scene, pp, C.cast(cc, C.c_void_p) if cc is not None else None, oo) == bad and err() == "rt_views_create: null argument"
    for size in (0, 36, C.sizeof(rt.rt_render_params)):
        p.struct_size = size
        assert rt.lib.rt_views_create(None, C.byref(p), C.cast(cams, C.c_void_p), C.byref(out)) == bad
        assert err() == "rt_views_create: params.struct_size mismatch (ABI skew)"
    assert out.value == 0x5a5a                                   # a refusal for a null argument writes nothing
    st = rt.rt_views_stats()
    st.struct_size = C.sizeof(st)
    buf = np.zeros(64, np.uint8)
    assert rt.lib.rt_views_render(None, 4, None, C.byref(st)) == bad and err() == "rt_views_render: null argument"
    assert rt.lib.rt_views_render(None, 4, buf.ctypes.data, None) == bad and err() == "rt_views_render: null argument"
    for size in (0, C.sizeof(st) - 8, C.sizeof(rt.rt_adaptive_stats)):
        st.struct_size = size
        assert rt.lib.rt_views_render(None, 4, None, C.byref(st)) == bad and err() == "rt_views_render: stats.struct_size mismatch (ABI skew)"
    assert rt.lib.rt_views_set_cameras(None, 0, 1, C.cast(cams, C.c_void_p)) == bad and err() == "rt_views_set_cameras: null argument"
    assert rt.lib.rt_views_samples(None, buf.ctypes.data) == bad and err() == "rt_views_samples: null argument"
    assert rt.lib.rt_views_resolve(None, 0, 0, None, None) == bad and err() == "rt_views_resolve: null argument"
    rt.lib.rt_views_destroy(None)                                # like free(NULL)

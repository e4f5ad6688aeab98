"""Every array and scalar that the host-side scene preparation (csrc/host/scene_prep.cpp) decides, pinned without a GPU.

The hook rtt_prepared_digest (csrc/test_hooks.hip) runs the preparation of one flavour and answers one line per member of the
prepared struct, `name element_count fnv1a64-of-the-raw-bytes` (a scalar: `name 1 its-bits-in-hex`).  tests/golden/prepared_digests.txt
is this module's output (python tests/test_prepared_host.py FILE) with the library as it was BEFORE scene_prep.cpp was brought to one
triangle stage, one tree result and one base struct; the test compares line by line, so every byte of every prepared array stays.
Recorded twice there, the two recordings were equal: no record type has bytes that the preparation leaves undefined, so whole records
are hashed.  The `txt.*` members (the .txt primitives, lights and light-primitive list) were prepared inside rt_scene_create then; their
lines were recorded from those same loops, lifted verbatim into a prepare_scene_txt for the recording.

The preparation's own refusals follow, through rt_host_prepare_orders: `name, return code, rt_last_error()`."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prepared_digests.txt")
TXT = os.path.join(ROOT, "tests", "golden", "scenes", "txt")


def _one_triangle(rt):
    import pin_cases
    sd = pin_cases.random_triangle_scene(n=40, seed=5)
    return rt.SceneData(sd.positions[:1], sd.texcoords[:1], sd.normals[:1], sd.tangents[:1], sd.material_index[:1],
                        list(sd.materials)[:sd.n_materials], camera=sd.camera)


def _cases(rt):
    """(name, make the SceneData, integrator, the tree_on_device values, environment)"""
    import pin_cases
    soup = pin_cases.random_triangle_scene
    hw8, hw7, hw6, hw5 = rt.RT_INTEGRATOR_HW8, rt.RT_INTEGRATOR_HW7, rt.RT_INTEGRATOR_HW6, rt.RT_INTEGRATOR_HW5
    txt = lambda name, flavor: (lambda: rt.load_txt(os.path.join(TXT, name + ".txt"), flavor)[0])
    yield "hw8.sphere_emissive", pin_cases.load_sphere, hw8, (0, 1), {}
    yield "hw7.practice7_4", lambda: pin_cases.load_hw7("practice7_4"), hw7, (0, 1), {}
    yield "hw8.soup_40", lambda: soup(n=40, seed=5, n_emissive_mats=2), hw8, (0, 1), {}
    yield "hw8.soup_700", lambda: soup(n=700, seed=11), hw8, (0, 1), {}
    yield "hw8.soup_40000", lambda: soup(n=40000, seed=12, n_emissive_mats=3), hw8, (0, 1), {}  # beyond the 16,384 fork; has tripwires
    yield "hw8.one_triangle", lambda: _one_triangle(rt), hw8, (0, 1), {}
    yield "hw8.no_emissive", lambda: soup(n=40, seed=5, n_emissive_mats=0), hw8, (0, 1), {}
    yield "hw8.soup_700_knobs", lambda: soup(n=700, seed=11), hw8, (0, 1), {"RTAMD_BOX_PAD_SCALE": "2", "RTAMD_TRIPWIRE_COS": "1e-3"}
    # the 700-triangle soup has no tripwire under either threshold; this one has 6 at the default and more at 1e-3, which pins the knob
    yield "hw8.soup_40000_tripwire_cos", lambda: soup(n=40000, seed=12, n_emissive_mats=3), hw8, (0,), {"RTAMD_TRIPWIRE_COS": "1e-3"}
    for name, (make, _, _, _) in pin_cases.HW6_CASES.items():
        yield "hw6." + name, make, hw6, (0, 1), {}
    yield "hw6.soup_700_knobs", lambda: pin_cases.hw6_soup(n=700, seed=11), hw6, (0, 1), {"RTAMD_BOX_PAD_SCALE": "2"}
    yield "hw5.hw5_mixed_figures", txt("hw5_mixed_figures", hw5), hw5, (0,), {}
    yield "hw5.hw3_practice3_5", txt("hw3_practice3_5", rt.RT_INTEGRATOR_HW3), hw5, (0,), {}                      # no triangles
    yield "hw5.hw2_sample", txt("hw2_sample", rt.RT_INTEGRATOR_HW2), hw5, (0,), {}                                # point and directional lights
    yield "hw5.hw4_box_and_ellipsoid_lights", txt("hw4_box_and_ellipsoid_lights", rt.RT_INTEGRATOR_HW4), hw5, (0,), {}  # light primitives


def _digest(hooks, sd, integrator, tree_on_device):
    buf = C.create_string_buffer(8192)
    n = hooks.rtt_prepared_digest(C.byref(sd.desc), integrator, tree_on_device, buf, len(buf))
    assert 0 < n < len(buf), n
    return buf.value.decode().splitlines()


def _refusals(rt):
    """The scenes the preparation refuses, each with the integrator it is prepared for."""
    import pin_cases
    def changed(sd, **fields):
        d = rt.rt_scene_desc.from_buffer_copy(sd.desc)   # the arrays stay owned by `sd`
        for k, v in fields.items():
            setattr(d, k, v)
        return sd, d
    def soup_with(change):
        sd = pin_cases.random_triangle_scene(n=40, seed=5)
        change(sd)
        sd._build_desc()
        return sd, sd.desc
    def material_index(sd): sd.material_index[7] = sd.n_materials
    def texture_index(sd): sd.materials[2].normal_texture = 1
    def texture_source(sd): sd.materials[2].emissive_texture, sd.texture_source = 0, np.array([1], np.uint32)
    def image_without_pixels(sd): sd.images = [np.zeros((0, 4, 3), np.uint8)]
    soup, soup6 = pin_cases.random_triangle_scene(n=40, seed=5), pin_cases.hw6_soup(n=40, seed=5)
    hw8, hw6, hw5 = rt.RT_INTEGRATOR_HW8, rt.RT_INTEGRATOR_HW6, rt.RT_INTEGRATOR_HW5
    yield "hw8.too_many_triangles", changed(soup, n_triangles=0x00FFFFFF), hw8   # refused before any array is read
    yield "hw6.too_many_triangles", changed(soup6, n_triangles=0x7FFFFFFF), hw6
    yield "hw8.no_positions", changed(soup, positions=None), hw8
    yield "hw6.no_positions", changed(soup6, positions=None), hw6
    yield "hw8.material_index", soup_with(material_index), hw8
    yield "hw6.material_index", changed(soup6, n_materials=int(soup6.material_index.max())), hw6
    yield "hw8.texture_index", soup_with(texture_index), hw8
    yield "hw8.texture_source", soup_with(texture_source), hw8
    yield "hw8.image_without_pixels", soup_with(image_without_pixels), hw8
    sd5 = rt.load_txt(os.path.join(TXT, "hw5_mixed_figures.txt"), hw5)[0]
    sd5.primitives[3].type = 9
    sd5._build_desc()
    yield "hw5.bad_primitive_type", (sd5, sd5.desc), hw5


def run(rt):
    hooks = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    hooks.rtt_prepared_digest.argtypes = [C.POINTER(rt.rt_scene_desc), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    lines = []
    for name, make, integrator, trees, env in _cases(rt):
        sd = make()
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)  # putenv: the library reads its knobs at every call
        try:
            for tree_on_device in trees:
                lines.append(f"[{name} tree_on_device={tree_on_device}]")
                lines += _digest(hooks, sd, integrator, tree_on_device)
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    lines.append("[refusals]")
    out = np.zeros(64, np.uint32)
    for name, (keep, desc), integrator in _refusals(rt):
        rc = rt.lib.rt_host_prepare_orders(C.byref(desc), integrator, out.ctypes.data, 64, out.ctypes.data, 64)
        lines.append(f"{name}, {rc}, " + rt.lib.rt_last_error().decode("utf-8", "replace"))
    return lines


def test_prepared_arrays_and_refusals_equal_the_parents(rt):
    got, want = run(rt), open(GOLDEN).read().splitlines()
    assert len(got) == len(want)
    section = ""
    for g, w in zip(got, want):
        section = g if g.startswith("[") else section
        assert g == w, section
    # the tripwire builder cannot drop out of the pin unnoticed: 6 tripwires in 4 groups (of 2, 1, 2 and 1 members)
    at = got.index("[hw8.soup_40000 tree_on_device=0]")
    members = dict(line.split(" ", 1) for line in got[at + 1:got.index("[hw8.soup_40000 tree_on_device=1]")])
    assert int(members["n_tripwire_groups"].split()[1], 16) == 4
    assert int(members["tripwires"].split()[0]) == (4 + 6) * 8
    at = got.index("[hw8.soup_40000_tripwire_cos tree_on_device=0]")
    knob = dict(line.split(" ", 1) for line in got[at + 1:at + 10])
    assert int(knob["tripwires"].split()[0]) > (4 + 6) * 8 and knob["tripwires"] != members["tripwires"]
    assert all(rc < 0 for rc in (int(line.split(", ")[1]) for line in got[got.index("[refusals]") + 1:]))


if __name__ == "__main__":  # python tests/test_prepared_host.py FILE: writes the transcript
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    lines = run(importlib.import_module("raytracing-course-hw_amd"))
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {sys.argv[1]}")

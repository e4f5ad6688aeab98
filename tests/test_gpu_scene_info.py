"""What scene creation leaves behind, pinned per branch of rt_scene_create against values recorded from the library before the
C-ABI source was split (tests/golden/scene_info_parent.json, recorded twice on an MI355X with RTAMD_LIB pointing at that build:
`python tests/test_gpu_scene_info.py out.json`; the two recordings agree in every field, so none is left out).

Per case: the integer fields of rt_scene_info and the light order; then a 32x24 frame at 4 spp with RT_FLAG_COUNTERS on every
pipeline the scene can take: the query counts, the exact-walk counts, rt_stats.pipeline / reference_exact and the frame's bytes
(as SHA-256 of the float and the 8-bit buffer).  node_visits and triangle_tests vary from run to run (which wave picks up which
ray) and are not compared."""
import hashlib
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_info_parent.json")
W, H, SPP = 32, 24, 4
INFO_FIELDS = ["n_triangles", "n_lights", "n_bvh_nodes", "n_light_bvh_nodes", "bvh_depth", "light_bvh_depth", "device_bytes",
               "bvh_on_device", "reserved"]
STAT_FIELDS = ["closest_hit_queries", "light_pdf_queries", "exact_closest_hits", "exact_light_sums", "pipeline", "reference_exact"]
HW8_PIPELINES = {"persistent": None, "wavefront": "wavefront", "mega": "mega"}  # RTAMD_KERNEL
HW8_BUILDS = ["default", "host_trees", "device_bvh"]
# hw8 scenes (pin_cases.random_triangle_scene): fewer than 64 triangles (the walkers use the reference topology); at least 64
# triangles but fewer than 64 lights (a walk tree of the library's own, the reference's light tree); at least 64 lights (both own)
HW8_SOUPS = {"hw8_40_tris": dict(n=40, seed=5, n_emissive_mats=2), "hw8_200_tris": dict(n=200, seed=5, n_emissive_mats=1),
             "hw8_600_tris_219_lights": dict(n=600, seed=3, n_emissive_mats=2)}
CASES = ["txt", "hw6_practice6_1"] + [f"{s}-{b}" for s in HW8_SOUPS for b in HW8_BUILDS]


def _record(case):
    """Creates the scene of `case` and renders it on its pipelines; the environment is restored on the way out."""
    import pin_cases
    rt = pin_cases.rt
    knobs = ["RTAMD_HOST_BVH", "RTAMD_HOST_LIGHT_BVH", "RTAMD_KERNEL"]
    saved = {k: os.environ.pop(k, None) for k in knobs}
    try:
        flags, pipelines = 0, {"default": None}
        if case == "txt":
            sd, integrator = rt.load_txt(os.path.join(pin_cases.SCENES, "txt", "hw3_practice3_5_64x48x8.txt"))[0], rt.RT_INTEGRATOR_HW3
        elif case == "hw6_practice6_1":
            sd, integrator, pipelines = pin_cases.load_hw6("practice6_1"), rt.RT_INTEGRATOR_HW6, {"persistent": None, "mega": "mega"}
        else:
            soup, build = case.split("-")
            sd, integrator, pipelines = pin_cases.random_triangle_scene(**HW8_SOUPS[soup]), rt.RT_INTEGRATOR_HW8, HW8_PIPELINES
            if build == "host_trees":
                os.environ["RTAMD_HOST_BVH"] = os.environ["RTAMD_HOST_LIGHT_BVH"] = "1"
            flags = rt.RT_BUILD_DEVICE_BVH if build == "device_bvh" else 0
        scene = rt.Scene(sd, build_flags=flags)
        info = scene.info()
        out = {"info": {f: int(getattr(info, f)) for f in INFO_FIELDS}, "light_order": [int(v) for v in scene.light_order()], "renders": {}}
        for name, kernel in pipelines.items():
            if kernel:
                os.environ["RTAMD_KERNEL"] = kernel
            rgb, rgb8, st = scene.render(W, H, SPP, integrator=integrator, counters=True)
            os.environ.pop("RTAMD_KERNEL", None)
            r = {f: int(getattr(st, f)) for f in STAT_FIELDS}
            r["rgb_sha256"], r["rgb8_sha256"] = hashlib.sha256(rgb.tobytes()).hexdigest(), hashlib.sha256(rgb8.tobytes()).hexdigest()
            out["renders"][name] = r
        scene.close()
        return out
    finally:
        for k in knobs:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_scene_info_and_counting_frame_as_before_the_split(golden, case):
    got, want = _record(case), golden[case]
    print(case, json.dumps(got["info"]), {k: (v["closest_hit_queries"], v["light_pdf_queries"]) for k, v in got["renders"].items()})
    assert got["info"] == want["info"]
    assert got["light_order"] == want["light_order"]
    assert sorted(got["renders"]) == sorted(want["renders"])
    for name in want["renders"]:
        assert got["renders"][name] == want["renders"][name], name
    # the cases reach the branches they are meant to
    soup, _, build = case.partition("-")
    if soup in HW8_SOUPS:
        assert got["info"]["bvh_on_device"] == (0 if soup == "hw8_40_tris" or build == "host_trees" else 1)
        assert (got["info"]["n_lights"] >= 64) == (soup == "hw8_600_tris_219_lights")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    with open(sys.argv[1], "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(f" {json.dumps(c)}: {json.dumps(_record(c), sort_keys=True)}" for c in sorted(CASES)) + "\n}\n")

"""Regenerates tests/golden/pins_*.npz from the compiled reference (oracle/_ref, built where the reference's sources are).
Run:  python tests/golden/make_goldens.py      (after `make -C oracle`)
      python tests/golden/make_goldens.py orders      only pins_oracle_orders.npz, which comes from the oracle itself
      python tests/golden/make_goldens.py shading     only pins_shading_edges.npz
      python tests/golden/make_goldens.py intersection     only pins_intersection_edges.npz
      python tests/golden/make_goldens.py analytic     only pins_analytic_edges.npz
      python tests/golden/make_goldens.py texture     only pins_texture_edges.npz and pins_hw8_paths.npz
      python tests/golden/make_goldens.py light_sums     only pins_light_sums.npz"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
import pin_cases  # noqa: E402


def main():
    L8 = C.CDLL(oracle_lib.ref_path("libref_hw8.so"))
    L8.ref8_brdf.argtypes = [C.c_float] + [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
    L8.ref8_tonemap.argtypes = [C.c_void_p, C.c_void_p]
    # per-function pins through the reference's hw8 headers + primitives.cpp + color.cpp
    for name, sd, seed in (("sphere", pin_cases.load_sphere(), 11), ("soup", pin_cases.random_triangle_scene(), 23)):
        out = pin_cases.eval_functions(oracle_lib.Ref8(sd), sd, seed)
        np.savez_compressed(os.path.join(HERE, f"pins_hw8_functions_{name}.npz"), **out)
        print(name, {k: v.shape for k, v in out.items()})
    save_function_inputs()
    bi = pin_cases.brdf_inputs()
    br = np.stack([oracle_lib.brdf(L8, "ref8_", float(bi["base_metallic"][i]), bi["base_color"][i], bi["l"][i], bi["v"][i], bi["n"][i],
                                   bi["color"][i], float(bi["metallic"][i]), float(bi["alpha"][i])) for i in range(len(bi["alpha"]))])
    ti = pin_cases.tonemap_inputs()
    tm = np.stack([oracle_lib.tonemap(L8, "ref8_tonemap", ti[i]) for i in range(len(ti))])
    np.savez_compressed(os.path.join(HERE, "pins_hw8_brdf_tonemap.npz"), brdf=br, tonemap=tm)
    # whole-integrator pins through the reference's hw7 scene.cpp (Scene::getPixel)
    cases = {"practice7_1": (pin_cases.load_hw7("practice7_1"), 48, 48, 8), "practice7_4": (pin_cases.load_hw7("practice7_4"), 48, 48, 8),
             "sphere_as_hw7": (pin_cases.as_hw7(pin_cases.load_sphere()), 40, 40, 6), "soup_as_hw7": (pin_cases.as_hw7(pin_cases.random_triangle_scene()), 40, 32, 6)}
    out = {}
    for name, (sd, w, h, spp) in cases.items():
        rgb, rgb8, _ = oracle_lib.Ref7(sd).render(w, h, spp)
        out[name + "_rgb"], out[name + "_rgb8"] = rgb, rgb8
        print(name, rgb.shape, float(rgb.mean()))
    np.savez_compressed(os.path.join(HERE, "pins_hw7_render.npz"), **out)
    # whole-integrator pins through the reference's hw6 scene.cpp (dielectric recursion, Mix{Cosine, lights})
    out = {}
    for name, (mk, w, h, spp) in pin_cases.HW6_CASES.items():
        rgb, rgb8, _ = oracle_lib.Ref6(mk()).render(w, h, spp)
        out[name + "_rgb"], out[name + "_rgb8"] = rgb, rgb8
        print(name, rgb.shape, float(rgb.mean()))
    np.savez_compressed(os.path.join(HERE, "pins_hw6_render.npz"), **out)
    # loader arithmetic through the reference's own transition.h (node chains, inverse-transpose normals, tangents)
    import tempfile as _tf
    with _tf.TemporaryDirectory() as td:
        _, lc = pin_cases.loader_case(td)
    L8.ref8_transform_chain.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    out = {}
    n = lc["pos"].shape[0]
    for tag, levels, chain, matrix in (("chain", 3, lc["chain"], None), ("matrix", 1, np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1], np.float32), lc["matrix"])):
        op, on, ot = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        ch = np.ascontiguousarray(chain, np.float32)
        L8.ref8_transform_chain(levels, ch.ctypes.data, matrix.ctypes.data if matrix is not None else None, n, lc["pos"].ctypes.data,
                                lc["nrm"].ctypes.data, lc["tan"].ctypes.data, op.ctypes.data, on.ctypes.data, ot.ctypes.data)
        out[tag + "_pos"], out[tag + "_nrm"], out[tag + "_tan"] = op, on, ot
    np.savez_compressed(os.path.join(HERE, "pins_loader_transforms.npz"), **out)
    print("loader transforms", {k: v.shape for k, v in out.items()})
    # byte-level pins through the reference's own unmodified CLI programs (hw1, hw3)
    import hashlib
    import subprocess
    import tempfile
    txt = os.path.join(HERE, "scenes", "txt")
    out = {}
    for name, prog in (("hw1_sample", "hw1_main"), ("hw1_sample_256", "hw1_main"), ("hw3_practice3_5_64x48x8", "hw3_main"), ("hw3_mixed_materials", "hw3_main")):
        with tempfile.TemporaryDirectory() as td:
            ppm = os.path.join(td, "o.ppm")
            subprocess.run([oracle_lib.ref_path(prog), os.path.join(txt, name + ".txt"), ppm], check=True, stderr=subprocess.DEVNULL)
            data = open(ppm, "rb").read()
        out[name + "_md5"] = np.frombuffer(hashlib.md5(data).hexdigest().encode(), np.uint8)
        if len(data) < 100000:
            out[name + "_ppm"] = np.frombuffer(data, np.uint8)
        print(name, hashlib.md5(data).hexdigest(), len(data))
    np.savez_compressed(os.path.join(HERE, "pins_txt_programs.npz"), **out)
    # hw2: float radiance through the reference's own loader + Scene::getPixel, and the program's PPM md5
    out = {}
    for name in pin_cases.HW2_CASES:
        path = os.path.join(txt, name + ".txt")
        out[name + "_rgb"] = oracle_lib.RefTxt(2, path).render()
        with tempfile.TemporaryDirectory() as td:
            ppm = os.path.join(td, "o.ppm")
            subprocess.run([oracle_lib.ref_path("hw2_main"), path, ppm], check=True, stderr=subprocess.DEVNULL)
            out[name + "_md5"] = np.frombuffer(hashlib.md5(open(ppm, "rb").read()).hexdigest().encode(), np.uint8)
        print(name, out[name + "_rgb"].shape, float(out[name + "_rgb"].mean()), bytes(out[name + "_md5"]).decode())
    with tempfile.TemporaryDirectory() as td:
        ppm = os.path.join(td, "o.ppm")
        subprocess.run([oracle_lib.ref_path("hw2_main"), os.path.join(txt, "hw2_sample.txt"), ppm], check=True, stderr=subprocess.DEVNULL)
        out["hw2_sample_md5"] = np.frombuffer(hashlib.md5(open(ppm, "rb").read()).hexdigest().encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "pins_hw2_render.npz"), **out)
    # hw4: float radiance of the reference's sequential stream (fresh process per scene: the engine is a file-static)
    out = {}
    for name in pin_cases.HW4_CASES:
        out[name + "_rgb"] = oracle_lib.ref_txt_render_fresh(4, os.path.join(txt, name + ".txt"))
        print(name, out[name + "_rgb"].shape, float(out[name + "_rgb"].mean()))
    np.savez_compressed(os.path.join(HERE, "pins_hw4_render.npz"), **out)
    # hw5: float radiance through the reference's own loader + Scene::getPixel(rng(y*W+x)), and the program's PPM md5
    out = {}
    for name in pin_cases.HW5_CASES:
        path = os.path.join(txt, name + ".txt")
        out[name + "_rgb"] = oracle_lib.RefTxt(5, path).render()
        with tempfile.TemporaryDirectory() as td:
            ppm = os.path.join(td, "o.ppm")
            subprocess.run([oracle_lib.ref_path("hw5_main"), path, ppm], check=True, stderr=subprocess.DEVNULL)
            out[name + "_md5"] = np.frombuffer(hashlib.md5(open(ppm, "rb").read()).hexdigest().encode(), np.uint8)
        print(name, out[name + "_rgb"].shape, float(out[name + "_rgb"].mean()), bytes(out[name + "_md5"]).decode())
    np.savez_compressed(os.path.join(HERE, "pins_hw5_render.npz"), **out)
    save_reference_crops()
    save_env_uv()
    save_shading_edges()
    save_intersection_edges()
    save_analytic_edges()
    save_texture_edges()
    save_hw8_paths()
    save_light_sums()


def save_light_sums():
    """Light-pdf sums by hit count (tests/light_sum_cases.py): the compiled reference's FiguresMix::pdf (Ref8.light_pdf) on every hw8 stack
    scene and ray set, with the rays, and the reference's own pixels (hw8 scene.cpp, Ref8Scene) of the frames the GPU tests render."""
    import light_sum_cases as lc
    out = {}
    for L in lc.HW8_LAYERS:
        sd = lc.stack_scene(L)
        ref = oracle_lib.Ref8(sd)
        for which in lc.RAY_SETS:
            o, d = lc.rays(L, which)
            key = lc.fixture_key(L, which)
            out[key + "_o"], out[key + "_d"], out[key + "_pdf"] = o, d, lc.light_pdfs(ref, o, d)
        if L in lc.FRAME_LAYERS:
            w, h, spp = lc.FRAME
            out[f"L{L}_frame_rgb"], out[f"L{L}_frame_rgb8"], _ = oracle_lib.Ref8Scene(sd).render(w, h, spp)
            print("light sums frame", L, float(out[f"L{L}_frame_rgb"].mean()))
    np.savez_compressed(os.path.join(HERE, "pins_light_sums.npz"), **out)
    print("light sums", {k: v.shape for k, v in out.items()})


def save_texture_edges():
    """The texture layer at its edges (tests/texture_cases.py) through the static sampleTexture and applyNormalMaps of the reference's own
    hw8 scene.cpp, and the reference's taps at the camera set's hits on the scene texture_edges.  Outputs only, but for the texcoords of those
    hits, which say which question each of those taps answers."""
    import texture_cases
    out = texture_cases.evaluate("reference")
    hits = texture_cases.edge_hits()
    out["edge_hit_uv"] = np.ascontiguousarray(hits["texcoord"]).view(np.uint32)
    out["edge_hit_taps"] = texture_cases.edge_taps(texture_cases.ref_scene_lib().ref8_sample_texture, hits)
    np.savez_compressed(os.path.join(HERE, "pins_texture_edges.npz"), **out)
    print("texture edges", {k: v.shape for k, v in out.items()})


def save_hw8_paths():
    """Float radiance of the reference's own hw8 Scene::getPixel (scene.cpp with its textures, normal maps and environment map) on the
    scenes of tests/test_texture_pins.py PATH_CASES."""
    import surface_cases
    import test_texture_pins
    out = {}
    for key, (name, depth) in test_texture_pins.PATH_CASES.items():
        out[key], _, _ = oracle_lib.Ref8Scene(surface_cases.scene_data(name)).render(*test_texture_pins.FRAME, ray_depth=depth)
        print(key, out[key].shape, float(np.nanmean(out[key])))
    np.savez_compressed(os.path.join(HERE, "pins_hw8_paths.npz"), **out)


def save_analytic_edges():
    """The analytic figures, the light pdf and the samplers of hw1 .. hw5 at their branch points (tests/analytic_cases.py) through each
    snapshot's own Figure::intersect, root function, FigureLight::pdf and sample().  Outputs only: the inputs are the case table's."""
    import analytic_cases
    out = analytic_cases.evaluate("reference")
    np.savez_compressed(os.path.join(HERE, "pins_analytic_edges.npz"), **{k: out[k] for k in analytic_cases.FAMILIES})
    print("analytic edges", {k: v.shape for k, v in out.items()})


def save_intersection_edges():
    """The box test and the triangle test at their branch points (tests/intersection_cases.py) through the reference's own AABB::intersect
    and Figure::intersect.  Outputs only: the inputs are the case table's."""
    import intersection_cases
    out = intersection_cases.evaluate("reference")
    np.savez_compressed(os.path.join(HERE, "pins_intersection_edges.npz"), **{k: out[k] for k in intersection_cases.FAMILIES})
    print("intersection edges", {k: v.shape for k, v in out.items()})


def save_shading_edges():
    """The shading layer at its branch points (tests/shading_cases.py) through the reference's own MaterialModel (hw8 and hw7), Vndf, Cosine
    and tone-mapping.  Outputs only: the inputs are the case table's."""
    import shading_cases
    out = shading_cases.evaluate("reference")
    np.savez_compressed(os.path.join(HERE, "pins_shading_edges.npz"), **{k: out[k] for k in shading_cases.REFERENCE_FAMILIES})
    print("shading edges", {k: v.shape for k, v in out.items()})


def save_env_uv():
    """The environment-map uv of a miss (hw8/src/scene.cpp:94-95) evaluated on the reference's own Ray / Vec3."""
    d = pin_cases.env_uv_directions()
    uv = oracle_lib.env_uv(C.CDLL(oracle_lib.ref_path("libref_hw8.so")), "ref8_env_uv", d)
    np.savez_compressed(os.path.join(HERE, "pins_env_uv.npz"), d=d, uv=uv)
    print("env uv", d.shape)


def save_oracle_orders():
    """Figure order, light order and tree statistics the ORACLE's builder leaves on the cases of tests/test_oracle_orders.py.  A pin of
    the oracle to itself: write it only from an oracle that passes tests/test_oracle_pins.py against the reference."""
    import test_oracle_orders
    out = {f"{case}/{k}": v for case in test_oracle_orders.CASES for k, v in test_oracle_orders.orders(case).items()}
    np.savez_compressed(os.path.join(HERE, "pins_oracle_orders.npz"), **out)
    print("oracle orders", {k: v.shape for k, v in out.items()})


def save_function_inputs():
    """The soup case's queries, so that tests can tell the goldens still answer the questions pin_cases asks today."""
    out = pin_cases.function_inputs(pin_cases.random_triangle_scene(), 23)
    np.savez_compressed(os.path.join(HERE, "pins_hw8_functions_soup_inputs.npz"), **out)
    print("soup inputs", {k: v.shape for k, v in out.items()})


def save_reference_crops():
    """Crops of full-size frames through the reference's hw7 and hw6 integrators (whole frames would take the CPU hours, hence crops)."""
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as td:
        ref7 = oracle_lib.Ref7(pin_cases.synth_room_without_textures(td))
    for x0, y0 in pin_cases.HW7_HEADLINE_CROPS:
        out[f"hw7_headline_{x0}_{y0}_rgb"], _, _ = ref7.render(1920, 1080, 256, rect=(x0, y0, 32, 32))
        print("hw7 headline crop", (x0, y0), float(out[f"hw7_headline_{x0}_{y0}_rgb"].mean()))
    x0, y0 = pin_cases.HW6_CONFIG3_REF_CROP
    out["hw6_config3_rgb"], out["hw6_config3_rgb8"], _ = oracle_lib.Ref6(pin_cases.load_hw6("practice6_2")).render(1024, 1024, 256, rect=(x0, y0, 16, 16))
    print("hw6 config3 crop", (x0, y0), float(out["hw6_config3_rgb"].mean()))
    np.savez_compressed(os.path.join(HERE, "pins_reference_crops.npz"), **out)


if __name__ == "__main__":
    if sys.argv[1:] == ["orders"]:
        save_oracle_orders()
    elif sys.argv[1:] == ["shading"]:
        save_shading_edges()
    elif sys.argv[1:] == ["intersection"]:
        save_intersection_edges()
    elif sys.argv[1:] == ["analytic"]:
        save_analytic_edges()
    elif sys.argv[1:] == ["texture"]:
        save_texture_edges()
        save_hw8_paths()
    elif sys.argv[1:] == ["light_sums"]:
        save_light_sums()
    else:
        main()

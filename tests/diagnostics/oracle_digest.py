#!/usr/bin/env python3
"""SHA-256 digests of everything one build of the CPU oracle computes on the repository's scenes, for comparing two builds of
oracle/ bit for bit (a refactor of the oracle must leave every digest as it was).  One process per library:

    python tests/diagnostics/oracle_digest.py path/to/liboracle.so out.json [--threads N]
    python tests/diagnostics/oracle_digest.py --compare a.json b.json

Covered: every scene under tests/golden/scenes, the pin_cases generators (sphere, triangle soup, hw7 scenes, HW2/4/5/6_CASES) and the
scene of tools/gen_synth_room.py, each through the oracle that takes it: figure / light orders, tree statistics, light counts, a
whole frame and an off-origin rectangle (float radiance, bytes and, for hw6 / hw8, the four counters), hw3 / hw4 in both seed modes,
hw6 / hw8 once more as sample stream 1, the hw8 scenes once more in hw7 mode where pin_cases.as_hw7 applies, the per-function entry
points on pin_cases.function_inputs(sd, 23) and one rto_hw8_trace_pixel log.  (diagnostic; the oracle is test infrastructure)"""
import argparse, ctypes as C, glob, hashlib, importlib, json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

RECT = (17, 9, 24, 16)
GLTF_FRAME = (64, 48, 8)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update((a.view(np.uint32) if a.dtype == np.float32 else a).tobytes())
    return h.hexdigest()


def counters(c):
    return np.array([c.closest, c.lightq, c.boxes, c.tris], np.uint64)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{len(a)} digests in {pa}, {len(b)} in {pb}, {len(diff)} differences")
    for k in diff:
        print("   differs:", k)
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib"); ap.add_argument("out")
    ap.add_argument("--threads", type=int, default=0, help="0 = the library's default")
    ap.add_argument("--compare", action="store_true", help="lib and out are two JSON files to compare")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.lib, a.out))
    rt = importlib.import_module("raytracing-course-hw_amd")
    import gen_synth_room, oracle_lib, pin_cases
    so = os.path.abspath(a.lib)
    oracle_lib._build = lambda: so                       # the library under test, not the tree's own build
    L = oracle_lib.lib()
    T = a.threads
    out = {}

    def frames(key, render):
        """render(rect, **kw) -> tuple of arrays (counters last, if any); whole frame and the off-origin rectangle."""
        for tag, rect in (("frame", None), ("rect", RECT)):
            r = render(rect)
            out[f"{key}/{tag}"] = sha(*[counters(x) if isinstance(x, oracle_lib.Counters) else x for x in r])

    def tri_scene(key, sd, hw6=False, hw7=False, functions=True):
        w, h, spp = GLTF_FRAME
        orc = oracle_lib.Hw6Oracle(sd) if hw6 else oracle_lib.Hw8Oracle(sd, hw7=hw7)
        out[f"{key}/figure_order"] = sha(orc.figure_order())
        out[f"{key}/light_order"] = sha(orc.light_order())
        out[f"{key}/bvh_stats"] = sha(orc.bvh_stats())
        out[f"{key}/num_lights"] = int(len(orc.light_order()))
        frames(key, lambda rect: orc.render(w, h, spp, rect=rect, threads=T))
        frames(key + "/stream1", lambda rect: orc.render(w, h, spp, rect=rect, threads=T, seed_offset=w * h))
        if functions and not hw6:
            for k, v in pin_cases.eval_functions(orc, sd, 23).items():
                out[f"{key}/fn_{k}"] = sha(v)
        return orc

    # ---- .txt scenes: the file's own size, or 64x48 where the file asks for less (the rectangle has to fit) ----
    flavors = {"hw1": rt.RT_INTEGRATOR_HW1, "hw2": rt.RT_INTEGRATOR_HW2, "hw3": rt.RT_INTEGRATOR_HW3, "hw4": rt.RT_INTEGRATOR_HW4,
               "hw5": rt.RT_INTEGRATOR_HW5}
    txt = sorted(glob.glob(os.path.join(pin_cases.SCENES, "txt", "*.txt")))
    names = [os.path.splitext(os.path.basename(p))[0] for p in txt]
    assert set(pin_cases.HW2_CASES + pin_cases.HW4_CASES + pin_cases.HW5_CASES) <= set(names)
    for path, name in zip(txt, names):
        hw = name[:3]
        sd, w, h, spp, depth = rt.load_txt(path, flavors[hw])
        if w * h < 64 * 48:
            w, h = 64, 48
        key = "txt/" + name
        if hw == "hw1":
            out[key + "/frame"] = sha(*oracle_lib.TxtOracle(sd).render_hw1(w, h))
        elif hw == "hw2":
            orc = oracle_lib.Hw2Oracle(sd)
            frames(key, lambda rect: orc.render(w, h, depth, rect=rect, threads=T))
        elif hw == "hw3":
            orc = oracle_lib.TxtOracle(sd)
            for mode in (False, True):
                frames(f"{key}/per_pixel_seed={int(mode)}", lambda rect: orc.render_hw3(w, h, spp, depth, mode, rect=rect, threads=T))
        elif hw == "hw4":
            orc = oracle_lib.Hw4Oracle(sd)
            out[key + "/num_lights"] = int(orc.num_lights())
            for mode in (False, True):
                frames(f"{key}/per_pixel_seed={int(mode)}", lambda rect: orc.render(w, h, spp, depth, mode, rect=rect, threads=T))
        else:
            orc = oracle_lib.Hw5Oracle(sd)
            fo, lo = orc.orders()
            out[key + "/figure_order"], out[key + "/light_order"], out[key + "/num_lights"] = sha(fo), sha(lo), int(len(lo))
            frames(key, lambda rect: orc.render(w, h, spp, depth, rect=rect, threads=T))
        print(key, (w, h, spp, depth), flush=True)

    # ---- glTF scenes of tests/golden/scenes and the generators ----
    for path in sorted(glob.glob(os.path.join(pin_cases.SCENES, "hw6", "*.gltf"))):
        tri_scene("hw6/" + os.path.basename(path)[:-5], rt.load_gltf(path, rt.RT_INTEGRATOR_HW6), hw6=True)
    tri_scene("hw6/hw6_soup", pin_cases.hw6_soup(), hw6=True)
    assert set(pin_cases.HW6_CASES) == {"practice6_1", "practice6_2", "hw6_soup"}
    print("hw6 done", flush=True)
    for path in sorted(glob.glob(os.path.join(pin_cases.SCENES, "hw7", "*.gltf"))):
        name = os.path.basename(path)[:-5]
        tri_scene("hw7/" + name, pin_cases.load_hw7(name), hw7=True)
    print("hw7 done", flush=True)
    for path in sorted(glob.glob(os.path.join(pin_cases.SCENES, "hw8_sphere", "*.gltf"))):
        name = os.path.basename(path)[:-5]
        tri_scene("hw8/" + name, rt.load_gltf(path))
        tri_scene("hw8_as_hw7/" + name, pin_cases.as_hw7(rt.load_gltf(path)), hw7=True)
    soup = pin_cases.random_triangle_scene()
    orc = tri_scene("hw8/soup", soup)
    L.rto_hw8_trace_pixel.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int]
    buf = np.zeros(12 * 4096, np.float32)
    m = L.rto_hw8_trace_pixel(orc._h, 40, 32, 6, 0, 20, 15, buf.ctypes.data, buf.size)
    assert m > 0
    out["hw8/soup/trace_pixel"] = sha(buf[:m])
    tri_scene("hw8_as_hw7/soup", pin_cases.as_hw7(pin_cases.random_triangle_scene()), hw7=True)
    print("hw8 done", flush=True)
    with tempfile.TemporaryDirectory() as td:
        gltf, _ = gen_synth_room.generate(td, 64, 50, 43)
        room = rt.load_gltf(gltf)
    tri_scene("hw8/synth_room", room)
    print("synth room done", flush=True)
    json.dump(out, open(a.out, "w"), indent=0, sort_keys=True)
    print(f"{len(out)} digests -> {a.out}")


if __name__ == "__main__":
    main()

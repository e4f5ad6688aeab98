import sys, importlib, os
sys.path.insert(0, os.getcwd())
rt = importlib.import_module("raytracing-course-hw_amd")
sd, _, _, _, depth = rt.load_txt(os.path.join(os.getcwd(), "tests", "golden", "scenes", "txt", "hw5_mixed_figures.txt"), rt.RT_INTEGRATOR_HW5)
w, h, spp = 400, 300, 32
scene = rt.Scene(sd)
best = 1e9
for _ in range(5):
    rgb, _, st = scene.render(w, h, spp, integrator=rt.RT_INTEGRATOR_HW5, ray_depth=depth, want_rgb8=False)
    best = min(best, st.kernel_ms)
print(f"hw5 mixed figures ({w}x{h}x{spp}): best of 5 {best:.3f} ms = {w * h * spp / best / 1e3:.0f} Msamples/s")

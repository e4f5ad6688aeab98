"""The headline frame (synth_room_v1 1920x1080x256) through the round pipeline (RTAMD_KERNEL=wavefront): kernel time and the sum of the
traverse launches, one line per render.  RTAMD_LIB selects the library, so a parent build and the tree's alternate as processes:
    python tools/profiling/round_pipeline.py [--runs N] [--lds-stack 3] [--sha]
--lds-stack K sets RTAMD_WF_LDS_STACK (3: the spill variant on every ray); --sha prints the SHA-256 of the float and the 8-bit frame."""
import argparse, hashlib, importlib, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=1)
ap.add_argument("--lds-stack", type=int, default=0)
ap.add_argument("--sha", action="store_true")
args = ap.parse_args()
os.environ["RTAMD_KERNEL"] = "wavefront"
if args.lds_stack: os.environ["RTAMD_WF_LDS_STACK"] = str(args.lds_stack)
rt = importlib.import_module("raytracing-course-hw_amd")
import gen_synth_room
with tempfile.TemporaryDirectory(prefix="synth_room_") as tmp:
    scene = rt.Scene(rt.load_gltf(gen_synth_room.generate(tmp, 64, 50, 43)[0]))
W, H, SPP = 1920, 1080, 256
for k in range(args.runs):
    rgb, rgb8, st = scene.render(W, H, SPP)
    assert st.pipeline == rt.RT_PIPELINE_ROUNDS
    sha = "  sha256 " + hashlib.sha256(rgb.tobytes()).hexdigest()[:16] + " " + hashlib.sha256(rgb8.tobytes()).hexdigest()[:16] if args.sha else ""
    print(f"round pipeline{' lds stack ' + str(args.lds_stack) if args.lds_stack else ''} {W}x{H}x{SPP}: kernel {st.kernel_ms:.1f} ms, traverse launches {st.dominant_kernel_ms:.1f} ms "
          f"({st.dominant_kernel_launches}), {W * H * SPP / st.kernel_ms / 1e3:.2f} Msamples/s{sha}", flush=True)
scene.close()

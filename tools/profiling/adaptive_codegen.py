"""CPU-side codegen checks of the adaptive-sampling change (profiles/r35_adaptive.txt, section c).  No GPU needed: hipcc cross-compiles.
  1. every kernel of a parent checkout against this tree, instruction for instruction: each translation unit that holds kernels is
     compiled to gfx950 assembly (the Makefile's flags, --cuda-device-only -S) in both trees, the assembly is cut into functions, label
     numbers are renamed in order of appearance, and each kernel symbol of the parent must have the same text here;
  2. the -Rpass-analysis=kernel-resource-usage lines of the persistent kernels and of the new flat kernels.
Run by hand:
    python tools/profiling/adaptive_codegen.py --parent /path/to/a/checkout/of/the/parent/commit"""
import argparse, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
args = ap.parse_args()
FLAGS = "-std=c++17 -O3 -fPIC -ffp-contract=off -Wall -Wno-unused-function".split()
UNITS = {"rtamd_api.hip": ["-mllvm", "-disable-machine-licm"], "rtamd_noise.hip": [], "rtamd_multi.hip": [], "rtamd_denoise.hip": [], "rtamd_build.hip": []}


def compile_unit(tree, unit, extra, out):
    csrc = os.path.join(tree, "raytracing-course-hw_amd", "csrc")
    cmd = [args.hipcc] + FLAGS + extra + ["--offload-arch=gfx950", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", unit, "-o", out]
    return subprocess.run(cmd, cwd=csrc, check=True, capture_output=True, text=True).stderr


def functions(path):
    """symbol -> normalised text of every function of an assembly file; and the set of kernel symbols"""
    funcs, kernels, name, body = {}, set(), None, []
    for raw in open(path):
        line = raw.rstrip()
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L") and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                funcs[name] = body
                name = None
                continue
            code = line.split(";")[0].strip()
            if code and not code.startswith((".p2align", ".loc", ".file", ".cfi")):
                body.append(code)
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernels.add(m.group(1))
    out = {}
    for k, body in funcs.items():
        names = {}
        def rename(m):
            return names.setdefault(m.group(0), f".L{len(names)}")
        out[k] = [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", rename, c) for c in body]
    return out, kernels


def usage(stderr):
    """kernel -> its resource line"""
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur and "AGPR" not in line:
                res[cur].setdefault(key, m.group(1))
    return {k: " ".join(f"{a}: {b}" for a, b in v.items()) for k, v in res.items()}


total = same = insns = 0
differ, new, lines = [], [], {}
with tempfile.TemporaryDirectory(prefix="adaptive_codegen_") as tmp:
    for unit, extra in UNITS.items():
        a, b = os.path.join(tmp, "parent_" + unit + ".s"), os.path.join(tmp, "this_" + unit + ".s")
        compile_unit(args.parent, unit, extra, a)
        err = compile_unit(ROOT, unit, extra, b)
        fa, ka = functions(a)
        fb, kb = functions(b)
        for k in sorted(ka):
            total += 1
            insns += len(fa[k])
            if k in kb and fa[k] == fb[k]:
                same += 1
            else:
                differ.append(f"{unit}: {k}" + ("" if k in kb else " (missing)"))
        new += [f"{unit}: {k}" for k in sorted(kb - ka)]
        for k, v in usage(err).items():
            lines[k] = v
print(f"kernels of the parent: {total} ({insns} lines of assembly); the same instructions in this tree: {same}; different or missing: {len(differ)}")
for d in differ:
    print("  DIFFERENT", d)
print(f"kernels only in this tree: {len(new)}")
for n in new:
    print("  new", n)
print("resource usage (this tree), the persistent hw8 kernels and the new flat kernels:")
for k in sorted(lines):
    if "pt_persistent_kernel" in k or "ad_" in k or "vw_" in k:
        print(f"  {k} {lines[k]}")
sys.exit(1 if differ else 0)

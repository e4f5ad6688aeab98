"""How the persistent kernels' walkers fetch what they test, read from the compiler's assembly (rtamd_api.hip for gfx950 with the Makefile's
flags, no GPU): no flat access anywhere in the four plain kernels, the budget of tests/test_kernel_resources.py unchanged, and in the four
hot loops of the hw8 / hw7 kernels (two node loops, two leaf loops) every fetch at a 32-bit offset from a scalar base — no 64-bit address
arithmetic in the VALU.  Static counts of pt_persistent_kernel<false,0>, parent of this test against the source it came with
(profiles/r32_walker_loads.txt): flat_load 25 -> 0, v_mad_u64_u32 65 -> 60, v_lshl_add_u64 81 -> 78, v_lshlrev_b64 10 -> 8.
One more case, host only: the bound that lets the offsets be 32 bits wide (rt_types.h walk_arrays_fit), on made-up counts."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
PT_KERNELS = ["pt_persistent_kernelILb0ELi0EEE", "pt_persistent_kernelILb0ELi1EEE", "pt_persistent_kernelILb0ELi2EEE"]
KERNELS = PT_KERNELS + ["p6_persistent_kernelILb0EEE"]
WIDE = ("v_mad_u64_u32", "v_lshl_add_u64", "v_lshlrev_b64")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = []
    for var in ("CXXFLAGS", "DEVFLAGS"):
        flags += re.search(rf"^{var} := (.*)$", text, re.M).group(1).replace("$(EXTRA)", "").split()
    return flags


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{kernel: assembly lines of its body}, {kernel: resource usage}"""
    if HIPCC is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / "rtamd_api.s"
    cmd = [HIPCC] + _makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", "rtamd_api.hip", "-o", str(out)]
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out).read().splitlines()
    bodies = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\S+):", lines[i])
        k = next((k for k in KERNELS if m and k in m.group(1)), None)
        if k:
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            bodies[k] = lines[i + 1:j]
            i = j
        i += 1
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), None)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split(" [")[0]] = int(m.group(2))
    assert sorted(bodies) == sorted(KERNELS) and sorted(usage) == sorted(KERNELS)
    return bodies, usage


def _insn(line):
    line = line.strip()
    if not line or line[0] in ".;" or line.endswith(":"):
        return None
    return line.split()[0]


def _loops(body):
    """(top, branch) line numbers of every backward branch"""
    labels = {m.group(1): n for n, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    out = []
    for n, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), n) < n:
            out.append((labels[m.group(1)], n))
    return out


def _count(body, a, b, pred):
    return sum(1 for l in body[a:b + 1] if (_insn(l) or "") and pred(_insn(l)))


def _hot_loops(body):
    """The two node loops: the smallest loops around a cluster of eight or more v_perm_b32 (the slab test on the 16-bit grid) with the four
    16-byte loads of a node.  The leaf loop of each: the smallest loop with divisions (v_div_scale_f32: the triangle test) that begins after it."""
    loops = _loops(body)
    nodes = []
    for a, b in sorted(loops, key=lambda ab: ab[1] - ab[0]):
        if _count(body, a, b, lambda x: x == "v_perm_b32") >= 8 and _count(body, a, b, lambda x: x == "global_load_dwordx4") >= 4 \
                and not _count(body, a, b, lambda x: x == "v_div_scale_f32") and not any(a <= c and d <= b for c, d in nodes):
            nodes.append((a, b))
    leaves = []
    for a, b in nodes:
        after = [(c, d) for c, d in loops if c > b and _count(body, c, d, lambda x: x == "v_div_scale_f32") >= 2]
        first = min(c for c, d in after)
        leaves.append(min(((c, d) for c, d in after if c - first < 8), key=lambda cd: cd[1] - cd[0]))
    return sorted(nodes), sorted(leaves)


def test_no_flat_access_and_the_budget(compiled):
    bodies, usage = compiled
    for k in KERNELS:
        ins = [x for x in map(_insn, bodies[k]) if x]
        print(k, usage[k], "flat", sum(x.startswith("flat_") for x in ins), {w: ins.count(w) for w in WIDE}, "VALU", sum(x.startswith("v_") for x in ins), "all", len(ins))
    for k in KERNELS:
        assert not [l for l in bodies[k] if (_insn(l) or "").startswith("flat_")], k
        u = usage[k]
        assert u["VGPRs"] <= 96 and u["ScratchSize"] == 0 and u["Occupancy"] == 5 and u["LDS Size"] <= 32000, (k, u)


@pytest.mark.parametrize("kernel", PT_KERNELS)
def test_hot_loops_fetch_at_32_bit_offsets(compiled, kernel):
    body = compiled[0][kernel]
    nodes, leaves = _hot_loops(body)
    print(kernel, "node loops", nodes, "leaf loops", leaves)
    assert len(nodes) == 2 and len(leaves) == 2 and len(set(leaves)) == 2
    for a, b in nodes + leaves:
        wide = [l.strip() for l in body[a:b + 1] if _insn(l) in WIDE]
        loads = [l.strip() for l in body[a:b + 1] if (_insn(l) or "").startswith("global_load")]
        print(f"  lines {a}-{b}: {len(loads)} loads, 64-bit address instructions: {wide}")
        assert not wide, (kernel, a, b, wide)
        assert loads and all(re.search(r"global_load_\w+ v(\[\d+:\d+\]|\d+), v\d+, s\[\d+:\d+\]", l) for l in loads), (kernel, a, b, loads)


def test_the_bound_of_the_32_bit_offsets():
    path = os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so")
    if not os.path.exists(path):
        pytest.skip("test hooks not built")
    L = C.CDLL(path)
    L.rtt_walk_arrays_fit.argtypes = [C.c_uint64] * 4
    L.rtt_walk_arrays_fit.restype = C.c_int
    fit = L.rtt_walk_arrays_fit
    assert fit(0, 0, 1, 1) == 1 and fit(1 << 24, 1 << 24, (1 << 24) - 1, (1 << 24) - 1) == 1  # the largest scene the figure index allows
    assert fit((1 << 24) + 1, 0, 1, 1) == 0 and fit(1, (1 << 24) + 1, 1, 1) == 0              # a record index beyond the 24-bit multiply
    assert fit(1, 1, 1 << 26, 1) == 0 and fit(1, 1, 1, 1 << 26) == 0                          # 2^26 nodes of 64 bytes are 4 GiB
    assert fit(1, 1, (1 << 26) - 1, (1 << 26) - 1) == 1

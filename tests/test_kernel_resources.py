"""The register, scratch and LDS budget of the persistent kernels, as the compiler reports it: the headline rests on five waves per SIMD
(96 VGPRs, no scratch, a CU's LDS shared by its workgroups) and on the Makefile's -disable-machine-licm, which is what keeps them there."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
KERNELS = ["pt_persistent_kernelILb0ELi0EEE", "pt_persistent_kernelILb0ELi1EEE", "pt_persistent_kernelILb0ELi2EEE", "p6_persistent_kernelILb0EEE"]


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = []
    for var in ("CXXFLAGS", "DEVFLAGS"):
        flags += re.search(rf"^{var} := (.*)$", text, re.M).group(1).replace("$(EXTRA)", "").split()
    return flags


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_persistent_kernels_keep_their_budget(tmp_path):
    """rtamd_api.hip compiled for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage: pt_persistent_kernel<false, 0|1|2>
    and p6_persistent_kernel<false> use at most 96 VGPRs, no scratch and at most 32,000 bytes of LDS, at an occupancy of 5 waves per SIMD
    (96 / 0 / 5, 31,680 and 31,904 bytes)."""
    cmd = [HIPCC] + _makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                         "-c", "rtamd_api.hip", "-o", str(tmp_path / "rtamd_api.device.o")]
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), None)
            if name:
                found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in KERNELS:
        print(k, found.get(k))
    assert sorted(found) == sorted(KERNELS)
    for k in KERNELS:
        u = found[k]
        assert u["VGPRs"] <= 96, (k, u)
        assert u["ScratchSize"] == 0, (k, u)
        assert u["Occupancy"] == 5, (k, u)
        assert u["LDS Size"] <= 32000, (k, u)

"""The compiler's resource report for the persistent hw8 kernel with a path source (WF_FEAT_SOURCE, with and without the environment
lookup): the budget the render's speed rests on -- at most 96 VGPRs, no scratch, five waves per SIMD, at most 32,000 bytes of LDS.
The compile line is tests/test_kernel_resources.py's."""
import re
import subprocess

import pytest

import test_kernel_resources as K

SOURCE = ["pt_persistent_kernelILb0ELi4EEE", "pt_persistent_kernelILb0ELi5EEE"]


@pytest.mark.skipif(K.HIPCC is None, reason="hipcc is not installed")
def test_source_kernels_keep_the_persistent_budget(tmp_path):
    cmd = [K.HIPCC] + K._makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                             "-c", "rtamd_api.hip", "-o", str(tmp_path / "rtamd_api.device.o")]
    r = subprocess.run(cmd, cwd=K.CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in SOURCE if k in m.group(1)), None)
            if name:
                found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in SOURCE:
        print(k, found.get(k))
    assert sorted(found) == sorted(SOURCE)
    for k in SOURCE:
        u = found[k]
        assert u["VGPRs"] <= 96 and u["ScratchSize"] == 0 and u["Occupancy"] == 5 and u["LDS Size"] <= 32000, (k, u)

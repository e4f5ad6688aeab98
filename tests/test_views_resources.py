"""The compiler's resource report for the persistent hw8 kernel with the view source (WF_FEAT_SOURCE | WF_FEAT_VIEWS, with and without
the environment lookup; include/rtamd.h: rt_views_*): the budget of the other source kernels -- at most 96 VGPRs, no scratch, five
waves per SIMD, at most 32,000 bytes of LDS.  The compile line is tests/test_kernel_resources.py's."""
import re
import subprocess

import pytest

import test_kernel_resources as K

VIEWS = ["pt_persistent_kernelILb0ELi36EEE", "pt_persistent_kernelILb0ELi37EEE"]   # 4 | 32, and with WF_FEAT_ENV = 1


@pytest.mark.skipif(K.HIPCC is None, reason="hipcc is not installed")
def test_view_kernels_keep_the_persistent_budget(tmp_path):
    cmd = [K.HIPCC] + K._makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                             "-c", "rtamd_api.hip", "-o", str(tmp_path / "rtamd_api.device.o")]
    r = subprocess.run(cmd, cwd=K.CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in VIEWS if k in m.group(1)), None)
            if name:
                found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in VIEWS:
        print(k, found.get(k))
    assert sorted(found) == sorted(VIEWS)
    for k in VIEWS:
        u = found[k]
        assert u["VGPRs"] <= 96 and u["ScratchSize"] == 0 and u["Occupancy"] == 5 and u["LDS Size"] <= 32000, (k, u)

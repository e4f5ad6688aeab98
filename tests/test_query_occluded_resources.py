"""The compiler's resource report for the occlusion walk: rq_any_kernel in both variants uses no scratch, at most rq_closest_kernel's
VGPRs (52, SPILL 56), 30,720 bytes of LDS and runs at five waves per SIMD; rq_closest_kernel and rq_light_kernel keep the figures of
profiles/r20_ray_queries.txt.  The compile line is tests/test_kernel_resources.py's."""
import re
import subprocess

import pytest

import test_kernel_resources as K

# mangled-name fragment -> (VGPRs, at most or exactly, LDS bytes)
ANY = {"rq_any_kernelILb0EEE": 52, "rq_any_kernelILb1EEE": 56}
KEPT = {"rq_closest_kernelILb0EEE": 52, "rq_closest_kernelILb1EEE": 56, "rq_light_kernelE": 72}


@pytest.mark.skipif(K.HIPCC is None, reason="hipcc is not installed")
def test_occlusion_walk_fits_the_closest_walks_budget(tmp_path):
    cmd = [K.HIPCC] + K._makefile_flags() + ["--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                             "-c", "rtamd_api.hip", "-o", str(tmp_path / "rtamd_api.device.o")]
    r = subprocess.run(cmd, cwd=K.CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    wanted = list(ANY) + list(KEPT)
    found, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in wanted if k in m.group(1)), None)
            if name:
                found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in wanted:
        print(k, found.get(k))
    assert sorted(found) == sorted(wanted)
    for k, vgprs in ANY.items():
        u = found[k]
        assert u["VGPRs"] <= vgprs and u["ScratchSize"] == 0 and u["LDS Size"] == 30720 and u["Occupancy"] == 5, (k, u)
    for k, vgprs in KEPT.items():
        u = found[k]
        assert u["VGPRs"] == vgprs and u["ScratchSize"] == 0 and u["LDS Size"] == 30720 and u["Occupancy"] == 5, (k, u)

"""Every refusal of the query layer that a caller can provoke (tests/query_refusal_cases.py: a null scene, then the sphere scene as
hw8 scene, as hw6 scene and without its light, device arrays offset into their allocations, RTAMD_KERNEL): return code and message
equal the transcript in tests/golden/query_refusals.txt line by line.  The cases run in a child process, where torch opens the GPU
before the library does."""
import os
import subprocess
import sys

import pytest

import query_refusal_cases as cases

pytestmark = pytest.mark.gpu


def test_refusals_equal_the_transcript():
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "query_refusal_cases.py"), "gpu", "-"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = open(cases.GOLDEN_GPU).read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w

"""What the query layer's thirteen launching calls answer and report (tests/query_digest_cases.py: digests of every array written,
the engines after the call, and the deterministic stats fields, across chunk seams, with host arrays and with device pointers)
equals the transcript in tests/golden/query_digests.txt line by line.  The cases run in one child process under
RTAMD_QUERY_CHUNK=64, where torch opens the GPU before the library does."""
import os
import subprocess
import sys

import pytest

import query_digest_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lines():
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "query_digest_cases.py"), "-"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_digests_and_stats_equal_the_transcript(lines):
    want = open(cases.GOLDEN).read().splitlines()
    assert len(lines) == len(want)
    for g, w in zip(lines, want):
        assert g == w


def test_host_arrays_and_device_pointers_give_the_same_digests(lines):
    assert len(lines) % 2 == 0 and cases.host_and_device_differ(lines) == []

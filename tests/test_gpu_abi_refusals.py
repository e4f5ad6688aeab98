"""Every refusal of rt_render, rt_accum_*, rt_multi_* and rt_noise_* / rt_multi_noise_* that a caller can provoke on live objects
(tests/abi_refusal_cases.py: the sphere scene, 16x16 and 8x8 frames, device lists [0] and [0, 0, 0]): return code and message
equal the transcript in tests/golden/abi_refusals.txt line by line."""
import pytest

import abi_refusal_cases as cases

pytestmark = pytest.mark.gpu


def test_refusals_equal_the_transcript(rt):
    want = open(cases.GOLDEN_GPU).read().splitlines()
    got = cases.run_host(rt, False) + cases.run_gpu(rt)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w

"""The refusals of the C-ABI that need no device (tests/abi_refusal_cases.py HOST: null handles, struct_size, rt_accum_state_bytes,
rt_unshard, rt_output_elems, and without a GPU the no-device answers): return code and message equal the transcript in
tests/golden/abi_refusals_host.txt line by line.  With a GPU present no call here reaches HIP, as in the other host tests."""
import abi_refusal_cases as cases


def test_host_refusals_equal_the_transcript(rt):
    import torch
    no_device = not torch.cuda.is_available()
    want = open(cases.GOLDEN_HOST).read().splitlines()
    if not no_device:  # with a GPU those two calls succeed: they are not refusals there
        want = [line for line in want if not line.startswith("nodevice.")]
    got = cases.run_host(rt, no_device)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w

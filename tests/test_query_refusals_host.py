"""The refusals of the query layer that are decided before the scene is looked at (tests/query_refusal_cases.py HOST: thirteen
entry points on a null scene): return code and message equal the transcript in tests/golden/query_refusals_host.txt line by line,
and so does the order in which a call judges its arguments.  No call here reaches HIP."""
import query_refusal_cases as cases


def test_host_refusals_equal_the_transcript(rt):
    want = open(cases.GOLDEN_HOST).read().splitlines()
    got = cases.run_host(rt)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w

"""The one guard of the C boundary (csrc/host/rt_guard.h), reached on the host through the test hooks: what a body throws becomes a
return code and `who` + its text in rt_last_error(); nothing crosses the boundary.  No GPU."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARG, RT_ERR_HIP = -1, -3


def test_guard_maps_exceptions_to_codes_and_prefixes_the_message(rt):
    hooks = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    hooks.rtt_guard_probe.argtypes = [C.c_int]
    assert rt.lib.rt_render(None, None, None, None, None) == RT_ERR_INVALID_ARG   # some other message first
    assert hooks.rtt_guard_probe(4) == 5                                        # no exception: the body's own answer, no message
    assert rt.lib.rt_last_error() == b"rt_render: null argument"
    assert hooks.rtt_guard_probe(0) == RT_ERR_HIP                               # HipError
    assert rt.lib.rt_last_error() == b"rtt_guard_probe: hipProbe(): failed"
    assert hooks.rtt_guard_probe(1) == RT_ERR_INVALID_ARG                       # std::bad_alloc
    assert rt.lib.rt_last_error() == b"rtt_guard_probe: std::bad_alloc"
    assert hooks.rtt_guard_probe(2) == RT_ERR_INVALID_ARG                       # any other std::exception
    assert rt.lib.rt_last_error() == b"rtt_guard_probe: a runtime error"
    assert hooks.rtt_guard_probe(3) == RT_ERR_INVALID_ARG                       # not a std::exception at all
    assert rt.lib.rt_last_error() == b"rtt_guard_probe: unknown exception"

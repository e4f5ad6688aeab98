"""rng_n01x3 (rt_device.h), the three normal draws of cosine_sample in one call, against three rng_n01 calls on the GPU: the three
values, the engine's state, the saved value and its flag, bit for bit, from both entry states (with and without a saved value)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEEDS = 4096


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    L.rtt_rng_triple.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    return L


def _triples(hooks, prior):
    """[seed][side][word]: side 0 three rng_n01 calls, side 1 rng_n01x3; words a, b, c, x, saved, has_saved, has_saved on entry, engine steps"""
    out = np.zeros((N_SEEDS, 2, 8), dtype=np.uint32)
    assert hooks.rtt_rng_triple(1, N_SEEDS, prior, out.ctypes.data) == 0
    return out


def test_rng_n01x3_is_three_rng_n01_calls(hooks):
    entered = set()
    rejected = 0
    for prior in (0, 1):
        out = _triples(hooks, prior)
        three, triple = out[:, 0, :], out[:, 1, :]
        bad = np.flatnonzero((three != triple).any(axis=1))
        print(f"after {prior} rng_n01 calls: {N_SEEDS} seeds, {bad.size} differ; entered with a saved value: {int(three[:, 6].sum())}; "
              f"engine steps of a triple: {np.bincount(three[:, 7]).nonzero()[0].tolist()}")
        for i in bad[:5]:
            print(f"  seed {1 + i}: three calls {[hex(v) for v in three[i]]}, rng_n01x3 {[hex(v) for v in triple[i]]}")
        assert bad.size == 0
        # the state on entry is what the test says it is, and the flag afterwards is its opposite (one or two polar rounds)
        assert (three[:, 6] == prior).all() and (three[:, 5] == 1 - prior).all()
        entered |= set(three[:, 6].tolist())
        # a polar round without a rejected pair takes two engine steps: one round after a saved value, two without
        base = 2 if prior else 4
        assert (three[:, 7] >= base).all() and ((three[:, 7] - base) % 2 == 0).all()
        rejected += int((three[:, 7] > base).sum())
    assert entered == {0, 1}
    print(f"triples with at least one rejected polar pair: {rejected}")
    assert rejected > 0

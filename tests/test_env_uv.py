"""Pins the environment-map uv of a miss (hw8/src/scene.cpp:94-95) against the reference's own types.

Vec3's members are float, so the reference's std::atan2 / std::asin resolve to atan2f / asinf; only their results are widened to
double.  tests/golden/pins_env_uv.npz holds directions (pin_cases.env_uv_directions: random unit vectors and the edges of both
functions) and the uv that the reference's two lines give for them, evaluated on its own Ray / Vec3 (oracle/ref/ref_hw8_funcs.cpp
ref8_env_uv).  The bar is bit-exact equality."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
import pin_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pins_env_uv.npz")
N_RANDOM = 20000   # pin_cases.env_uv_directions: the random unit vectors come first, the edge set after them


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g["d"], g["uv"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uv_from_libm(d):
    """scene.cpp:94-95 with the host libm's atan2f / asinf (rto_atan2f_array, rto_asinf_array) and the rest in double."""
    L = oracle_lib.lib()
    L.rto_atan2f_array.argtypes = [C.c_void_p] * 3 + [C.c_size_t]
    L.rto_asinf_array.argtypes = [C.c_void_p] * 2 + [C.c_size_t]
    y, x, dy = (np.ascontiguousarray(d[:, i]) for i in (2, 0, 1))
    a, s = np.zeros_like(y), np.zeros_like(y)
    L.rto_atan2f_array(y.ctypes.data, x.ctypes.data, a.ctypes.data, y.size)
    L.rto_asinf_array(dy.ctypes.data, s.ctypes.data, dy.size)
    tx = (0.5 + 0.5 * a.astype(np.float64) / np.pi).astype(np.float32)
    ty = (0.5 - s.astype(np.float64) / np.pi).astype(np.float32)
    return np.stack([tx, ty], axis=1)


def test_golden_answers_todays_directions(gold):
    d, uv = gold
    assert np.array_equal(_bits(d), _bits(pin_cases.env_uv_directions())), "pin_cases.env_uv_directions changed: regenerate the golden"
    assert uv.shape == (d.shape[0], 2) and d.shape[0] > N_RANDOM


def test_oracle_env_uv_matches_reference(gold):
    d, uv = gold
    got = oracle_lib.env_uv(oracle_lib.lib(), "rto_hw8_env_uv", d)
    bad = np.flatnonzero((_bits(got) != _bits(uv)).any(axis=1))
    assert bad.size == 0, f"{bad.size} directions differ from the reference, first {d[bad[:3]].tolist()}: {got[bad[:3]].tolist()} vs {uv[bad[:3]].tolist()}"


def test_golden_is_reproduced_by_host_float_libm(gold):
    """The golden is atan2f / asinf of this host's libm plus double arithmetic.  If not, the host libm is not the one the golden was
    made with (glibc 2.35, x86-64), and the oracle's env-map pixels cannot be the reference's on this host."""
    d, uv = gold
    live = _uv_from_libm(d)
    bad = int((_bits(live) != _bits(uv)).any(axis=1).sum())
    assert bad == 0, f"this host's atan2f / asinf differ from the libm the golden was made with on {bad} of {d.shape[0]} directions"


def test_double_argument_formula_is_told_apart(gold):
    """Sensitivity: the double-argument formula (atan2 / asin on doubles, the former oracle and device) misses the golden on many of the
    random directions, so a pin that passes is a pin on the float overloads."""
    d, uv = gold
    dd = d[:N_RANDOM].astype(np.float64)
    tx = (0.5 + 0.5 * np.arctan2(dd[:, 2], dd[:, 0]) / np.pi).astype(np.float32)
    ty = (0.5 - np.arcsin(dd[:, 1]) / np.pi).astype(np.float32)
    frac_x = float((_bits(tx) != _bits(uv[:N_RANDOM, 0])).mean())
    frac_y = float((_bits(ty) != _bits(uv[:N_RANDOM, 1])).mean())
    print(f"double-argument formula differs from the float overloads: tx {frac_x:.2%}, ty {frac_y:.2%} of {N_RANDOM} random directions")
    assert frac_x > 0.10 and frac_y > 0.10


def test_edges_where_the_overloads_part(gold):
    """The seam and the poles, where the float overloads give a coordinate just below 0 (and the texture lookup wraps it to 1.0f):
    atan2f(-0, -x) = -pi_f gives tx < 0, asinf(1) = pi_f / 2 gives ty < 0.  Double atan2 / asin gave exactly 0 there."""
    d, uv = gold
    seam = (d[:, 2] == 0) & np.signbit(d[:, 2]) & (d[:, 0] < 0) & (d[:, 1] == 0)
    pole = d[:, 1] == 1
    assert seam.any() and pole.any()
    assert np.all(uv[seam, 0] < 0) and np.all(uv[seam, 0] > -1e-7)
    assert np.all(uv[pole, 1] < 0) and np.all(uv[pole, 1] > -1e-7)
    seam_p = (d[:, 2] == 0) & ~np.signbit(d[:, 2]) & (d[:, 0] < 0) & (d[:, 1] == 0)
    assert seam_p.any() and np.all(uv[seam_p, 0] == 1.0)

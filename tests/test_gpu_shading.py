"""The device's shading layer (rt_device.h: material_brdf and its two variants, the cosine and VNDF samplers with both signatures, aces1 /
tonemap1) at the branch points of that code, one lane per case (csrc/test_hooks.hip rtt_brdf .. rtt_disk_point call the product's
functions).  Against the compiled reference's answers (tests/golden/pins_shading_edges.npz) and against the CPU oracle, bit for bit
or NaN on both sides; the persistent shader's variants against the plain forms; and the disk point of the VNDF sampler — where the
device's double cos / sin stand in for glibc's — on 2^22 consecutive seeds."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
import shading_cases as sc
from test_shading_pins import GOLD, differing

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(os.path.join(ROOT, "raytracing-course-hw_amd", "librtamd_testhooks.so"))
    P = C.c_void_p
    L.rtt_brdf.argtypes = [C.c_int, P, P, C.c_size_t]
    L.rtt_vndf.argtypes = [C.c_int, P, P, P, P, C.c_size_t]
    L.rtt_cosine.argtypes = [P, P, P, P, C.c_size_t]
    for name in ("rtt_vndf_local", "rtt_vndf_pdf", "rtt_cosine_pdf", "rtt_tonemap"):
        getattr(L, name).argtypes = [P, P, C.c_size_t]
    L.rtt_disk_point.argtypes = [C.c_uint32, C.c_size_t, P, P, P]
    return L


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def run(fn, family, width, *head, dtype=F):
    """A hook of the form fn(*head, rows, out, n) on the rows of a family: out is n x width."""
    rows = sc.rows(family)
    out = np.zeros((len(rows), width) if width > 1 else len(rows), dtype)
    assert fn(*head, rows.ctypes.data, out.ctypes.data, len(rows)) == 0
    return out


def run_seeded(fn, family, *head):
    """A sampler hook fn(*head, seeds, rows, out5, state, n): the five outputs and the engine's state after the sample."""
    rows, seed = sc.rows(family), np.ascontiguousarray(sc.families()[family]["seed"], np.uint32)
    out, state = np.zeros((len(rows), 5), F), np.zeros(len(rows), np.uint32)
    assert fn(*head, seed.ctypes.data, rows.ctypes.data, out.ctypes.data, state.ctypes.data, len(rows)) == 0
    return out, state


def check(name, dev, want, against, family=None):
    bad = differing(dev, want)
    print(f"{name}: {len(want)} cases, {bad.size} differ from {against}")
    if bad.size:
        rows = sc.rows(family or name)
        for i in bad[:8]:
            print(f"  case {i}: in {[float(x).hex() for x in rows[i]]}\n    device {np.atleast_1d(dev[i]).tolist()} {against} {np.atleast_1d(want[i]).tolist()}")
    return bad.size


def test_brdf_equals_reference_and_oracle(hooks, gold):
    """material_brdf (hw8) and material_brdf_hw7 on the v.n / l.n gates (both sides, +-0, +-denormal), the 1e-4 gate to the bit, dotHN <= 0,
    l = -v, alpha down to 0."""
    o = sc.oracle_answers()
    dev8, dev7 = run(hooks.rtt_brdf, "brdf", 3, 0), run(hooks.rtt_brdf, "brdf_hw7", 3, 2)
    n_bad = check("brdf", dev8, gold["brdf"], "the reference") + check("brdf", dev8, o["brdf"], "the oracle")
    n_bad += check("brdf_hw7", dev7, gold["brdf_hw7"], "the reference") + check("brdf_hw7", dev7, o["brdf_hw7"], "the oracle")
    assert n_bad == 0


def test_brdf_with_products_formed_by_the_caller_is_the_plain_brdf(hooks):
    """material_brdf_pre, what the persistent shader runs, on bc = base_color * color and metallic * base_metallic formed on the device."""
    assert check("brdf", run(hooks.rtt_brdf, "brdf", 3, 1), run(hooks.rtt_brdf, "brdf", 3, 0), "material_brdf") == 0


def test_vndf_sample_and_pdf_equal_reference_and_oracle(hooks, gold):
    """vndf_sample then vndf_pdf of the sample: vndf_getq's three branches with n.z on +-0.9999 and its neighbours, lensq = 0, v in the
    surface and below it, normals a little off unit length; and the next uniform draw, the stream's position after the sampler."""
    dev, _ = run_seeded(hooks.rtt_vndf, "vndf", 0)
    assert check("vndf", dev, gold["vndf"], "the reference") + check("vndf", dev, sc.oracle_answers()["vndf"], "the oracle") == 0


def test_vndf_with_the_frame_given_is_the_plain_vndf(hooks):
    """vndf_sample(rng, q, vT, alpha) / vndf_pdf(q, vT, d, alpha) on the frame the persistent shader builds, engine state included."""
    plain, plain_state = run_seeded(hooks.rtt_vndf, "vndf", 0)
    framed, framed_state = run_seeded(hooks.rtt_vndf, "vndf", 1)
    assert check("vndf", framed, plain, "the plain form") == 0
    assert np.array_equal(framed_state, plain_state)


def test_vndf_pdf_equals_reference_and_oracle(hooks, gold):
    dev = run(hooks.rtt_vndf_pdf, "vndf_pdf", 1)
    assert check("vndf_pdf", dev, gold["vndf_pdf"], "the reference") + check("vndf_pdf", dev, sc.oracle_answers()["vndf_pdf"], "the oracle") == 0


def test_vndf_sample_local_equals_oracle(hooks):
    """Points no seed is known to reach: t1 = +-1, on the unit circle and an ulp beyond it (rem < 0), the centre; vT = +-z (lensq = 0),
    vT.z = +-0.  Vndf::sample_ is private in the reference, so the oracle — pinned through Vndf::sample — is the other side."""
    assert check("vndf_local", run(hooks.rtt_vndf_local, "vndf_local", 3), sc.oracle_answers()["vndf_local"], "the oracle") == 0


def test_cosine_sample_and_pdf_equal_reference_and_oracle(hooks, gold):
    """cosine_sample's three-way fallback (n = 0, a tiny n, a NaN in n, a length whose square overflows), cosine_pdf of the sample, the
    next uniform draw; and cosine_pdf at d.n = +-0, +-denormal, negative, NaN, infinite."""
    dev, _ = run_seeded(hooks.rtt_cosine, "cosine")
    n_bad = check("cosine", dev, gold["cosine"], "the reference") + check("cosine", dev, sc.oracle_answers()["cosine"], "the oracle")
    n_bad += check("cosine_pdf", run(hooks.rtt_cosine_pdf, "cosine_pdf", 1), sc.oracle_answers()["cosine_pdf"], "the oracle")
    assert n_bad == 0


def test_tonemap_equals_reference_and_oracle_at_every_byte_step(hooks, gold):
    """tonemap1 on the floats around each of the 255 places where the byte steps, and on NaN, infinities, -0, negatives, denormals and
    inputs whose square overflows in aces1."""
    dev = run(hooks.rtt_tonemap, "tonemap", 1, dtype=np.uint8)
    assert check("tonemap", dev, gold["tonemap"], "the reference") + check("tonemap", dev, sc.oracle_answers()["tonemap"], "the oracle") == 0


def _ulps(a, b):
    """|a - b| in units of b's last place, for doubles of one sign (cos / sin values that differ at all differ by a few)."""
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.where((ia < 0) == (ib < 0), np.abs(ia - ib), np.abs(ia & np.int64(0x7FFFFFFFFFFFFFFF)) + np.abs(ib & np.int64(0x7FFFFFFFFFFFFFFF)))


def test_disk_points_equal_the_host_libm_on_4m_seeds(hooks):
    """vndf_disk_point on seeds 0 .. 2^22 - 1: t1 = (float)((double)r * cos((double)phi)) and the sin form, with cos / sin from the
    host's glibc (rto_cos_array / rto_sin_array: what the reference calls) on the uniforms the device drew.  The device's double cos /
    sin come from its own libm; they may differ from glibc's in the last place, and the assertion is that no such difference survives
    the narrowing to float.  The census of the doubles is printed, not asserted."""
    n = 1 << 22
    u, t, cs = np.zeros((n, 2), F), np.zeros((n, 2), F), np.zeros((n, 2), np.float64)
    assert hooks.rtt_disk_point(0, n, u.ctypes.data, t.ctypes.data, cs.ctypes.data) == 0
    L = oracle_lib.lib()
    for name in ("rto_cos_array", "rto_sin_array"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        getattr(L, name).restype = None
    # the uniforms are the streams' first two draws (libstdc++'s generate_canonical on minstd: (x - 1) / 2^31)
    seed = np.arange(n, dtype=np.uint64)
    x0 = np.where(seed % 2147483647 == 0, 1, seed % 2147483647)
    x1 = x0 * 48271 % 2147483647
    x2 = x1 * 48271 % 2147483647
    canon = lambda x: np.minimum((x - 1).astype(F) * F(2.0 ** -31), np.nextafter(F(1), F(0)))
    assert np.array_equal(u[:, 0], canon(x1)) and np.array_equal(u[:, 1], canon(x2))
    r = np.sqrt(u[:, 0]).astype(np.float64)                                # (float)sqrt((double)u1): one correctly rounded root
    phi = np.ascontiguousarray((2.0 * np.pi * u[:, 1].astype(np.float64)).astype(F).astype(np.float64))
    host = np.zeros((n, 2), np.float64)
    hc, hs = np.zeros(n), np.zeros(n)
    L.rto_cos_array(phi.ctypes.data, hc.ctypes.data, n)
    L.rto_sin_array(phi.ctypes.data, hs.ctypes.data, n)
    host[:, 0], host[:, 1] = hc, hs
    want = (r[:, None] * host).astype(F)
    for k, name in enumerate(("cos", "sin")):
        d = _ulps(cs[:, k], host[:, k])
        print(f"device double {name} on {n} angles: {int((d != 0).sum())} differ from glibc's, by at most {int(d.max())} ulp")
    bad = np.flatnonzero((t.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    print(f"disk points: {n} seeds, {bad.size} differ from the host's after the narrowing")
    for i in bad[:16]:
        print(f"  seed {i}: u {[float(x).hex() for x in u[i]]} device t {[float(x).hex() for x in t[i]]} host t {[float(x).hex() for x in want[i]]}"
              f" device cos, sin {[float(x).hex() for x in cs[i]]} glibc {[float(x).hex() for x in host[i]]}")
    assert bad.size == 0

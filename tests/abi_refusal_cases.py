"""The calls the C-ABI must refuse, as a table, and run(): one line per case, `name, return code, rt_last_error()`.

tests/golden/abi_refusals_host.txt (HOST + NO_DEVICE, no GPU) and tests/golden/abi_refusals.txt (HOST + GPU, on a GPU) are this
module's output with the library as it was BEFORE its host layer was pulled together (one guard, one fan-out, one staging, one
checkpoint check); test_abi_refusals_host.py and test_gpu_abi_refusals.py compare line by line, so every return code and every
message a caller can provoke stays byte for byte.

Covered: every fail( site of rtamd_api.hip from accum_unsupported down, of rtamd_multi.hip and of rtamd_noise.hip whose condition a
caller can meet with the sphere scene (as hw8 and as hw6 scene), 16x16 and 8x8 frames, tile 8, 1-2 samples, device lists [0] and
[0, 0, 0] (more entries than tiles on the 8x8 frame), and the RTAMD_KERNEL knob.

Left out, and why:
  behind a failing HIP call -- the catch clauses of every entry point; the `shard push`, `hipSetDevice failed` and `stream / event
    creation failed` reports of the device threads; grow(); `rt_multi_accum_save/load: ` + the single accumulator's HIP failure
    (one entry); `rt_multi_noise_create: shard i: ` (rt_noise_create fails with a HIP error only); rt_multi_accum_load's MA_BREAK.
  behind a failed allocation or thread start -- the std::exception and `unknown exception` clauses.
  the launch-deadline and lost-path reports of collect_frame.
  the "broken" refusals (rt_accum_*, rt_multi_accum_*: MA_ENTER, rt_noise_* / rt_multi_noise_*: MN_ENTER, noise_snapshot and the
    two noise checks): an object is broken only after one of the above.
  unreachable, because the same check has refused earlier in the same call: accum_unsupported in check_frame under rt_accum_render
    (accum_check_slice asks first), resolve_tiles at the end of rt_multi_accum_create and `rt_multi_accum_load: ` + rt_accum_load's
    refusal with one entry (shard 0 has taken the same frame / the same blob), the per-shard `rt_accum_load has replaced the state`
    under rt_multi_noise_* (the rt_multi_accum's own count is looked at first).  `rt_multi_render: bad render parameters` could never
    be met either (one entry's picture has W*H*3 elements, never 0 for positive W and H); it went when the frame plan was shared.
  need a scene that is not the sphere scene (all in check_frame, which only moves under the guard): `sample_streams > 1 is
    implemented for HW6 / HW7 / HW8 only`, `hw3 ray_depth above`, `TRIANGLE figures`, `hw5 BVH deeper than 64`, `hw4 supports at
    most 32 emissive`, `the hw1 caster renders unsharded frames only` under rt_render (a .txt scene), and the Mega8 answer for a
    tree beyond the kernels' limits (here RTAMD_KERNEL=mega provokes it).
"""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE = os.path.join(ROOT, "tests", "golden", "scenes", "hw8_sphere", "sphere_emissive.gltf")
GOLDEN_HOST = os.path.join(ROOT, "tests", "golden", "abi_refusals_host.txt")
GOLDEN_GPU = os.path.join(ROOT, "tests", "golden", "abi_refusals.txt")
AH_MAGIC, AH_SAMPLES, AH_LIGHT_HASH = 0, 13, 16  # words of the checkpoint header (host/rt_accum_state.h)


class Ctx:
    """What the cases share: the binding, the scenes and the objects the sequences below build up."""

    def __init__(self, rt):
        self.rt, self.lib = rt, rt.lib
        self.out = C.c_void_p()
        self.buf = C.create_string_buffer(4096)

    def P(self, w=16, h=16, s=1, **kw):
        kw.setdefault("tile", 8)
        return self.rt.make_params(w, h, s, **kw)

    def summary(self, struct_size=None):
        s = self.rt.rt_noise_summary()
        s.struct_size = C.sizeof(s) if struct_size is None else struct_size
        return s


def _with(p, **fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _env(name, value, fn):
    def run(c):
        os.environ[name] = value  # putenv: the library reads its knobs at every call
        try:
            return fn(c)
        finally:
            del os.environ[name]
    return run


def _patched(blob, word, value):
    b = bytearray(blob)
    b[4 * word:4 * word + 4] = int(value).to_bytes(4, "little")
    return bytes(b)


# ---- no device needed ---------------------------------------------------------------------------------------------------------
HOST = [
    ("rt_render.null", lambda c: c.lib.rt_render(None, C.byref(c.P()), None, None, None)),
    ("rt_accum_create.null", lambda c: c.lib.rt_accum_create(None, C.byref(c.P()), C.byref(c.out))),
    ("rt_accum_samples.null", lambda c: c.lib.rt_accum_samples(None)),
    ("rt_accum_render.null", lambda c: c.lib.rt_accum_render(None, 1, None)),
    ("rt_accum_resolve.null", lambda c: c.lib.rt_accum_resolve(None, 0, None, None)),
    ("rt_accum_save.null", lambda c: c.lib.rt_accum_save(None, c.buf, 4096)),
    ("rt_accum_load.null", lambda c: c.lib.rt_accum_load(None, c.buf.raw, 4096)),
    ("rt_noise_create.null", lambda c: c.lib.rt_noise_create(None, C.byref(c.out))),
    ("rt_noise_reset.null", lambda c: c.lib.rt_noise_reset(None)),
    ("rt_noise_batches.null", lambda c: c.lib.rt_noise_batches(None)),
    ("rt_noise_update.null", lambda c: c.lib.rt_noise_update(None)),
    ("rt_noise_estimate.null", lambda c: c.lib.rt_noise_estimate(None, 0, None, None)),
    ("rt_noise_estimate.struct_size", lambda c: c.lib.rt_noise_estimate(None, 0, None, C.byref(c.summary(8)))),
    ("rt_multi_create.null_desc", lambda c: c.lib.rt_multi_create(None, None, 1, C.byref(c.out))),
    ("rt_multi_render.null", lambda c: c.lib.rt_multi_render(None, C.byref(c.P()), None, None, None)),
    ("rt_multi_accum_create.null", lambda c: c.lib.rt_multi_accum_create(None, C.byref(c.P()), C.byref(c.out))),
    ("rt_multi_accum_samples.null", lambda c: c.lib.rt_multi_accum_samples(None)),
    ("rt_multi_accum_render.null", lambda c: c.lib.rt_multi_accum_render(None, 1, None)),
    ("rt_multi_accum_resolve.null", lambda c: c.lib.rt_multi_accum_resolve(None, 0, None, None)),
    ("rt_multi_accum_save.null", lambda c: c.lib.rt_multi_accum_save(None, c.buf, 4096)),
    ("rt_multi_accum_load.null", lambda c: c.lib.rt_multi_accum_load(None, c.buf.raw, 4096)),
    ("rt_multi_noise_create.null", lambda c: c.lib.rt_multi_noise_create(None, C.byref(c.out))),
    ("rt_multi_noise_reset.null", lambda c: c.lib.rt_multi_noise_reset(None)),
    ("rt_multi_noise_batches.null", lambda c: c.lib.rt_multi_noise_batches(None)),
    ("rt_multi_noise_update.null", lambda c: c.lib.rt_multi_noise_update(None)),
    ("rt_multi_noise_estimate.null", lambda c: c.lib.rt_multi_noise_estimate(None, 0, None, None)),
    ("rt_multi_noise_estimate.struct_size", lambda c: c.lib.rt_multi_noise_estimate(None, 0, None, C.byref(c.summary(8)))),
    ("rt_accum_state_bytes.null", lambda c: c.lib.rt_accum_state_bytes(None)),
    ("rt_accum_state_bytes.struct_size", lambda c: c.lib.rt_accum_state_bytes(C.byref(_with(c.P(), struct_size=8)))),
    ("rt_accum_state_bytes.reserved", lambda c: c.lib.rt_accum_state_bytes(C.byref(_with(c.P(), reserved=1)))),
    ("rt_accum_state_bytes.hw3", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(integrator=3)))),
    ("rt_accum_state_bytes.width_0", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(w=0)))),
    ("rt_accum_state_bytes.too_large", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(w=65536, h=32768)))),
    ("rt_accum_state_bytes.ray_depth_17", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(ray_depth=17)))),
    ("rt_accum_state_bytes.hw6_ray_depth_9", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(integrator=6, ray_depth=9)))),
    ("rt_accum_state_bytes.shard_index", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(shard_index=2, shard_count=2)))),
    ("rt_accum_state_bytes.tile_12", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(shard_count=2, tile=12)))),
    ("rt_accum_state_bytes.slots", lambda c: c.lib.rt_accum_state_bytes(C.byref(c.P(w=32768, h=32768)))),
    ("rt_unshard.null", lambda c: c.lib.rt_unshard(C.byref(c.P()), None, 4, None)),
    ("rt_unshard.elem_size", lambda c: c.lib.rt_unshard(C.byref(c.P()), c.buf, 2, c.buf)),
    ("rt_unshard.width_0", lambda c: c.lib.rt_unshard(C.byref(c.P(w=0)), c.buf, 4, c.buf)),
    ("rt_unshard.tile_12", lambda c: c.lib.rt_unshard(C.byref(c.P(shard_count=2, tile=12)), c.buf, 4, c.buf)),
]
# rt_output_elems answers 0 and leaves no message
HOST_SILENT = [
    ("rt_output_elems.null", lambda c: c.lib.rt_output_elems(None)),
    ("rt_output_elems.width_0", lambda c: c.lib.rt_output_elems(C.byref(c.P(w=0)))),
    ("rt_output_elems.ray_depth_17", lambda c: c.lib.rt_output_elems(C.byref(c.P(ray_depth=17)))),
]


def _no_device_cases(c):
    sd = c.rt.load_gltf(SPHERE)
    dev = (C.c_int * 1)(0)
    return [
        ("nodevice.rt_scene_create", lambda c: c.lib.rt_scene_create(C.byref(sd.desc), C.byref(c.out))),
        ("nodevice.rt_multi_create", lambda c: c.lib.rt_multi_create(C.byref(sd.desc), dev, 1, C.byref(c.out))),
    ]


# ---- on a GPU -----------------------------------------------------------------------------------------------------------------
def _render(scene, P={}, **fields):
    return lambda c: c.lib.rt_render(getattr(c, scene)._h, C.byref(_with(c.P(**P), **fields)), None, None, None)


def _create(scene, P={}, **fields):
    return lambda c: c.lib.rt_accum_create(getattr(c, scene)._h, C.byref(_with(c.P(s=0, **P), **fields)), C.byref(c.out))


RENDER = [
    ("rt_render.null_params", lambda c: c.lib.rt_render(c.scene._h, None, None, None, None)),
    ("rt_render.struct_size", _render("scene", struct_size=8)),
    ("rt_render.integrator_0", _render("scene", integrator=0)),
    ("rt_render.integrator_9", _render("scene", integrator=9)),
    ("rt_render.flavor", _render("scene", integrator=6)),
    ("rt_render.flavor_hw6_scene", _render("scene6", integrator=8)),
    ("rt_render.width_0", _render("scene", P=dict(w=0))),
    ("rt_render.samples_0", _render("scene", P=dict(s=0))),
    ("rt_render.too_large", _render("scene", P=dict(w=65536, h=32768))),
    ("rt_render.ray_depth_17", _render("scene", P=dict(ray_depth=17))),
    ("rt_render.shard_index", _render("scene", P=dict(shard_index=2, shard_count=2))),
    ("rt_render.tile_12", _render("scene", P=dict(shard_count=2, tile=12))),
    ("rt_render.reserved", _render("scene", reserved=1)),
    ("rt_render.sample_seeds", _render("scene", flags=4)),
    ("rt_render.russian_roulette", _render("scene", flags=8)),
    ("rt_render.streams_3_of_4", _render("scene", P=dict(s=4, sample_streams=3))),
    ("rt_render.streams_257", _render("scene", P=dict(s=257, sample_streams=257))),
    ("rt_render.stream_seeds", _render("scene", P=dict(w=32768, h=32768, s=2, sample_streams=2))),
    ("rt_render.path_slots", _render("scene", P=dict(w=16384, h=16384, s=4, sample_streams=4))),
    ("rt_render.mega_streams", _env("RTAMD_KERNEL", "mega", _render("scene", P=dict(s=2, sample_streams=2)))),
    ("rt_render.hw6_ray_depth_9", _render("scene6", P=dict(integrator=6, ray_depth=9))),
    ("rt_render.hw6_sample_seeds", _render("scene6", P=dict(integrator=6, s=2, sample_streams=2, flags=4))),
    ("rt_accum_create.null_params", lambda c: c.lib.rt_accum_create(c.scene._h, None, C.byref(c.out))),
    ("rt_accum_create.null_out", lambda c: c.lib.rt_accum_create(c.scene._h, C.byref(c.P()), None)),
    ("rt_accum_create.streams", _create("scene", P=dict(sample_streams=2))),
    ("rt_accum_create.hw3", _create("scene", P=dict(integrator=3))),
    ("rt_accum_create.struct_size", _create("scene", struct_size=8)),
    ("rt_accum_create.reserved", _create("scene", reserved=1)),
    ("rt_accum_create.integrator_0", _create("scene", integrator=0)),
    ("rt_accum_create.width_0", _create("scene", P=dict(w=0))),
    ("rt_accum_create.too_large", _create("scene", P=dict(w=65536, h=32768))),
    ("rt_accum_create.ray_depth_17", _create("scene", P=dict(ray_depth=17))),
    ("rt_accum_create.hw6_ray_depth_9", _create("scene6", P=dict(integrator=6, ray_depth=9))),
    ("rt_accum_create.shard_index", _create("scene", P=dict(shard_index=2, shard_count=2))),
    ("rt_accum_create.tile_12", _create("scene", P=dict(shard_count=2, tile=12))),
    ("rt_accum_create.slots", _create("scene", P=dict(w=32768, h=32768))),
    ("rt_accum_create.flavor", _create("scene", P=dict(integrator=6))),
    ("rt_accum_create.flags", _create("scene", P=dict(flags=1))),
    ("rt_accum_create.mega", _env("RTAMD_KERNEL", "mega", _create("scene"))),
    ("rt_accum_create.mega_hw6", _env("RTAMD_KERNEL", "mega", _create("scene6", P=dict(integrator=6)))),
]


def _accum_cases(c):
    """One Accumulator of 16x16 and one of 8x8 on the single scene, a monitor on the first: the refusals in the order of a session."""
    lib = c.lib
    a16, a8 = c.scene.accumulator(16, 16), c.scene.accumulator(8, 8)
    mon = a16.noise_monitor()
    c.keep = [a16, a8, mon]
    h, n = a16._h, mon._h
    yield "rt_accum_render.n_0", lambda c: lib.rt_accum_render(h, 0, None)
    yield "rt_accum_render.n_negative", lambda c: lib.rt_accum_render(h, -3, None)
    yield "rt_accum_render.limit", lambda c: lib.rt_accum_render(h, 1 << 25, None)
    yield "rt_accum_render.mega", _env("RTAMD_KERNEL", "mega", lambda c: lib.rt_accum_render(h, 1, None))
    yield "rt_accum_resolve.flags", lambda c: lib.rt_accum_resolve(h, 2, None, None)
    yield "rt_accum_resolve.no_samples", lambda c: lib.rt_accum_resolve(h, 0, None, None)
    yield "rt_accum_save.null_blob", lambda c: lib.rt_accum_save(h, None, 4096)
    yield "rt_accum_save.small", lambda c: lib.rt_accum_save(h, c.buf, 100)
    yield "rt_noise_update.no_samples", lambda c: lib.rt_noise_update(n)
    yield "rt_noise_estimate.batches_0", lambda c: lib.rt_noise_estimate(n, 0, None, None)
    a16.render(1)
    mon.update()
    c.blob16 = blob = a16.save()
    yield "rt_noise_update.no_samples_since", lambda c: lib.rt_noise_update(n)
    yield "rt_noise_estimate.batches_1", lambda c: lib.rt_noise_estimate(n, 0, None, None)
    yield "rt_noise_estimate.flags", lambda c: lib.rt_noise_estimate(n, 2, None, None)
    yield "rt_noise_estimate.struct_size_live", lambda c: lib.rt_noise_estimate(n, 0, None, C.byref(c.summary(8)))
    yield "rt_accum_load.null_blob", lambda c: lib.rt_accum_load(h, None, len(blob))
    yield "rt_accum_load.short_header", lambda c: lib.rt_accum_load(h, blob, 64)
    yield "rt_accum_load.magic", lambda c: lib.rt_accum_load(h, _patched(blob, AH_MAGIC, 7), len(blob))
    yield "rt_accum_load.light_hash", lambda c: lib.rt_accum_load(h, _patched(blob, AH_LIGHT_HASH, 7), len(blob))
    yield "rt_accum_load.other_frame", lambda c: lib.rt_accum_load(a8._h, blob, len(blob))
    yield "rt_accum_load.samples_beyond", lambda c: lib.rt_accum_load(h, _patched(blob, AH_SAMPLES, 1 << 25), len(blob))
    yield "rt_accum_load.truncated", lambda c: lib.rt_accum_load(h, blob, len(blob) - 1)
    a16.load(blob)
    yield "rt_noise_update.after_load", lambda c: lib.rt_noise_update(n)
    yield "rt_noise_estimate.after_load", lambda c: lib.rt_noise_estimate(n, 0, None, None)


def _multi_create_cases(c):
    lib, desc = c.lib, c.sd.desc
    bad = c.rt.rt_scene_desc.from_buffer_copy(desc)
    bad.build_flags = 2
    c.keep.append(bad)
    ints = lambda *v: (C.c_int * len(v))(*v)
    yield "rt_multi_create.null_out", lambda c: lib.rt_multi_create(C.byref(desc), ints(0), 1, None)
    yield "rt_multi_create.devices_0", lambda c: lib.rt_multi_create(C.byref(desc), ints(0), 0, C.byref(c.out))
    yield "rt_multi_create.devices_65", lambda c: lib.rt_multi_create(C.byref(desc), ints(*[0] * 65), 65, C.byref(c.out))
    yield "rt_multi_create.device_99", lambda c: lib.rt_multi_create(C.byref(desc), ints(0, 99), 2, C.byref(c.out))
    yield "rt_multi_create.device_negative", lambda c: lib.rt_multi_create(C.byref(desc), ints(-1), 1, C.byref(c.out))
    yield "rt_multi_create.build_flags@1", lambda c: lib.rt_multi_create(C.byref(bad), ints(0), 1, C.byref(c.out))
    yield "rt_multi_create.build_flags@3", lambda c: lib.rt_multi_create(C.byref(bad), ints(0, 0, 0), 3, C.byref(c.out))


def _multi_cases(c, multi, tag):
    """The stateless refusals of one MultiScene."""
    lib, m = c.lib, multi._h
    P0 = lambda **kw: _with(c.P(**kw), shard_count=kw.get("shard_count", 0), shard_index=0)
    render = lambda p: (lambda c: lib.rt_multi_render(m, C.byref(p), None, None, None))
    create = lambda p: (lambda c: lib.rt_multi_accum_create(m, C.byref(p), C.byref(c.out)))
    yield f"rt_multi_render.null_params@{tag}", lambda c: lib.rt_multi_render(m, None, None, None, None)
    yield f"rt_multi_render.struct_size@{tag}", render(_with(P0(), struct_size=8))
    yield f"rt_multi_render.shard_count@{tag}", render(P0(shard_count=2))
    yield f"rt_multi_render.hw1@{tag}", render(P0(integrator=1))
    yield f"rt_multi_render.square_tiles@{tag}", render(_with(P0(), tile_h=16))
    yield f"rt_multi_render.width_0@{tag}", render(P0(w=0))
    yield f"rt_multi_render.samples_0@{tag}", render(P0(s=0))
    if tag == "1":  # one entry: the frame's own geometry is looked at here; with more it is each shard's business
        yield f"rt_multi_render.ray_depth_17@{tag}", render(P0(ray_depth=17))
        yield f"rt_multi_render.too_large@{tag}", render(P0(w=65536, h=32768))
    yield f"rt_multi_render.flavor@{tag}", render(P0(integrator=6))
    yield f"rt_multi_render.reserved@{tag}", render(_with(P0(), reserved=1))
    yield f"rt_multi_render.flavor_8x8@{tag}", render(P0(w=8, h=8, integrator=6))
    yield f"rt_multi_accum_create.null_params@{tag}", lambda c: lib.rt_multi_accum_create(m, None, C.byref(c.out))
    yield f"rt_multi_accum_create.null_out@{tag}", lambda c: lib.rt_multi_accum_create(m, C.byref(P0()), None)
    yield f"rt_multi_accum_create.struct_size@{tag}", create(_with(P0(), struct_size=8))
    yield f"rt_multi_accum_create.shard_count@{tag}", create(P0(shard_count=2))
    yield f"rt_multi_accum_create.square_tiles@{tag}", create(_with(P0(), tile_h=16))
    yield f"rt_multi_accum_create.width_0@{tag}", create(P0(w=0))
    yield f"rt_multi_accum_create.hw3@{tag}", create(P0(integrator=3))
    yield f"rt_multi_accum_create.flags@{tag}", create(P0(flags=1))
    yield f"rt_multi_accum_create.reserved@{tag}", create(_with(P0(), reserved=1))
    yield f"rt_multi_accum_create.mega@{tag}", _env("RTAMD_KERNEL", "mega", create(P0()))


def _multi_accum_cases(c, multi, size, tag):
    """A MultiAccumulator of size x size with a monitor, through a session; c.blob16 is the 16x16 frame's checkpoint after one sample."""
    lib = c.lib
    acc = multi.accumulator(size, size, tile=8)
    mon = acc.noise_monitor()
    c.keep += [acc, mon]
    a, n, tag = acc._h, mon._h, f"{size}x{size}@{tag}"
    yield f"rt_multi_accum_render.n_0.{tag}", lambda c: lib.rt_multi_accum_render(a, 0, None)
    yield f"rt_multi_accum_render.limit.{tag}", lambda c: lib.rt_multi_accum_render(a, 1 << 25, None)
    yield f"rt_multi_accum_render.mega.{tag}", _env("RTAMD_KERNEL", "mega", lambda c: lib.rt_multi_accum_render(a, 1, None))
    yield f"rt_multi_accum_resolve.flags.{tag}", lambda c: lib.rt_multi_accum_resolve(a, 2, None, None)
    yield f"rt_multi_accum_resolve.no_samples.{tag}", lambda c: lib.rt_multi_accum_resolve(a, 0, None, None)
    yield f"rt_multi_accum_save.null_blob.{tag}", lambda c: lib.rt_multi_accum_save(a, None, 4096)
    yield f"rt_multi_accum_save.small.{tag}", lambda c: lib.rt_multi_accum_save(a, c.buf, 100)
    yield f"rt_multi_noise_update.no_samples.{tag}", lambda c: lib.rt_multi_noise_update(n)
    yield f"rt_multi_noise_estimate.batches_0.{tag}", lambda c: lib.rt_multi_noise_estimate(n, 0, None, None)
    acc.render(1)
    mon.update()
    blob = acc.save()
    other = c.blob16 if size == 8 else c.blob8
    yield f"rt_multi_noise_update.no_samples_since.{tag}", lambda c: lib.rt_multi_noise_update(n)
    yield f"rt_multi_noise_estimate.batches_1.{tag}", lambda c: lib.rt_multi_noise_estimate(n, 0, None, None)
    yield f"rt_multi_noise_estimate.flags.{tag}", lambda c: lib.rt_multi_noise_estimate(n, 1, None, None)
    yield f"rt_multi_noise_estimate.struct_size_live.{tag}", lambda c: lib.rt_multi_noise_estimate(n, 0, None, C.byref(c.summary(8)))
    yield f"rt_multi_accum_load.null_blob.{tag}", lambda c: lib.rt_multi_accum_load(a, None, len(blob))
    yield f"rt_multi_accum_load.short_header.{tag}", lambda c: lib.rt_multi_accum_load(a, blob, 64)
    yield f"rt_multi_accum_load.magic.{tag}", lambda c: lib.rt_multi_accum_load(a, _patched(blob, AH_MAGIC, 7), len(blob))
    yield f"rt_multi_accum_load.other_frame.{tag}", lambda c: lib.rt_multi_accum_load(a, other, len(other))
    yield f"rt_multi_accum_load.samples_beyond.{tag}", lambda c: lib.rt_multi_accum_load(a, _patched(blob, AH_SAMPLES, 1 << 25), len(blob))
    yield f"rt_multi_accum_load.truncated.{tag}", lambda c: lib.rt_multi_accum_load(a, blob, len(blob) - 1)
    acc.load(blob)
    yield f"rt_multi_noise_update.after_load.{tag}", lambda c: lib.rt_multi_noise_update(n)
    yield f"rt_multi_noise_estimate.after_load.{tag}", lambda c: lib.rt_multi_noise_estimate(n, 0, None, None)


def _line(c, name, fn, silent=False):
    rc = fn(c)
    return f"{name}, {rc}, " + ("-" if silent else c.lib.rt_last_error().decode("utf-8", "replace"))


def run_host(rt, no_device):
    """The lines of HOST (+ the no-device answers when `no_device`): no GPU is touched unless one is there and asked for."""
    c = Ctx(rt)
    lines = [_line(c, name, fn) for name, fn in HOST] + [_line(c, name, fn, silent=True) for name, fn in HOST_SILENT]
    if no_device:
        lines += [_line(c, name, fn) for name, fn in _no_device_cases(c)]
    return lines


def run_gpu(rt):
    """The lines of the cases that need live objects, on device 0."""
    c = Ctx(rt)
    c.keep = []
    c.sd = rt.load_gltf(SPHERE)
    c.scene, c.scene6 = rt.Scene(c.sd), rt.Scene(rt.load_gltf(SPHERE, flavor=rt.RT_INTEGRATOR_HW6))
    lines = [_line(c, name, fn) for name, fn in RENDER]
    lines += [_line(c, name, fn) for name, fn in _accum_cases(c)]
    a8 = c.scene.accumulator(8, 8)
    a8.render(1)
    c.blob8 = a8.save()
    a8.close()
    lines += [_line(c, name, fn) for name, fn in _multi_create_cases(c)]
    for devices, tag in (([0], "1"), ([0, 0, 0], "3")):
        multi = rt.MultiScene(c.sd, devices)
        lines += [_line(c, name, fn) for name, fn in _multi_cases(c, multi, tag)]
        for size in (16, 8):
            lines += [_line(c, name, fn) for name, fn in _multi_accum_cases(c, multi, size, tag)]
        multi.close()
    c.scene.close()
    c.scene6.close()
    return lines


if __name__ == "__main__":  # python tests/abi_refusal_cases.py host|gpu FILE: writes the transcript
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    rt = importlib.import_module("raytracing-course-hw_amd")
    lines = run_host(rt, rt.lib.rt_device_count() == 0) if sys.argv[1] == "host" else run_host(rt, False) + run_gpu(rt)
    with open(sys.argv[2], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {sys.argv[2]}")

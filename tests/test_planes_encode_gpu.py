"""Planar float tensors straight to block textures and Hap frames (HapGpuCompressPlanes, HapGpuEncodeFramesPlanes[Begin]).
The definition is exact: byte = quantise(float32(element) * float32(scale[c]) + float32(bias[c])) -- two roundings, NaN
and anything not above 0 to 0, 255 and above to 255, else to nearest with halves to even --, and the textures and frames
are those of the RGBA8 picture of these bytes.  Every expected value is computed on the CPU: numpy for the quantiser
(tests/_planes_encode.py), the checker's block encoder (tests/_data.oracle_bc_encode) for textures, the checker's frame
decoder (tests/_libs.oracle_api) for frames.  Every comparison is on bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import _data as D
import _libs as L
import _planes_encode as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
ORACLE = L.oracle_api()
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "rgtc1": L.FMT_RGTC1}
# one lane; two lanes either way; exactly one wave a row; a second wave of one lane; a ninth wave
GEOMETRIES = ((4, 4), (8, 4), (4, 8), (256, 8), (260, 12), (516, 12))
KINDS = {"f16": (torch.float16, P.F16, 2), "bf16": (torch.bfloat16, P.BF16, 2), "f32": (torch.float32, P.F32, 4)}
STD = P.IMAGENET_STD + (1.0,)
MEAN = P.IMAGENET_MEAN + (0.0,)
CONSTANTS = {
    "bytes": ((255.0,) * 4, (0.0,) * 4),
    "signed": ((127.5,) * 4, (127.5,) * 4),
    "imagenet": (tuple(float(np.float32(255.0 * s)) for s in STD), tuple(float(np.float32(255.0 * m)) for m in MEAN)),
}


@pytest.fixture(scope="module")
def hap():
    import hap_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hap_amd


@pytest.fixture(scope="module")
def ctx(hap):
    c = hap.Context(0)
    yield c
    c.close()


def host(t):
    return t.cpu().numpy()


def filled(n, where="cuda"):
    t = torch.full((n,), SENTINEL, dtype=torch.uint8, device=where)
    if where == "cuda":
        torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def random_elements(kind, constants, channels, h, w, seed=0):
    """A (channels, h, w) CPU tensor of `kind`: seeded random bytes spread by the inverse of the constants, plus noise
    below half a step; and the float32 values its elements have.  Made once."""
    scale, bias = CONSTANTS[constants]
    rng = np.random.default_rng([sorted(KINDS).index(kind), sorted(CONSTANTS).index(constants), channels, h, w, seed])
    x = np.empty((channels, h, w), dtype=np.float64)
    for c in range(channels):
        b = rng.integers(0, 256, (h, w)).astype(np.float64) + rng.uniform(-0.45, 0.45, (h, w))
        x[c] = (b - bias[c]) / scale[c]
    t = torch.from_numpy(x.astype(np.float32)).to(KINDS[kind][0]).contiguous()
    values = t.to(torch.float32).numpy()                       # (exact for all three kinds)
    values.setflags(write=False)
    return t, values


def placed(t, row=None, plane=None, first=0):
    """The CPU tensor `t` (channels, h, w) on the device: `first` elements into a buffer, rows `row` and planes `plane`
    elements apart (None: packed)"""
    channels, h, w = t.shape
    row = row or w
    plane = plane or row * h
    flat = torch.zeros(first + channels * plane + 8, dtype=t.dtype, device="cuda")
    view = torch.as_strided(flat[first:], (channels, h, w), (plane, row, 1))
    view.copy_(t)
    torch.cuda.synchronize()
    return view


def picture(values, constants):
    scale, bias = CONSTANTS[constants] if isinstance(constants, str) else constants
    return P.picture_of(values, scale, bias)


def texture_bytes(w, h, fmts):
    return [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]


# -------------------------------------------------------------------------------------------------------- 1. textures --
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_textures_are_the_checkers_of_the_tensors_picture(ctx, name, kind):
    fmt = FORMATS[name]
    e = KINDS[kind][2]
    calls = 0
    for constants in sorted(CONSTANTS):
        scale, bias = CONSTANTS[constants]
        for channels in (3, 4):
            for w, h in GEOMETRIES:
                t, values = random_elements(kind, constants, channels, h, w)
                want = D.oracle_bc_encode(picture(values, constants), fmt)
                # packed, and as a slice of a larger tensor: longer rows, longer planes, a first element 4 * e bytes in
                for layout in (dict(), dict(row=w + 8, plane=(w + 8) * (h + 3), first=4)):
                    src = placed(t, **layout)
                    assert src.data_ptr() % (4 * e) == 0
                    where = ("cuda", "cpu")[calls % 2]
                    out = filled(len(want) + 64, where)
                    r, used = ctx.compress_planes(src, w, h, fmt, scale=scale[:channels], bias=bias[:channels],
                                                  output=out[: len(want)])
                    note = (constants, channels, w, h, sorted(layout), where)
                    assert (r, used) == (0, len(want)), note
                    got = host(out)
                    assert got[: len(want)].tobytes() == want, note
                    assert (got[len(want):] == SENTINEL).all(), note
                    calls += 1
    print(f"{name} {kind}: {calls} textures equal to the checker's")


def test_the_defaults_and_a_short_output(ctx, hap):
    w, h = 8, 8
    t, values = random_elements("f16", "bytes", 4, h, w)
    src = placed(t)
    r, tex = ctx.compress_planes(src, w, h, L.FMT_DXT5)                              # scale=None: 255, bias=None: 0
    assert r == 0 and tex == D.oracle_bc_encode(picture(values, "bytes"), L.FMT_DXT5)
    out = filled(128)
    assert ctx.compress_planes(src, w, h, L.FMT_DXT5, output=out[:63])[0] == hap.HapResult.Buffer_Too_Small
    assert ctx.compress_planes(src, w, h, L.FMT_BC7, output=out[:64])[0] == hap.HapResult.Bad_Arguments
    assert (host(out) == SENTINEL).all()


# ------------------------------------------------------------------------------ 2. every element pattern on the device --
@functools.lru_cache(maxsize=None)
def constant_blocks(fmt):
    """The checker's block of a 4 x 4 block whose sixteen texels are (v, v, v, v), for v = 0 .. 255"""
    pic = np.repeat(np.arange(256, dtype=np.uint8), 4)[None, :, None] * np.ones((4, 1, 4), dtype=np.uint8)
    raw = np.frombuffer(D.oracle_bc_encode(np.ascontiguousarray(pic), fmt), dtype=np.uint8)
    return raw.reshape(256, D.BLOCK_BYTES[fmt]).copy()


def test_a_constant_block_carries_its_byte():
    """What the sweep below rests on: 256 distinct blocks, the byte in the open -- and why DXT1 is not the carrier"""
    a, y, d = constant_blocks(L.FMT_RGTC1), constant_blocks(L.FMT_YCOCG), constant_blocks(L.FMT_DXT1)
    assert len({b.tobytes() for b in a}) == 256 and len({b.tobytes() for b in y}) == 256
    assert (a[:, 0] == np.arange(256)).all() and (a[:, 1] == np.arange(256)).all()
    assert (y[:, 0] == np.arange(256)).all() and (y[:, 1] == np.arange(256)).all()          # Y = v
    assert len({b.tobytes() for b in d}) < 256


SWEEPS = {"f16": np.arange(65536, dtype=np.uint16), "bf16": np.arange(65536, dtype=np.uint16),
          "f32": P.float_set()[:65536]}
SWEEP_CONSTANTS = {"255": (255.0, 0.0), "1": (1.0, 0.0), "2^24": (float(2 ** 24), 0.0)}


@pytest.mark.parametrize("constants", list(SWEEP_CONSTANTS))
@pytest.mark.parametrize("kind", list(SWEEPS))
def test_every_pattern_through_the_devices_quantiser(ctx, hap, kind, constants):
    """A 1024 x 1024 tensor of four identical planes in which block i holds pattern i in all 16 texels: the device's
    conversions, multiply, add, rounding and clamps for every half, every bfloat16 and the float set"""
    dtype, element, e = KINDS[kind]
    bits = SWEEPS[kind]
    assert bits.size == 65536
    scale, bias = SWEEP_CONSTANTS[constants]
    v = P.quantise(P.values_of(element, bits), scale, bias)
    if kind == "f16" and constants == "2^24":
        assert (v[1:256] == np.arange(1, 256)).all() and (v[256:1024] == 255).all()     # subnormal halves: not flushed
    plane = np.repeat(np.repeat(bits.reshape(256, 256), 4, axis=0), 4, axis=1)
    signed = plane.view(np.int16 if e == 2 else np.int32)
    tensor = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(signed, (4, 1024, 1024)))).cuda().view(dtype)
    torch.cuda.synchronize()
    w = h = 1024
    want = {f: constant_blocks(f)[v].tobytes() for f in (L.FMT_YCOCG, L.FMT_RGTC1)}
    # both textures through the frames call
    fmts = [L.FMT_YCOCG, L.FMT_RGTC1]
    sizes = texture_bytes(w, h, fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [1, 1])
    out = filled(cap)
    r, used, res = ctx.encode_frames_planes(tensor[None], w, h, fmts, [L.COMP_NONE] * 2, [1, 1], [out],
                                            scale=[scale] * 4, bias=[bias] * 4)
    assert r == 0 and res == [0], (r, res)
    frame = host(out)[: used[0]].tobytes()
    for i, f in enumerate(fmts):
        rr, tex, fmt = ORACLE.decode(frame, i, out_bytes=sizes[i])
        assert (rr, fmt) == (0, f)
        bad = np.nonzero((np.frombuffer(tex, np.uint8).reshape(65536, -1) != np.frombuffer(want[f], np.uint8).reshape(65536, -1)).any(axis=1))[0]
        assert bad.size == 0, (f, [(hex(int(bits[k])), int(v[k])) for k in bad[:8]])
    # ... and the alpha plane alone through the texture call
    r, tex = ctx.compress_planes(tensor, w, h, L.FMT_RGTC1, scale=[scale] * 4, bias=[bias] * 4)
    assert r == 0 and tex == want[L.FMT_RGTC1]


# ---------------------------------------------------------------------------------------------------------- 3. frames --
FLAVOURS = {"hap": [L.FMT_DXT1], "hap_alpha": [L.FMT_DXT5], "hap_q": [L.FMT_YCOCG], "hap_q_alpha": [L.FMT_YCOCG, L.FMT_RGTC1],
            "alpha_only": [L.FMT_RGTC1]}
FRAME_GEOMETRIES = ((64, 32), (260, 12))


def smooth_elements(kind, channels, n, h, w):
    """n tensors (CPU) that compress: the project's synthetic pictures as elements in 0 .. 1, and their values"""
    pics = np.stack([D.rgba(w, h, f) for f in range(n)])                                   # (n, h, w, 4)
    x = pics.transpose(0, 3, 1, 2)[:, :channels].astype(np.float32) / np.float32(255.0)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(KINDS[kind][0])
    return t, t.to(torch.float32).numpy()


def rgba_call(ctx, pictures, w, h, fmts, comps, chunks, cap, flags):
    """HapGpuEncodeFramesRGBA of the pictures (uploaded): (used, [frames])"""
    pics = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures]
    outs = [filled(cap) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba(pics, w, h, w * 4, fmts, comps, chunks, outs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return used, [host(o)[:u].tobytes() for o, u in zip(outs, used)]


@pytest.mark.parametrize("size", FRAME_GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_frames_equal_the_rgba_calls_and_the_checkers_textures(ctx, hap, flavour, size):
    w, h = size
    fmts = FLAVOURS[flavour]
    count, n = len(fmts), 3
    sizes = texture_bytes(w, h, fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [max(2, hap.fine_chunk_count(b, f)) for b, f in zip(sizes, fmts)]) + 4096
    combo = 0
    for flags in (0, hap.ENCODE_FRAGMENT_INDEX, hap.ENCODE_FINE_CHUNKS):
        for comp in (L.COMP_SNAPPY, L.COMP_NONE):
            kind = sorted(KINDS)[combo % 3]
            channels = 3 + (combo // 3) % 2
            t, values = smooth_elements(kind, channels, n, h, w)
            pictures = [picture(values[f], ((255.0,) * 4, (0.0,) * 4)) for f in range(n)]
            comps, chunks = [comp] * count, [2] * count
            want_used, want = rgba_call(ctx, pictures, w, h, fmts, comps, chunks, cap, flags)
            tensor = t.cuda()
            outs = [filled(cap + 64) for _ in range(n)]
            r, used, res = ctx.encode_frames_planes(tensor, w, h, fmts, comps, chunks, [o[:cap] for o in outs], flags=flags)
            note = (flags, comp, kind, channels)
            assert r == 0 and res == [0] * n and used == want_used, (note, r, res, used, want_used)
            got = [host(o) for o in outs]
            assert all((g[cap:] == SENTINEL).all() for g in got), note
            got = [g[:u].tobytes() for g, u in zip(got, used)]
            assert got == want, note
            # the checker reads its own block encoder's textures out of them
            for f in (0, n - 1):
                for i, fmt in enumerate(fmts):
                    rr, tex, ff = ORACLE.decode(got[f], i, out_bytes=sizes[i])
                    assert (rr, ff) == (0, fmt) and tex == D.oracle_bc_encode(pictures[f], fmt), (note, f, i)
            # the two halves give what the one call gives; between them the context takes no other call
            outs2 = [filled(cap) for _ in range(n)]
            assert ctx.encode_frames_planes_begin(tensor, w, h, fmts, comps, chunks, outs2, flags=flags) == 0, note
            if combo == 0:
                r3, _used3, res3 = ctx.encode_frames_planes(tensor, w, h, fmts, comps, chunks, [filled(cap) for _ in range(n)])
                assert r3 == hap.HapResult.Internal_Error and res3 == [hap.HapResult.Internal_Error] * n
                assert ctx.compress_planes(tensor[0], w, h, fmts[0])[0] == hap.HapResult.Internal_Error
            r2, used2, res2 = ctx.encode_finish()
            assert r2 == 0 and res2 == [0] * n and used2 == want_used, note
            assert [host(o)[:u].tobytes() for o, u in zip(outs2, used2)] == want, note
            combo += 1


@pytest.mark.parametrize("content", ("smooth", "noise"))
def test_a_batch_large_enough_to_be_placed(hap, content):
    """Nine frames with the fragment table and room in their buffers: the second stage writes fragments where they belong
    in the frame, and frames of noise, whose chunks do not shrink, are encoded a second time -- from the tensors again.
    (A context of its own, the planar call first: a call that encodes most frames twice makes the next ones gather.)"""
    w, h, n = 256, 64, 9
    fmts = [L.FMT_YCOCG]
    sizes = texture_bytes(w, h, fmts)
    cap = 2 * hap.HapMaxEncodedLength(sizes, fmts, [2]) + 65536
    ctx = hap.Context(0)
    if content == "smooth":
        t, values = smooth_elements("bf16", 3, n, h, w)
        constants = ((255.0,) * 4, (0.0,) * 4)
    else:
        parts = [random_elements("f32", "imagenet", 3, h, w, seed=f) for f in range(n)]
        t, values = torch.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        constants = CONSTANTS["imagenet"]
    pictures = [picture(values[f], constants) for f in range(n)]
    outs = [filled(cap) for _ in range(n)]
    r, used, res = ctx.encode_frames_planes(t.cuda(), w, h, fmts, [L.COMP_SNAPPY], [2], outs, scale=constants[0][:3],
                                            bias=constants[1][:3], flags=hap.ENCODE_FRAGMENT_INDEX)
    again = ctx.placement_retries()
    print(f"{content}: {again} of {n} frames encoded a second time")
    assert r == 0 and res == [0] * n
    assert (again > 0) == (content == "noise")
    want_used, want = rgba_call(ctx, pictures, w, h, fmts, [L.COMP_SNAPPY], [2], cap, hap.ENCODE_FRAGMENT_INDEX)
    ctx.close()
    assert used == want_used
    assert [host(o)[:u].tobytes() for o, u in zip(outs, used)] == want


# ----------------------------------------------------------------------------------------------- 4. per-frame refusal --
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_tensor_that_cannot_be_read_fails_alone(ctx, hap, kind):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    w, h, channels = 64, 32, 4
    dtype, element, e = KINDS[kind]
    t, values = smooth_elements(kind, channels, 1, h, w)
    good = placed(t[0])
    shifted = placed(t[0], first=1)                            # misaligned by one element
    assert shifted.data_ptr() % (4 * e) == e
    on_host = t[0].contiguous()
    fmts = [L.FMT_YCOCG, L.FMT_RGTC1]
    sizes = texture_bytes(w, h, fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [2, 2]) + 4096
    pictures = [picture(values[0], ((255.0,) * 4, (0.0,) * 4))]
    want_used, want = rgba_call(ctx, pictures, w, h, fmts, [L.COMP_SNAPPY] * 2, [2, 2], cap, 0)
    for order in ((None, "host", "shifted", "good"), ("good", "shifted", None, "host")):
        tensors = {None: None, "host": on_host.data_ptr(), "shifted": shifted.data_ptr(), "good": good.data_ptr()}
        outs = [filled(cap) for _ in order]
        ptrs = (C.c_void_p * 4)(*[tensors[k] for k in order])
        optrs = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
        caps = (C.c_ulong * 4)(*([cap] * 4))
        used = (C.c_ulong * 4)(*([7] * 4))
        res = (C.c_uint * 4)(*([99] * 4))
        two = (C.c_uint * 2)
        r = lib.HapGpuEncodeFramesPlanes(ctx.handle, 4, ptrs, channels, element, w * h * e, w * e, (C.c_float * 4)(*([255.0] * 4)),
                                         (C.c_float * 4)(), w, h, 2, two(*fmts), two(L.COMP_SNAPPY, L.COMP_SNAPPY), two(2, 2),
                                         optrs, caps, used, res, 0)
        assert r == bad, order                                 # the first failure
        for k, o in zip(order, outs):
            f = order.index(k)
            if k == "good":
                assert res[f] == 0 and used[f] == want_used[0] and host(o)[: used[f]].tobytes() == want[0], order
            else:
                assert res[f] == bad and (host(o) == SENTINEL).all(), (order, k)


# -------------------------------------------------------------------------------- 5. round trip across the two roads --
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_decoded_planes_encode_to_what_the_transcoder_makes(ctx, hap, kind):
    """Hap Q frames -> planes (1/255, 0) -> Hap frames (255, 0) is the transcoder's Hap Q -> Hap: every byte comes back
    through every element kind, and the transcoder is defined as encode of decode"""
    w, h, n = 64, 32, 3
    pics = [torch.from_numpy(D.rgba(w, h, f)).cuda() for f in range(n)]
    src_sizes = texture_bytes(w, h, [L.FMT_YCOCG])
    cap = hap.HapMaxEncodedLength(src_sizes, [L.FMT_YCOCG], [2]) + 4096
    outs = [filled(cap) for _ in range(n)]
    r, lens, res = ctx.encode_frames_rgba(pics, w, h, w * 4, [L.FMT_YCOCG], [L.COMP_SNAPPY], [2], outs)
    assert r == 0 and res == [0] * n
    frames = [o[:u] for o, u in zip(outs, lens)]
    dst_sizes = texture_bytes(w, h, [L.FMT_DXT1])
    dcap = hap.HapMaxEncodedLength(dst_sizes, [L.FMT_DXT1], [2]) + 4096
    direct = [filled(dcap) for _ in range(n)]
    r, want_used, res = ctx.transcode_frames(frames, lens, 1, w, h, 0, [L.FMT_DXT1], [L.COMP_SNAPPY], [2], direct)
    assert r == 0 and res == [0] * n
    planes = torch.zeros((n, 3, h, w), dtype=KINDS[kind][0], device="cuda")
    r, res = ctx.decode_frames_planes(frames, lens, 1, planes, w, h)                     # 1 / 255, 0
    assert r == 0 and res == [0] * n
    back = [filled(dcap) for _ in range(n)]
    r, used, res = ctx.encode_frames_planes(planes, w, h, [L.FMT_DXT1], [L.COMP_SNAPPY], [2], back)     # 255, 0
    assert r == 0 and res == [0] * n and used == want_used
    for f in range(n):
        assert host(back[f])[: used[f]].tobytes() == host(direct[f])[: used[f]].tobytes(), f

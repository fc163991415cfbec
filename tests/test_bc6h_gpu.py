"""Hap HDR (BC6H) to RGBA16F pictures on the GPU: HapGpuDecompressRGBAHalf and HapGpuDecodeFramesRGBAHalf, bit-exact
(uint16 half bit patterns) with the CPU reference of tests/_bc6h.py (itself pinned to Pillow and to hand-worked blocks
by tests/test_bc6h_reference.py)."""
import numpy as np
import pytest

import _bc6h as B
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
REF = L.ref_api() or ORA
FORMATS = [(L.FMT_BC6U, False), (L.FMT_BC6S, True)]


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


def texture(nblocks, seed):
    """A Hap HDR texture that Snappy can shrink: blocks of the generated sets (every mode, reserved ones included) and
    random blocks, each repeated a few times."""
    sets = B.block_sets()
    pool = sets["mixed_u"] + sets["mixed_s"]
    pool = [pool[i:i + 16] for i in range(0, len(pool), 16)]
    rng = B.SplitMix64(seed)
    out = []
    while len(out) < nblocks:
        blk = pool[rng.next() % len(pool)] if rng.next() % 4 else rng.bits(128).to_bytes(16, "little")
        out.extend([blk] * (1 + rng.next() % 4))
    return b"".join(out[:nblocks])


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def picture(buf, w, h, stride=None):
    """uint16 [h, w, 4] of a picture held in bytes, numpy or torch (host or device), rows `stride` bytes apart."""
    if hasattr(buf, "cpu"):
        buf = buf.cpu().contiguous().view(torch.uint8).numpy()
    if isinstance(buf, (bytes, bytearray)):
        buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    a = np.asarray(buf).view(np.uint8).reshape(-1)
    stride = stride or w * 8
    return a[: h * stride].reshape(h, stride)[:, : w * 8].copy().view(np.uint16).reshape(h, w, 4)


def guard_ok(buf, w, h, stride, fill=0xEE):
    a = buf.cpu().view(torch.uint8).numpy() if hasattr(buf, "cpu") else np.asarray(buf).view(np.uint8).reshape(-1)
    rows = a[: h * stride].reshape(h, stride)
    return bool((rows[:, w * 8:] == fill).all() and (a[(h - 1) * stride + w * 8:] == fill).all())


# ------------------------------------------------------------ HapGpuDecompressRGBAHalf --
@pytest.mark.parametrize("fmt,signed", FORMATS)
def test_every_block_set_decodes_bit_exactly(ctx, fmt, signed):
    for name, data in B.block_sets().items():
        w, h = B.geometry(len(data) // 16)
        r, got = ctx.decompress_rgba_half(data, fmt, w, h)
        assert r == 0, name
        assert np.array_equal(picture(got, w, h), B.decode(data, w, h, signed)), name


@pytest.mark.parametrize("fmt,signed", FORMATS)
@pytest.mark.parametrize("size", [(4, 4), (260, 36), (1024, 256)])
def test_host_and_device_textures_and_pictures(ctx, size, fmt, signed):
    w, h = size
    nb = (w // 4) * (h // 4)
    data = texture(nb, 0x1000 + w) if nb > 1 else B.block_sets()["mode0b_s"][:16]
    want = B.decode(data, w, h, signed)
    dtex = dev(data)
    # host or device texture, host picture
    for tex in (data, dtex):
        r, got = ctx.decompress_rgba_half(tex, fmt, w, h)
        assert r == 0 and np.array_equal(picture(got, w, h), want)
    # into host and device pictures, tight and with 64 guard bytes after every row
    for tex in (data, dtex):
        for stride in (w * 8, w * 8 + 64):
            hout = np.full(h * stride + 256, 0xEE, dtype=np.uint8)
            r, _ = ctx.decompress_rgba_half(tex, fmt, w, h, out=hout, row_bytes=stride)
            assert r == 0 and np.array_equal(picture(hout, w, h, stride), want) and guard_ok(hout, w, h, stride)
            dout = torch.full((h * stride + 256,), 0xEE, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r, _ = ctx.decompress_rgba_half(tex, fmt, w, h, out=dout, row_bytes=stride)
            assert r == 0 and np.array_equal(picture(dout, w, h, stride), want) and guard_ok(dout, w, h, stride)
    # a torch.float16 (H, W, 4) CUDA tensor is a picture
    t = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    r, _ = ctx.decompress_rgba_half(dtex, fmt, w, h, out=t)
    assert r == 0 and np.array_equal(t.cpu().numpy().view(np.uint16), want)


def test_bad_arguments(ctx, hap):
    w, h = 64, 16
    data = texture((w // 4) * (h // 4), 7)
    big = dev(data + bytes(64))
    out = torch.zeros(w * h * 8 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = hap.HapResult.Bad_Arguments
    fmt = L.FMT_BC6U
    assert ctx.decompress_rgba_half(big[8: 8 + len(data)], fmt, w, h, out=out)[0] == bad        # misaligned texture
    assert ctx.decompress_rgba_half(big[16: 16 + len(data)], fmt, w, h, out=out)[0] == 0        # (aligned: fine)
    assert ctx.decompress_rgba_half(data, fmt, w, h, out=out[8:])[0] == bad                     # misaligned picture
    assert ctx.decompress_rgba_half(data[:-16], fmt, w, h)[0] == bad                            # short texture
    for other in (L.FMT_DXT5, L.FMT_BC7, L.FMT_YCOCG, L.FMT_DXT1, L.FMT_RGTC1):
        assert ctx.decompress_rgba_half(data, other, w, h)[0] == bad, other
    assert ctx.decompress_rgba_half(data, fmt, w, h, out=out, row_bytes=w * 8 - 16)[0] == bad   # rows too short
    assert ctx.decompress_rgba_half(data, fmt, w, h, out=out, row_bytes=w * 8 + 8)[0] == bad    # not a multiple of 16
    assert ctx.decompress_rgba_half(data, fmt, w, h - 2)[0] == bad                              # not a multiple of 4


# ------------------------------------------------------------ HapGpuDecodeFramesRGBAHalf --
W, H = 512, 256
NB = (W // 4) * (H // 4)


def hap_hdr_frames(ctx, hap, tex, fmt):
    """Hap HDR frames of the texture from every encoder road: (name, frame bytes)."""
    out = []
    r, f = hap.HapEncode([tex], [fmt], [1], [4])
    assert r == 0
    out.append(("HapEncode", f))
    fine = hap.fine_chunk_count(len(tex), fmt)
    for name, flags, chunks in (("default", 0, 4), ("coarse", hap.ENCODE_COARSE_MATCHES, 4),
                                ("fine", hap.ENCODE_FINE_CHUNKS, fine)):
        buf = np.zeros(hap.HapMaxEncodedLength([len(tex)], [fmt], [chunks]), dtype=np.uint8)
        r, used, res = ctx.encode_frames([[tex]], [fmt], [1], [4], [buf], flags=flags)
        assert r == 0 and res == [0], name
        out.append((name, buf[: used[0]].tobytes()))
    r, f = REF.encode([tex], [fmt], [1], [3])
    assert r == 0
    out.append(("reference", f))
    return out


def want_of(frame, fmt):
    code, t, f = REF.decode(frame, 0, NB * 16)
    assert code == 0 and f == fmt
    return B.decode(t, W, H, fmt == L.FMT_BC6S)


@pytest.mark.parametrize("fmt,signed", FORMATS)
def test_hap_hdr_frames_of_every_encoder_decode_to_pictures(ctx, hap, fmt, signed):
    tex = texture(NB, 0x2024 + signed)
    frames = hap_hdr_frames(ctx, hap, tex, fmt)
    want = [want_of(f, fmt) for _, f in frames]
    assert all(np.array_equal(w, B.decode(tex, W, H, signed)) for w in want)
    n = len(frames)
    # host frames, host pictures
    hpics = [np.zeros(W * H * 8, dtype=np.uint8) for _ in range(n)]
    r, res = ctx.decode_frames_rgba_half([f for _, f in frames], [len(f) for _, f in frames], hpics, W, H)
    assert r == 0 and res == [0] * n
    for i, (name, _f) in enumerate(frames):
        assert np.array_equal(picture(hpics[i], W, H), want[i]), name
    # device frames, strided device pictures whose guard bytes stay untouched
    stride = W * 8 + 64
    dframes = [dev(f) for _, f in frames]
    pics = [torch.full((H * stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    r, res = ctx.decode_frames_rgba_half(dframes, [len(f) for _, f in frames], pics, W, H, row_bytes=stride)
    assert r == 0 and res == [0] * n
    for i, (name, _f) in enumerate(frames):
        assert np.array_equal(picture(pics[i], W, H, stride), want[i]), name
        assert guard_ok(pics[i], W, H, stride), name
    # strided host pictures are written row by row: their guard bytes stay too
    hpics = [np.full(H * stride, 0xEE, dtype=np.uint8) for _ in range(n)]
    r, res = ctx.decode_frames_rgba_half(dframes, [len(f) for _, f in frames], hpics, W, H, row_bytes=stride)
    assert r == 0 and res == [0] * n
    for i, (name, _f) in enumerate(frames):
        assert np.array_equal(picture(hpics[i], W, H, stride), want[i]) and guard_ok(hpics[i], W, H, stride), name


def test_a_batch_mixing_unsigned_and_signed_frames(ctx, hap):
    tex_a, tex_b = texture(NB, 11), texture(NB, 12)
    fu = hap_hdr_frames(ctx, hap, tex_a, L.FMT_BC6U)[1][1]
    fs = hap_hdr_frames(ctx, hap, tex_b, L.FMT_BC6S)[4][1]
    frames = [fu, fs, fs, fu]
    want = [B.decode(tex_a, W, H, False), B.decode(tex_b, W, H, True)] * 2
    want = [want[0], want[1], want[1], want[0]]
    pics = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    ctx.collect_profile()
    r, res = ctx.decode_frames_rgba_half(frames, [len(f) for f in frames], pics, W, H)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert r == 0 and res == [0] * len(frames)
    for i in range(len(frames)):
        assert np.array_equal(pics[i].cpu().numpy().view(np.uint16), want[i]), i
    # one block-decode launch per signedness, timed under the existing class
    assert prof["block_decode"][0] == 2, prof["block_decode"]
    ctx.set_profiling(True)
    ctx.collect_profile()
    assert ctx.decompress_rgba_half(tex_a, L.FMT_BC6U, W, H)[0] == 0
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 1 and prof["block_decode"][1] > 0


def _other_frames(ctx, hap):
    """A Hap (DXT1), a Hap Q and a Hap R frame of the same geometry."""
    from hap_amd import synth
    rgba = [synth.rgba_frame(W, H, 40 + i, device="cuda") for i in range(2)]
    torch.cuda.synchronize()
    out = []
    for fmt, src in ((L.FMT_DXT1, rgba[0]), (L.FMT_YCOCG, rgba[1])):
        size = NB * (8 if fmt == L.FMT_DXT1 else 16)
        buf = torch.zeros(hap.HapMaxEncodedLength([size], [fmt], [4]), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r, used, res = ctx.encode_frames_rgba([src], W, H, W * 4, [fmt], [1], [4], [buf])
        assert r == 0 and res == [0]
        out.append(buf[: used[0]].cpu().numpy().tobytes())
    r, f = hap.HapEncode([texture(NB, 77)], [L.FMT_BC7], [1], [4])
    assert r == 0
    out.append(f)
    return out


def test_other_formats_and_geometries_fail_alone(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    hap1, hapq, hapr = _other_frames(ctx, hap)
    tex = texture(NB, 31)
    good = hap_hdr_frames(ctx, hap, tex, L.FMT_BC6S)[2][1]
    small = texture(NB // 4, 32)                            # a BC6U frame of 256 x 128
    r, wrong = hap.HapEncode([small], [L.FMT_BC6U], [1], [1])
    assert r == 0
    frames = [hap1, good, hapq, wrong, hapr, good]
    pics = [np.full(W * H * 8, 0xEE, dtype=np.uint8) for _ in frames]
    for flags in (0, hap.DECODE_BPTC_PICTURES):
        r, res = ctx.decode_frames_rgba_half(frames, [len(f) for f in frames], pics, W, H, flags=flags)
        assert r == bad and res == [bad, 0, bad, bad, bad, 0], res
        want = B.decode(tex, W, H, True)
        for i in (1, 5):
            assert np.array_equal(picture(pics[i], W, H), want), i
        for i in (0, 2, 3, 4):
            assert (pics[i] == 0xEE).all(), i


def test_one_8k_frame(ctx, hap):
    w, h = 8192, 4320
    nb = (w // 4) * (h // 4)
    pool = B.block_sets()["mixed_s"]
    pool = np.frombuffer(pool, dtype=np.uint8).reshape(-1, 16)
    tex = pool[(np.arange(nb, dtype=np.int64) * 7919) % len(pool)].tobytes()
    r, f = hap.HapEncode([tex], [L.FMT_BC6S], [1], [16])
    assert r == 0
    pic = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    r, res = ctx.decode_frames_rgba_half([f], [len(f)], [pic], w, h)
    assert r == 0 and res == [0]
    got = pic.cpu().numpy().view(np.uint16)
    # every distinct block of the set decodes somewhere; check the first and last block rows and a row in the middle
    for by in (0, h // 8, h // 4 - 1):
        row = tex[by * (w // 4) * 16: (by + 1) * (w // 4) * 16]
        assert np.array_equal(got[4 * by: 4 * by + 4], B.decode(row, w, 4, True)), by

"""Hap R (BC7) to RGBA pictures on the GPU: HapGpuDecompressRGBA with RGBA_BPTC_UNORM textures and
HapGpuDecodeFramesRGBA with HAPGPU_DECODE_BPTC_PICTURES, bit-exact with the CPU reference of tests/_bptc.py (itself
pinned to Pillow by tests/test_bptc_reference.py)."""
import itertools

import numpy as np
import pytest

import _bptc as B
import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
REF = L.ref_api() or ORA


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
    """A Hap R texture that Snappy can shrink: blocks of the generated sets (every mode, reserved ones included) and
    random blocks, each repeated a few times."""
    pool = B.block_sets()["mixed"]
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
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    stride = stride or w * 4
    return a[: h * stride].reshape(h, stride)[:, : w * 4].reshape(h, w, 4)


# ------------------------------------------------------------ HapGpuDecompressRGBA --
def test_every_block_set_decodes_bit_exactly(ctx):
    for name, data in B.block_sets().items():
        w, h = B.geometry(len(data) // 16)
        r, got = ctx.decompress_rgba(data, L.FMT_BC7, w, h)
        assert r == 0, name
        assert np.array_equal(np.frombuffer(got, dtype=np.uint8).reshape(h, w, 4), B.decode(data, w, h)), name


@pytest.mark.parametrize("size", [(4, 4), (260, 36), (1024, 256)])
def test_host_and_device_textures_and_pictures(ctx, size):
    w, h = size
    nb = (w // 4) * (h // 4)
    data = texture(nb, 0x1000 + w) if nb > 1 else B.block_sets()["mode3"][:16]
    want = B.decode(data, w, h)
    # host texture, host picture
    r, got = ctx.decompress_rgba(data, L.FMT_BC7, w, h)
    assert r == 0 and np.array_equal(np.frombuffer(got, dtype=np.uint8).reshape(h, w, 4), want)
    # device texture, host picture
    dtex = dev(data)
    r, got = ctx.decompress_rgba(dtex, L.FMT_BC7, w, h)
    assert r == 0 and np.array_equal(np.frombuffer(got, dtype=np.uint8).reshape(h, w, 4), want)
    # host texture and device texture into device and host pictures, tight and with 64 guard bytes after every row:
    # only the picture's bytes of each row are written
    for tex in (data, dtex):
        for stride, where in itertools.product((w * 4, w * 4 + 64), ("cuda", "cpu")):
            out = torch.full((h * stride + 256,), 0xEE, dtype=torch.uint8, device=where)
            torch.cuda.synchronize()
            r, _ = ctx.decompress_rgba(tex, L.FMT_BC7, w, h, rgba=out, row_bytes=stride)
            assert r == 0
            a = out.cpu().numpy()
            assert np.array_equal(picture(a, w, h, stride), want)
            assert (a[: h * stride].reshape(h, stride)[:, w * 4:] == 0xEE).all()
            assert (a[(h - 1) * stride + w * 4:] == 0xEE).all()


def test_bad_arguments(ctx, hap):
    w, h = 64, 16
    data = texture((w // 4) * (h // 4), 7)
    big = dev(data + bytes(64))
    out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = hap.HapResult.Bad_Arguments
    assert ctx.decompress_rgba(big[8: 8 + len(data)], L.FMT_BC7, w, h, rgba=out)[0] == bad      # misaligned texture
    assert ctx.decompress_rgba(big[16: 16 + len(data)], L.FMT_BC7, w, h, rgba=out)[0] == 0      # (aligned: fine)
    assert ctx.decompress_rgba(data[:-16], L.FMT_BC7, w, h)[0] == bad                          # short texture
    assert ctx.decompress_rgba(data, L.FMT_BC7, w, h, alpha=bytes((w // 4) * (h // 4) * 8))[0] == bad   # no alpha plane
    assert ctx.decompress_rgba(data, L.FMT_BC6U, w, h)[0] == bad


# ------------------------------------------------------------ HapGpuDecodeFramesRGBA --
W, H = 512, 256
NB = (W // 4) * (H // 4)


def hap_r_frames(ctx, hap, tex):
    """Hap R frames of the texture from every encoder road: (name, frame bytes)."""
    out = []
    r, f = hap.HapEncode([tex], [L.FMT_BC7], [1], [4])
    assert r == 0
    out.append(("HapEncode", f))
    fine = hap.fine_chunk_count(len(tex), L.FMT_BC7)
    for name, flags, chunks in (("default", 0, 4), ("coarse", hap.ENCODE_COARSE_MATCHES, 4),
                                ("fine", hap.ENCODE_FINE_CHUNKS, fine)):
        buf = np.zeros(hap.HapMaxEncodedLength([len(tex)], [L.FMT_BC7], [chunks]), dtype=np.uint8)
        r, used, res = ctx.encode_frames([[tex]], [L.FMT_BC7], [1], [4], [buf], flags=flags)
        assert r == 0 and res == [0], name
        out.append((name, buf[: used[0]].tobytes()))
    r, f = REF.encode([tex], [L.FMT_BC7], [1], [3])
    assert r == 0
    out.append(("reference", f))
    return out


def want_of(frame, fmt, size, alpha=False):
    code, t, f = REF.decode(frame, 0, size)
    assert code == 0 and f == fmt
    if fmt == L.FMT_BC7:
        return B.decode(t, W, H)
    pic = D.oracle_bc_decode(t, fmt, W, H)
    if alpha:
        code, t1, f1 = REF.decode(frame, 1, NB * 8)
        assert code == 0 and f1 == L.FMT_RGTC1
        pic[..., 3] = D.oracle_bc_decode(t1, L.FMT_RGTC1, W, H)
    return pic


def test_hap_r_frames_of_every_encoder_decode_to_pictures(ctx, hap):
    tex = texture(NB, 0x2024)
    frames = hap_r_frames(ctx, hap, tex)
    want = [want_of(f, L.FMT_BC7, len(tex)) for _, f in frames]
    assert all(np.array_equal(w, want[0]) for w in want)
    n = len(frames)
    flag = hap.DECODE_BPTC_PICTURES
    # host frames, host pictures
    hpics = [np.zeros(W * H * 4, dtype=np.uint8) for _ in range(n)]
    r, res = ctx.decode_frames_rgba([f for _, f in frames], [len(f) for _, f in frames], 1, hpics, W, H, flags=flag)
    assert r == 0 and res == [0] * n
    for i, (name, _f) in enumerate(frames):
        assert np.array_equal(picture(hpics[i], W, H), want[i]), name
    # device frames, strided device pictures whose guard bytes stay untouched
    stride = W * 4 + 64
    dframes = [dev(f) for _, f in frames]
    pics = [torch.full((H * stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    r, res = ctx.decode_frames_rgba(dframes, [len(f) for _, f in frames], 1, pics, W, H, row_bytes=stride, flags=flag)
    assert r == 0 and res == [0] * n
    for i, (name, _f) in enumerate(frames):
        got = pics[i].cpu().numpy().reshape(H, stride)
        assert np.array_equal(got[:, : W * 4].reshape(H, W, 4), want[i]), name
        assert (got[:-1, W * 4:] == 0xEE).all(), name


def _hap_and_hap_q_frames(ctx, hap):
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
        f = buf[: used[0]].cpu().numpy().tobytes()
        out.append((f, want_of(f, fmt, size)))
    return out


def test_a_batch_mixing_hap_hap_q_and_hap_r(ctx, hap):
    (hap1, want1), (hapq, wantq) = _hap_and_hap_q_frames(ctx, hap)
    tex_a, tex_b = texture(NB, 11), texture(NB, 12)
    ra = hap_r_frames(ctx, hap, tex_a)[1][1]
    rb = hap_r_frames(ctx, hap, tex_b)[4][1]
    frames = [ra, hap1, hapq, rb, hap1]
    want = [B.decode(tex_a, W, H), want1, wantq, B.decode(tex_b, W, H), want1]
    stride = W * 4 + 32
    pics = [torch.full((H * stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    ctx.collect_profile()
    r, res = ctx.decode_frames_rgba(frames, [len(f) for f in frames], 1, pics, W, H, row_bytes=stride,
                                    flags=hap.DECODE_BPTC_PICTURES)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert r == 0 and res == [0] * len(frames)
    for i in range(len(frames)):
        got = pics[i].cpu().numpy().reshape(H, stride)
        assert np.array_equal(got[:, : W * 4].reshape(H, W, 4), want[i]), i
        assert (got[:-1, W * 4:] == 0xEE).all(), i
    # one block-decode launch per format present (DXT1, YCoCg-DXT5, BC7), timed under the existing class
    assert prof["block_decode"][0] == 3, prof["block_decode"]
    # HapGpuDecompressRGBA with BC7 is timed there too
    ctx.set_profiling(True)
    ctx.collect_profile()
    assert ctx.decompress_rgba(tex_a, L.FMT_BC7, W, H)[0] == 0
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 1 and prof["block_decode"][1] > 0


def test_without_the_flag_hap_r_frames_fail_alone(ctx, hap):
    (hap1, want1), (hapq, wantq) = _hap_and_hap_q_frames(ctx, hap)
    tex = texture(NB, 21)
    hr = hap_r_frames(ctx, hap, tex)[0][1]
    bad = hap.HapResult.Bad_Arguments
    pics = [np.zeros(W * H * 4, dtype=np.uint8) for _ in range(3)]
    r, res = ctx.decode_frames_rgba([hap1, hr, hapq], [len(hap1), len(hr), len(hapq)], 1, pics, W, H)
    assert res == [0, bad, 0] and r == bad
    assert np.array_equal(picture(pics[0], W, H), want1) and np.array_equal(picture(pics[2], W, H), wantq)
    assert not pics[1].any()
    # with the flag the same call decodes all three
    r, res = ctx.decode_frames_rgba([hap1, hr, hapq], [len(hap1), len(hr), len(hapq)], 1, pics, W, H,
                                    flags=hap.DECODE_BPTC_PICTURES)
    assert r == 0 and res == [0, 0, 0]
    assert np.array_equal(picture(pics[1], W, H), B.decode(tex, W, H))


def test_two_textures_and_bc6h_stay_bad_arguments(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    tex = texture(NB, 31)
    hr = hap_r_frames(ctx, hap, tex)[0][1]
    # textureCount 2: a Hap R frame fails alone, a Hap Q Alpha frame beside it decodes
    from hap_amd import synth
    src = synth.rgba_frame(W, H, 50, device="cuda")
    fmts = [L.FMT_YCOCG, L.FMT_RGTC1]
    sizes = [NB * 16, NB * 8]
    buf = torch.zeros(hap.HapMaxEncodedLength(sizes, fmts, [4, 4]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, used, res = ctx.encode_frames_rgba([src], W, H, W * 4, fmts, [1, 1], [4, 4], [buf])
    assert r == 0 and res == [0]
    qa = buf[: used[0]].cpu().numpy().tobytes()
    pics = [np.zeros(W * H * 4, dtype=np.uint8) for _ in range(2)]
    r, res = ctx.decode_frames_rgba([hr, qa], [len(hr), len(qa)], 2, pics, W, H, flags=hap.DECODE_BPTC_PICTURES)
    assert res == [bad, 0] and r == bad
    assert np.array_equal(picture(pics[1], W, H), want_of(qa, L.FMT_YCOCG, NB * 16, alpha=True))
    # BC6H frames have no pixel decoder, flag or not
    for fmt in (L.FMT_BC6U, L.FMT_BC6S):
        r, f = hap.HapEncode([tex], [fmt], [1], [1])
        assert r == 0
        for flags in (0, hap.DECODE_BPTC_PICTURES):
            r, res = ctx.decode_frames_rgba([f], [len(f)], 1, pics[:1], W, H, flags=flags)
            assert r == bad and res == [bad]

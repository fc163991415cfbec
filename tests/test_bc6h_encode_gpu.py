"""RGBA16F pictures to Hap HDR (BC6H) on the GPU: HapGpuCompressRGBAHalf byte-identical to the reference encoder of
tests/_bc6h_encode.py in both formats, and HapGpuEncodeFramesRGBAHalf (blocking, Begin / Finish) writing Hap HDR frames
that the unmodified reference decodes to exactly that encoder's texture and HapGpuDecodeFramesRGBAHalf to exactly
tests/_bc6h.py's picture of it."""
import numpy as np
import pytest

import _bc6h as H
import _bc6h_encode as E
import _hdr_data as HD
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
REF = L.ref_api() or ORA
FORMATS = {False: L.FMT_BC6U, True: L.FMT_BC6S}


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


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def pictures():
    rng = np.random.default_rng(0xBC6)
    out = dict(HD.hdr_images())
    y, x = np.mgrid[0:68, 0:300]
    ramp = 0x2C00 + x * 40 + y * 13
    out["ramp_300x68"] = np.stack([ramp, ramp + 900 - 3 * x, 0x3000 + ((x * y) & 1023), ramp], -1).astype(np.uint16)   # 75 blocks a row: partial waves
    out["random_bits"] = rng.integers(0, 65536, (64, 260, 4), dtype=np.uint16)
    solid = rng.integers(0, 65536, (8, 16, 1, 1, 4), dtype=np.uint16).repeat(4, 2).repeat(4, 3)
    out["solid_blocks"] = np.ascontiguousarray(solid.transpose(0, 2, 1, 3, 4).reshape(32, 64, 4))
    out["zero"] = np.zeros((16, 16, 4), np.uint16)
    return out


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", sorted(pictures()))
def test_compress_is_byte_identical_to_the_reference(ctx, hap, name, signed):
    pic = pictures()[name]
    h, w = pic.shape[:2]
    r, got = ctx.compress_rgba_half(pic, w, h, w * 8, FORMATS[signed])
    assert r == 0
    want = E.encode(pic, signed)
    if got != want:
        g, wb = np.frombuffer(got, np.uint8).reshape(-1, 16), np.frombuffer(want, np.uint8).reshape(-1, 16)
        bad = np.nonzero((g != wb).any(1))[0]
        assert False, (name, signed, len(bad), int(bad[0]), g[bad[0]].tobytes().hex(), wb[bad[0]].tobytes().hex())


@pytest.mark.parametrize("signed", [False, True])
def test_pointers_pitches_alignment_and_batches_give_the_same_bytes(ctx, hap, signed):
    fmt = FORMATS[signed]
    pic = np.ascontiguousarray(HD.hdr_images()["signed"][64:128, 128:384])
    h, w = pic.shape[:2]
    want = E.encode(pic, signed)
    nb = (w // 4) * (h // 4)
    bad = hap.HapResult.Bad_Arguments
    # float16 view and bytes of a host picture; host picture, device output
    assert ctx.compress_rgba_half(pic.view(np.float16), w, h, w * 8, fmt) == (0, want)
    assert ctx.compress_rgba_half(pic.tobytes(), w, h, w * 8, fmt) == (0, want)
    out = torch.zeros(nb * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, used = ctx.compress_rgba_half(pic, w, h, w * 8, fmt, output=out)
    assert r == 0 and used == nb * 16 and out.cpu().numpy().tobytes() == want
    # device picture, host output
    assert ctx.compress_rgba_half(dev(pic), w, h, w * 8, fmt) == (0, want)
    # padded pitches that keep the 16-byte rule, device and host
    for pad in (64, 16):
        stride = w * 8 + pad
        buf = np.full((h, stride), 0x5A, np.uint8)
        buf[:, : w * 8] = pic.view(np.uint8).reshape(h, w * 8)
        assert ctx.compress_rgba_half(dev(buf), w, h, stride, fmt) == (0, want), pad
        assert ctx.compress_rgba_half(buf, w, h, stride, fmt) == (0, want), pad
    # refused: a row pitch off the 16-byte rule or too short, a misaligned device picture or output, another format
    assert ctx.compress_rgba_half(pic, w, h, w * 8 + 8, fmt)[0] == bad
    assert ctx.compress_rgba_half(pic, w, h, w * 8 - 16, fmt)[0] == bad
    off = torch.zeros(w * h * 8 + 16, dtype=torch.uint8, device="cuda")
    off[8: 8 + w * h * 8] = dev(pic)
    torch.cuda.synchronize()
    assert ctx.compress_rgba_half(off[8:], w, h, w * 8, fmt)[0] == bad
    big = torch.zeros(nb * 16 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compress_rgba_half(pic, w, h, w * 8, fmt, output=big[8:8 + nb * 16])[0] == bad
    for other in (L.FMT_BC7, L.FMT_DXT5, L.FMT_YCOCG):
        assert ctx.compress_rgba_half(pic, w, h, w * 8, other)[0] == bad
    # one block-encode launch per call, timed under the existing class
    ctx.set_profiling(True)
    ctx.collect_profile()
    assert ctx.compress_rgba_half(pic, w, h, w * 8, fmt)[0] == 0
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_encode"][0] == 1 and prof["block_encode"][1] > 0


W, HT = 256, 128
NB = (W // 4) * (HT // 4)


def frames_of(n):
    base = HD.hdr_images()
    pics = [np.ascontiguousarray(base[("noisy", "hard_edge", "signed", "smooth")[i % 4]][16 * i: 16 * i + HT, 32 * i: 32 * i + W]) for i in range(n)]
    return pics, [dev(p) for p in pics]


def check_frames(bufs, used, results, pics, signed):
    assert results == [0] * len(pics)
    for buf, u, pic in zip(bufs, used, pics):
        frame = buf[:u].cpu().numpy().tobytes()
        want = E.encode(pic, signed)
        code, tex, fmt = REF.decode(frame, 0, NB * 16)
        assert code == 0 and fmt == FORMATS[signed] and tex == want
        yield frame, want


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("chunks", [1, 4, 7])
@pytest.mark.parametrize("flags", ["none", "coarse", "fine", "index", "coarse_index"])
def test_frames_decode_to_the_reference_texture_and_back_to_pictures(ctx, hap, chunks, flags, signed):
    f = {"none": 0, "coarse": hap.ENCODE_COARSE_MATCHES, "fine": hap.ENCODE_FINE_CHUNKS, "index": hap.ENCODE_FRAGMENT_INDEX,
         "coarse_index": hap.ENCODE_COARSE_MATCHES | hap.ENCODE_FRAGMENT_INDEX}[flags]
    fmt = FORMATS[signed]
    pics, srcs = frames_of(3)
    if chunks == 7:
        srcs = pics                                         # host pictures: staged
    cc = hap.fine_chunk_count(NB * 16, fmt) if flags == "fine" else chunks
    cap = hap.HapMaxEncodedLength([NB * 16], [fmt], [cc])
    bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in srcs]
    torch.cuda.synchronize()
    r, used, res = ctx.encode_frames_rgba_half(srcs, W, HT, W * 8, fmt, L.COMP_SNAPPY, chunks, bufs, flags=f)
    assert r == 0
    frames = list(check_frames(bufs, used, res, pics, signed))
    outs = [np.zeros(W * HT * 4, dtype=np.uint16) for _ in frames]
    r, dres = ctx.decode_frames_rgba_half([fr for fr, _ in frames], [len(fr) for fr, _ in frames], outs, W, HT)
    assert r == 0 and dres == [0] * len(frames)
    for out, (_fr, tex) in zip(outs, frames):
        assert np.array_equal(out.reshape(HT, W, 4), H.decode(tex, W, HT, signed))


def test_begin_finish_gives_the_same_frames_and_bad_frames_are_refused(ctx, hap):
    pics, srcs = frames_of(4)
    fmt = L.FMT_BC6U
    cap = hap.HapMaxEncodedLength([NB * 16], [fmt], [4])
    args = (W, HT, W * 8, fmt, L.COMP_SNAPPY, 4)
    bad = hap.HapResult.Bad_Arguments

    def bufs():
        b = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in srcs]
        torch.cuda.synchronize()
        return b

    b0 = bufs()
    r, used, res = ctx.encode_frames_rgba_half(srcs, *args, b0)
    assert r == 0
    want = [fr for fr, _ in check_frames(b0, used, res, pics, False)]
    b1 = bufs()
    assert ctx.encode_frames_rgba_half_begin(srcs, *args, b1) == 0
    r, used, res = ctx.encode_finish()
    assert r == 0 and res == [0] * len(srcs)
    assert [b1[i][: used[i]].cpu().numpy().tobytes() for i in range(len(srcs))] == want
    # a format that is not BC6H, a pitch off the 16-byte rule: the whole call; a misaligned device picture: its frame
    for a in ((W, HT, W * 8, L.FMT_BC7, L.COMP_SNAPPY, 4), (W, HT, W * 8 + 8, fmt, L.COMP_SNAPPY, 4)):
        r, _u, res = ctx.encode_frames_rgba_half(srcs, *a, bufs())
        assert r == bad and res == [bad] * len(srcs)
        assert ctx.encode_frames_rgba_half_begin(srcs, *a, bufs()) == bad
        ctx.encode_finish()
    off = torch.zeros(W * HT * 8 + 16, dtype=torch.uint8, device="cuda")
    off[8: 8 + W * HT * 8] = srcs[1]
    torch.cuda.synchronize()
    b2 = bufs()
    r, used, res = ctx.encode_frames_rgba_half([srcs[0], off[8:], srcs[2], srcs[3]], *args, b2)
    assert r == bad and res == [0, bad, 0, 0]
    assert [b2[i][: used[i]].cpu().numpy().tobytes() for i in (0, 2, 3)] == [want[0], want[2], want[3]]

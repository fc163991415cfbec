"""RGBA pictures to Hap R (BC7) on the GPU: HapGpuCompressRGBAFlags with HAPGPU_ENCODE_BPTC_BLOCKS byte-identical to the
reference encoder of tests/_bc7_encode.py, and HapGpuEncodeFramesRGBA (blocking, Begin / Finish, OnDevices) writing Hap R
frames that the unmodified reference decodes to exactly that encoder's texture."""
import numpy as np
import pytest

import _bc7_encode as E
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


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def compress(ctx, hap, img, **kw):
    h, w = img.shape[:2]
    r, got = ctx.compress_rgba(np.ascontiguousarray(img), w, h, w * 4, L.FMT_BC7, flags=hap.ENCODE_BPTC_BLOCKS, **kw)
    assert r == 0
    return got


def pictures():
    rng = np.random.default_rng(0xBC7)
    out = dict(D.quality_images())
    for name in list(out):
        o = out[name].copy()
        o[..., 3] = 255
        out[name + "_opaque"] = o
    from hap_amd import synth
    out["synth_300x68"] = synth.rgba_frame(300, 68, 3, device="cpu").numpy()        # 75 blocks a row: partial waves
    noise = rng.integers(0, 256, (64, 260, 4), dtype=np.uint8)
    for alpha in ("opaque", "binary", "random"):
        n = noise.copy()
        if alpha == "opaque":
            n[..., 3] = 255
        elif alpha == "binary":
            n[..., 3] = rng.integers(0, 2, n.shape[:2]) * 255
        out["noise_" + alpha] = n
    solid = np.empty((32, 64, 4), np.uint8)
    solid[:] = rng.integers(0, 256, (8, 16, 1, 1, 4), dtype=np.uint8).repeat(4, 2).repeat(4, 3).transpose(0, 2, 1, 3, 4).reshape(32, 64, 4)
    out["solid_blocks"] = solid
    out["transparent"] = np.zeros((16, 16, 4), np.uint8)
    return out


@pytest.mark.parametrize("name", sorted(pictures()))
def test_compress_is_byte_identical_to_the_reference(ctx, hap, name):
    img = pictures()[name]
    assert compress(ctx, hap, img) == E.encode(img), name


def test_pointers_pitches_alignment_and_batches_give_the_same_bytes(ctx, hap):
    from hap_amd import synth
    w, h = 256, 64
    img = synth.rgba_frame(w, h, 9, device="cpu").numpy()
    want = E.encode(img)
    nb = (w // 4) * (h // 4)
    flags = hap.ENCODE_BPTC_BLOCKS
    # host picture, device output
    out = torch.zeros(nb * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, used = ctx.compress_rgba(img, w, h, w * 4, L.FMT_BC7, output=out, flags=flags)
    assert r == 0 and used == nb * 16 and out.cpu().numpy().tobytes() == want
    # device picture, host output
    r, got = ctx.compress_rgba(dev(img), w, h, w * 4, L.FMT_BC7, flags=flags)
    assert r == 0 and got == want
    # padded pitch (16-byte and 4-byte aligned rows) and a source 4 bytes off 16-byte alignment
    for pad in (64, 4):
        stride = w * 4 + pad
        buf = np.full((h, stride), 0x5A, np.uint8)
        buf[:, : w * 4] = img.reshape(h, w * 4)
        r, got = ctx.compress_rgba(dev(buf), w, h, stride, L.FMT_BC7, flags=flags)
        assert r == 0 and got == want, pad
    off = torch.zeros(w * h * 4 + 16, dtype=torch.uint8, device="cuda")
    off[4: 4 + w * h * 4] = dev(img)
    torch.cuda.synchronize()
    r, got = ctx.compress_rgba(off[4:], w, h, w * 4, L.FMT_BC7, flags=flags)
    assert r == 0 and got == want
    # a misaligned device output is refused
    big = torch.zeros(nb * 16 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compress_rgba(img, w, h, w * 4, L.FMT_BC7, output=big[8:8 + nb * 16], flags=flags)[0] == hap.HapResult.Bad_Arguments
    # one block-encode launch per call, timed under the existing class
    ctx.set_profiling(True)
    ctx.collect_profile()
    assert ctx.compress_rgba(img, w, h, w * 4, L.FMT_BC7, flags=flags)[0] == 0
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_encode"][0] == 1 and prof["block_encode"][1] > 0


W, H = 512, 256
NB = (W // 4) * (H // 4)


def frames_of(hap, n, aligned=True):
    from hap_amd import synth
    pics = [synth.rgba_frame(W, H, 60 + i, device="cuda") for i in range(n)]
    if not aligned:
        pics = [torch.cat([torch.zeros(4, dtype=torch.uint8, device="cuda"), p.reshape(-1)])[4:] for p in pics]
    torch.cuda.synchronize()
    return pics


def check_frames(hap, bufs, used, results, srcs):
    assert results == [0] * len(srcs)
    for buf, u, src in zip(bufs, used, srcs):
        frame = buf[:u].cpu().numpy().tobytes()
        want = E.encode(src.reshape(H, W, 4).cpu().numpy())
        code, tex, fmt = REF.decode(frame, 0, NB * 16)
        assert code == 0 and fmt == L.FMT_BC7 and tex == want
        yield frame, want


@pytest.mark.parametrize("chunks", [1, 4, 7])
@pytest.mark.parametrize("flags", ["none", "coarse", "fine", "index", "coarse_index"])
def test_frames_decode_to_the_reference_texture_and_back_to_pictures(ctx, hap, chunks, flags):
    f = {"none": 0, "coarse": hap.ENCODE_COARSE_MATCHES, "fine": hap.ENCODE_FINE_CHUNKS, "index": hap.ENCODE_FRAGMENT_INDEX,
         "coarse_index": hap.ENCODE_COARSE_MATCHES | hap.ENCODE_FRAGMENT_INDEX}[flags]
    srcs = frames_of(hap, 3, aligned=chunks != 7)
    cc = hap.fine_chunk_count(NB * 16, L.FMT_BC7) if flags == "fine" else chunks
    cap = hap.HapMaxEncodedLength([NB * 16], [L.FMT_BC7], [cc])
    bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in srcs]
    torch.cuda.synchronize()
    r, used, res = ctx.encode_frames_rgba(srcs, W, H, W * 4, [L.FMT_BC7], [L.COMP_SNAPPY], [chunks], bufs,
                                          flags=f | hap.ENCODE_BPTC_BLOCKS)
    assert r == 0
    frames = list(check_frames(hap, bufs, used, res, srcs))
    pics = [np.zeros(W * H * 4, dtype=np.uint8) for _ in frames]
    r, dres = ctx.decode_frames_rgba([fr for fr, _ in frames], [len(fr) for fr, _ in frames], 1, pics, W, H,
                                     flags=hap.DECODE_BPTC_PICTURES)
    assert r == 0 and dres == [0] * len(frames)
    for pic, (_fr, tex) in zip(pics, frames):
        assert np.array_equal(pic.reshape(H, W, 4), B.decode(tex, W, H))


def test_begin_finish_and_on_devices_give_the_same_frames(ctx, hap):
    srcs = frames_of(hap, 4)
    cap = hap.HapMaxEncodedLength([NB * 16], [L.FMT_BC7], [4])
    args = (W, H, W * 4, [L.FMT_BC7], [L.COMP_SNAPPY], [4])
    flags = hap.ENCODE_BPTC_BLOCKS

    def bufs():
        b = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in srcs]
        torch.cuda.synchronize()
        return b

    b0 = bufs()
    r, used, res = ctx.encode_frames_rgba(srcs, *args, b0, flags=flags)
    assert r == 0
    want = [fr for fr, _ in check_frames(hap, b0, used, res, srcs)]
    b1 = bufs()
    assert ctx.encode_frames_rgba_begin(srcs, *args, b1, flags=flags) == 0
    r, used, res = ctx.encode_finish()
    assert r == 0 and res == [0] * len(srcs)
    assert [b1[i][: used[i]].cpu().numpy().tobytes() for i in range(len(srcs))] == want
    contexts = [ctx] + [hap.Context(d) for d in range(1, min(torch.cuda.device_count(), 2))]
    try:
        b2 = bufs()
        r, used, res = hap.encode_frames_rgba_on_devices(contexts, srcs, *args, b2, flags=flags)
        assert r == 0 and res == [0] * len(srcs)
        assert [b2[i][: used[i]].cpu().numpy().tobytes() for i in range(len(srcs))] == want
    finally:
        for c in contexts[1:]:
            c.close()


def test_without_the_flag_and_outside_hap_r_the_format_is_refused(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    img = pictures()["transparent"]
    h, w = img.shape[:2]
    assert ctx.compress_rgba(img, w, h, w * 4, L.FMT_BC7)[0] == bad
    for fmt in (L.FMT_BC6U, L.FMT_BC6S):
        assert ctx.compress_rgba(img, w, h, w * 4, fmt, flags=hap.ENCODE_BPTC_BLOCKS)[0] == bad
    srcs = frames_of(hap, 2)
    cap = hap.HapMaxEncodedLength([NB * 16, NB * 16], [L.FMT_BC7, L.FMT_BC7], [4, 4])
    bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in srcs]
    torch.cuda.synchronize()
    for fmts, flags in (([L.FMT_BC7], 0), ([L.FMT_BC7, L.FMT_BC7], hap.ENCODE_BPTC_BLOCKS),
                        ([L.FMT_BC7, L.FMT_RGTC1], hap.ENCODE_BPTC_BLOCKS),
                        ([L.FMT_BC6U], hap.ENCODE_BPTC_BLOCKS), ([L.FMT_BC6S], hap.ENCODE_BPTC_BLOCKS)):
        n = len(fmts)
        r, _used, res = ctx.encode_frames_rgba(srcs, W, H, W * 4, fmts, [L.COMP_SNAPPY] * n, [4] * n, bufs, flags=flags)
        assert r == bad and res == [bad, bad], (fmts, flags)
        assert ctx.encode_frames_rgba_begin(srcs, W, H, W * 4, fmts, [L.COMP_SNAPPY] * n, [4] * n, bufs, flags=flags) == bad
        ctx.encode_finish()
        r, _used, res = hap.encode_frames_rgba_on_devices([ctx], srcs, W, H, W * 4, fmts, [L.COMP_SNAPPY] * n, [4] * n, bufs,
                                                          flags=flags)
        assert r == bad and res == [bad, bad], (fmts, flags)

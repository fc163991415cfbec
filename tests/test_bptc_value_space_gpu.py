"""GPU half of the BPTC value-space sweeps (tests/_bptc_value_space.py), byte for byte against the definitions.

  encode: every picture through HapGpuCompressRGBAHalf (both formats, tight and padded pitch), HapGpuEncodeFramesRGBAHalf
          (the frame decoded by the oracle, its texture compared), HapGpuCompressRGBAFlags with BPTC blocks (tight pitch:
          16-byte loads; w * 4 + 4: 4-byte loads) and HapGpuEncodeFramesRGBA for Hap R, against tests/_bc6h_encode.py and
          tests/_bc7_encode.py.  Only here do v_rcp_f32 in rdiv, the wave ballots and partial waves run.
  decode: every decode block set through HapGpuDecompressRGBAHalf / HapGpuDecodeFramesRGBAHalf in both formats and
          HapGpuDecompressRGBA / HapGpuDecodeFramesRGBA (Hap R), one frame in HBM and one on the host, against the
          array decoders of the sweep module (pinned to tests/_bc6h.py and tests/_bptc.py by test_bptc_value_space.py)

The kernel class that ran is asserted from the context's profile.  A mismatch reports the first differing block: its
input and both outputs.  The reference results are computed once per module."""
import numpy as np
import pytest

import _bc6h_encode as E6
import _bc7_encode as E7
import _bptc_value_space as V
import _libs as L
from test_value_space_gpu import first_difference, profiled

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
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


_pics, _want = {}, {}


def pictures(kind):
    """kind: False / True (BC6H unsigned / signed) or "bc7" """
    if kind not in _pics:
        _pics[kind] = V.bc7_pictures() if kind == "bc7" else V.bc6h_pictures(kind)
    return _pics[kind]


def want(kind, name):
    if (kind, name) not in _want:
        pic = pictures(kind)[name]
        tex = E7.encode(pic) if kind == "bc7" else E6.encode(pic, kind)
        _want[(kind, name)] = np.frombuffer(tex, np.uint8).reshape(-1, 16)
    return _want[(kind, name)]


def check(got, kind, name, what):
    got = np.frombuffer(bytes(got), np.uint8).reshape(-1, 16)
    first_difference(got, want(kind, name), V.blocks_of_picture(pictures(kind)[name]), "%s %s %s" % (what, kind, name))


def padded(pic, stride):
    h = pic.shape[0]
    rows = np.ascontiguousarray(pic).view(np.uint8).reshape(h, -1)
    buf = np.full((h, stride), 0x5A, np.uint8)
    buf[:, : rows.shape[1]] = rows
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t


BC6H_NAMES = [n for n in V.BC6H_FAMILIES if n != "trigger_blocks"] + ["trigger_waves"]
BC7_NAMES = list(V.BC7_FAMILIES) + ["mode_waves"]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", BC6H_NAMES)
@pytest.mark.parametrize("pad", [0, 48])
def test_compress_rgba_half_sweeps(ctx, name, signed, pad):
    pic = pictures(signed)[name]
    h, w = pic.shape[:2]
    stride = w * 8 + pad
    src = padded(pic, stride)
    (r, got), launches = profiled(ctx, lambda: ctx.compress_rgba_half(src, w, h, stride, FORMATS[signed]))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    check(got, signed, name, "HapGpuCompressRGBAHalf pitch %d" % stride)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", BC6H_NAMES)
def test_encode_frames_rgba_half_sweeps(ctx, hap, name, signed):
    pic = pictures(signed)[name]
    h, w = pic.shape[:2]
    fmt = FORMATS[signed]
    size = (w // 4) * (h // 4) * 16
    out = torch.zeros(hap.HapMaxEncodedLength([size], [fmt], [4]), dtype=torch.uint8, device="cuda")
    src = padded(pic, w * 8)
    (r, used, res), launches = profiled(ctx, lambda: ctx.encode_frames_rgba_half([src], w, h, w * 8, fmt, L.COMP_SNAPPY, 4, [out]))
    assert r == 0 and res == [0] and launches["block_encode"] >= 1, (r, res, launches)
    code, tex, got_fmt = ORA.decode_np(out[: used[0]].cpu().numpy(), 0, size)
    assert code == 0 and got_fmt == fmt and len(tex) == size, (code, got_fmt)
    check(tex.tobytes(), signed, name, "HapGpuEncodeFramesRGBAHalf")


@pytest.mark.parametrize("name", BC7_NAMES)
@pytest.mark.parametrize("pitch", ["tight", "plus4"])
def test_compress_rgba_bc7_sweeps(ctx, hap, name, pitch):
    """bptc_encode_kernel: 16-byte row loads at a tight pitch, 4-byte loads at w * 4 + 4."""
    pic = pictures("bc7")[name]
    h, w = pic.shape[:2]
    stride = w * 4 if pitch == "tight" else w * 4 + 4
    src = padded(pic, stride)
    (r, got), launches = profiled(ctx, lambda: ctx.compress_rgba(src, w, h, stride, L.FMT_BC7, flags=hap.ENCODE_BPTC_BLOCKS))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    check(got, "bc7", name, "HapGpuCompressRGBAFlags pitch %d" % stride)


@pytest.mark.parametrize("name", BC7_NAMES)
def test_encode_frames_rgba_hap_r_sweeps(ctx, hap, name):
    pic = pictures("bc7")[name]
    h, w = pic.shape[:2]
    size = (w // 4) * (h // 4) * 16
    out = torch.zeros(hap.HapMaxEncodedLength([size], [L.FMT_BC7], [4]), dtype=torch.uint8, device="cuda")
    src = padded(pic, w * 4)
    (r, used, res), launches = profiled(ctx, lambda: ctx.encode_frames_rgba(
        [src], w, h, w * 4, [L.FMT_BC7], [L.COMP_SNAPPY], [4], [out], flags=hap.ENCODE_BPTC_BLOCKS))
    assert r == 0 and res == [0] and launches["block_encode"] >= 1, (r, res, launches)
    code, tex, got_fmt = ORA.decode_np(out[: used[0]].cpu().numpy(), 0, size)
    assert code == 0 and got_fmt == L.FMT_BC7 and len(tex) == size, (code, got_fmt)
    check(tex.tobytes(), "bc7", name, "HapGpuEncodeFramesRGBA Hap R")


# ------------------------------------------------------------------------------------------------- decode --
_decode = {}


def decode_case(kind):
    """(texture blocks [n, 16], w, h, reference picture as texels [n, 16, 4]) of all decode sets of a format, once"""
    if kind not in _decode:
        blocks, w, h = V.texture_of_sets(V.bc7_decode_sets() if kind == "bc7" else V.bc6h_decode_sets())
        want = V.decode_bc7_blocks(blocks) if kind == "bc7" else V.decode_bc6h_blocks(blocks, kind)
        _decode[kind] = (blocks, w, h, want)
    return _decode[kind]


def texels(buf, w, h, dtype):
    if hasattr(buf, "cpu"):
        buf = buf.cpu().contiguous().view(torch.uint8).numpy()
    a = np.frombuffer(bytes(buf), np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf).view(np.uint8).reshape(-1)
    return V.blocks_of_picture(a[: h * w * 4 * np.dtype(dtype).itemsize].view(dtype).reshape(h, w, 4))


def two_frames(tex, fmt):
    """one frame of the texture in HBM and one on the host"""
    r, frame = ORA.encode([tex.tobytes()], [fmt], [L.COMP_SNAPPY], [4])
    assert r == 0
    dframe = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return [dframe, frame], [len(frame)] * 2


@pytest.mark.parametrize("signed", [False, True])
def test_decompress_rgba_half_sweeps(ctx, signed):
    blocks, w, h, want = decode_case(signed)
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_rgba_half(blocks.tobytes(), FORMATS[signed], w, h))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(texels(got, w, h, np.uint16), want, blocks, "HapGpuDecompressRGBAHalf signed %s" % signed)


@pytest.mark.parametrize("signed", [False, True])
def test_decode_frames_rgba_half_sweeps(ctx, signed):
    blocks, w, h, want = decode_case(signed)
    frames, sizes = two_frames(blocks, FORMATS[signed])
    pics = [torch.zeros(h * w * 8, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    (r, res), launches = profiled(ctx, lambda: ctx.decode_frames_rgba_half(frames, sizes, pics, w, h))
    assert r == 0 and res == [0, 0] and launches["block_decode"] >= 1, (r, res, launches)
    for i, pic in enumerate(pics):
        first_difference(texels(pic, w, h, np.uint16), want, blocks, "HapGpuDecodeFramesRGBAHalf signed %s frame %d" % (signed, i))


def test_decompress_rgba_bc7_sweeps(ctx):
    blocks, w, h, want = decode_case("bc7")
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_rgba(blocks.tobytes(), L.FMT_BC7, w, h))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(texels(got, w, h, np.uint8), want, blocks, "HapGpuDecompressRGBA BC7")


def test_decode_frames_rgba_hap_r_sweeps(ctx, hap):
    blocks, w, h, want = decode_case("bc7")
    frames, sizes = two_frames(blocks, L.FMT_BC7)
    pics = [torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    (r, res), launches = profiled(ctx, lambda: ctx.decode_frames_rgba(frames, sizes, 1, pics, w, h, flags=hap.DECODE_BPTC_PICTURES))
    assert r == 0 and res == [0, 0] and launches["block_decode"] >= 1, (r, res, launches)
    for i, pic in enumerate(pics):
        first_difference(texels(pic, w, h, np.uint8), want, blocks, "HapGpuDecodeFramesRGBA Hap R frame %d" % i)

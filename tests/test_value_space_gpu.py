"""GPU half of the value-space sweeps (tests/_value_space.py): every sweep through every launch that runs the DXT1 /
DXT5 / RGTC1 / scaled YCoCg-DXT5 block code equals the oracle bit for bit.

  decode: HapGpuDecompressRGBA (DXT1, DXT5, Hap Q, Hap Q + RGTC1 alpha plane) and HapGpuDecodeFramesRGBA (the batch
          kernel) on frames carrying the sweep textures
  encode: HapGpuCompressRGBA with a tight row pitch (16-byte loads) and with w * 4 + 4 (4-byte loads), and
          HapGpuEncodeFramesRGBA with default flags (DXT5 / Hap Q through the fused compressor, DXT1 / RGTC1 through the
          batch kernel, Hap Q Alpha through the two-texture batch kernel) and with HAP_AMD_NO_FUSION (batch kernels)

The kernel class that ran is asserted from the context's profile, so a change of road cannot skip the kernel under
test.  A mismatch reports the first differing block: its input and both outputs."""
import os

import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()


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


@pytest.fixture(scope="module")
def unfused_ctx(hap):
    old = os.environ.get("HAP_AMD_NO_FUSION")
    os.environ["HAP_AMD_NO_FUSION"] = "1"
    try:
        c = hap.Context(0)
    finally:
        if old is None:
            del os.environ["HAP_AMD_NO_FUSION"]
        else:
            os.environ["HAP_AMD_NO_FUSION"] = old
    yield c
    c.close()


def profiled(ctx, call):
    """(call(), {kernel class: launches}) of the launches call() makes"""
    ctx.set_profiling(True)
    ctx.collect_profile()
    try:
        out = call()
        prof = ctx.collect_profile()
    finally:
        ctx.set_profiling(False)
    return out, {k: v[0] for k, v in prof.items()}


def first_difference(got, want, inputs, what):
    """Asserts got == want (arrays [n, ...] per block); else names the first differing block with its input."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d blocks differ; first: block %d\n  input  %s\n  kernel %s\n  oracle %s" % (
            what, len(bad), len(got), i, np.asarray(inputs[i]).tolist(), got[i].tolist(), want[i].tolist()))


# ------------------------------------------------------------------------------------------------- decode --
def _decode_case(case):
    """(texture blocks [n, b], format, alpha plane [n, 8] or None)"""
    if case == "dxt1":
        return V.pad_blocks(V.colour_blocks()), L.FMT_DXT1, None
    if case == "dxt5":
        return V.dxt5_sweep(), L.FMT_DXT5, None
    blocks, alpha = V.hapq_sweep()
    return blocks, L.FMT_YCOCG, (alpha if case == "hapq_alpha" else None)


def _oracle_picture(blocks, fmt, alpha, w, h):
    want = D.oracle_bc_decode(np.ascontiguousarray(blocks).tobytes(), fmt, w, h)
    if alpha is not None:
        want[..., 3] = D.oracle_bc_decode(alpha.tobytes(), L.FMT_RGTC1, w, h)
    return want


def _block_inputs(blocks, alpha):
    return blocks if alpha is None else np.concatenate([blocks, alpha], axis=1)


DECODE_CASES = ["dxt1", "dxt5", "hapq", "hapq_alpha"]


@pytest.mark.parametrize("case", DECODE_CASES)
def test_decompress_rgba_sweeps(ctx, case):
    blocks, fmt, alpha = _decode_case(case)
    w, h = 4 * V.BLOCK_ROW, 4 * len(blocks) // V.BLOCK_ROW
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_rgba(np.ascontiguousarray(blocks), fmt, w, h, alpha=alpha))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    got = np.frombuffer(got, dtype=np.uint8).reshape(h, w, 4)
    first_difference(V.blocks_of_picture(got), V.blocks_of_picture(_oracle_picture(blocks, fmt, alpha, w, h)),
                     _block_inputs(blocks, alpha), "HapGpuDecompressRGBA " + case)


@pytest.mark.parametrize("case", DECODE_CASES)
def test_decode_frames_rgba_sweeps(ctx, case):
    """The batch kernel on two frames of the sweep (one in HBM, one on the host), pictures in HBM."""
    blocks, fmt, alpha = _decode_case(case)
    w, h = 4 * V.BLOCK_ROW, 4 * len(blocks) // V.BLOCK_ROW
    textures = [np.ascontiguousarray(blocks).tobytes()] + ([alpha.tobytes()] if alpha is not None else [])
    fmts = [fmt] + ([L.FMT_RGTC1] if alpha is not None else [])
    T = len(fmts)
    r, frame = ORA.encode(textures, fmts, [L.COMP_SNAPPY] * T, [4] * T)
    assert r == 0
    frames = [torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda(), frame]
    pics = [torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    (r, res), launches = profiled(ctx, lambda: ctx.decode_frames_rgba(frames, [len(frame)] * 2, T, pics, w, h))
    assert r == 0 and res == [0, 0] and launches["block_decode"] >= 1, (r, res, launches)
    want = V.blocks_of_picture(_oracle_picture(blocks, fmt, alpha, w, h))
    for i, pic in enumerate(pics):
        got = V.blocks_of_picture(pic.cpu().numpy().reshape(h, w, 4))
        first_difference(got, want, _block_inputs(blocks, alpha), "HapGpuDecodeFramesRGBA %s frame %d" % (case, i))


# ------------------------------------------------------------------------------------------------- encode --
_pictures, _oracle = {}, {}


def picture(name):
    if name not in _pictures:
        _pictures[name] = V.ENCODE_PICTURES[name]()
    return _pictures[name]


def oracle_blocks(name, fmt):
    if (name, fmt) not in _oracle:
        _oracle[(name, fmt)] = D.oracle_bc_encode(picture(name), fmt)
    return _oracle[(name, fmt)]


def _check_blocks(got, name, fmt, what):
    bb = D.BLOCK_BYTES[fmt]
    want = np.frombuffer(oracle_blocks(name, fmt), dtype=np.uint8).reshape(-1, bb)
    got = np.frombuffer(bytes(got), dtype=np.uint8).reshape(-1, bb)
    first_difference(got, want, V.blocks_of_picture(picture(name)), "%s %s %#x" % (what, name, fmt))


PICTURES = list(V.ENCODE_PICTURES)
BC_FORMATS = [L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1]


@pytest.mark.parametrize("name", PICTURES)
@pytest.mark.parametrize("fmt", BC_FORMATS)
@pytest.mark.parametrize("pitch", ["tight", "plus4"])
def test_compress_rgba_sweeps(ctx, name, fmt, pitch):
    """bc_encode_kernel: 16-byte row loads at a tight pitch, 4-byte loads at w * 4 + 4."""
    img = picture(name)
    h, w = img.shape[:2]
    stride = w * 4 if pitch == "tight" else w * 4 + 4
    src = np.zeros((h, stride), dtype=np.uint8)
    src[:, : w * 4] = img.reshape(h, w * 4)
    dsrc = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    (r, got), launches = profiled(ctx, lambda: ctx.compress_rgba(dsrc, w, h, stride, fmt))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    _check_blocks(got, name, fmt, "HapGpuCompressRGBA pitch %d" % stride)


ENCODE_SETS = {"dxt1": [L.FMT_DXT1], "dxt5": [L.FMT_DXT5], "hapq": [L.FMT_YCOCG], "rgtc1": [L.FMT_RGTC1],
               "hapq_alpha": [L.FMT_YCOCG, L.FMT_RGTC1]}
ROADS = [(s, "default") for s in ENCODE_SETS] + [(s, "no_fusion") for s in ("dxt5", "hapq", "hapq_alpha")]


@pytest.mark.parametrize("name", PICTURES)
@pytest.mark.parametrize("formats,road", ROADS)
def test_encode_frames_rgba_sweeps(ctx, unfused_ctx, hap, name, formats, road):
    """HapGpuEncodeFramesRGBA: a frame whose every texture the oracle decodes to exactly oracle_bc_encode of the
    picture.  By default DXT5 and Hap Q run the fused compressor (encode_fused, no block_encode launch); DXT1, RGTC1,
    Hap Q Alpha (two textures) and everything with HAP_AMD_NO_FUSION run the batch kernels (block_encode)."""
    c = ctx if road == "default" else unfused_ctx
    fmts = ENCODE_SETS[formats]
    T = len(fmts)
    img = picture(name)
    h, w = img.shape[:2]
    sizes = [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]
    cap = hap.HapMaxEncodedLength(sizes, fmts, [4] * T)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    (r, used, results), launches = profiled(c, lambda: c.encode_frames_rgba([src], w, h, w * 4, fmts, [1] * T, [4] * T, [out]))
    assert r == 0 and results == [0], (r, results)
    fused = road == "default" and formats in ("dxt5", "hapq")
    if fused:
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    else:
        assert launches["block_encode"] >= 1 and launches["encode_fused"] == 0, launches
    frame = out[: used[0]].cpu().numpy()
    for t, f in enumerate(fmts):
        code, tex, got_fmt = ORA.decode_np(frame, t, sizes[t])
        assert code == 0 and got_fmt == f and len(tex) == sizes[t], (code, got_fmt)
        _check_blocks(tex.tobytes(), name, f, "HapGpuEncodeFramesRGBA (%s, texture %d)" % (road, t))

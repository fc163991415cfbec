"""A8 pictures <-> RGTC1 textures and Hap Alpha-Only frames on the GPU (alpha_plane.hip and the ...Alpha calls).

The truth is the oracle: D.oracle_bc_encode(rgba, L.FMT_RGTC1) of an RGBA picture that carries the plane in its alpha
channel, and D.oracle_bc_decode(blocks, L.FMT_RGTC1, w, h).  Everything is compared byte for byte; a mismatch names
the first differing block with its input.  Shapes and pitches cover both roads of each kernel: the four-blocks-per-lane
road (picture and pitch 16-byte aligned) with its tail of one to three blocks, and the one-block-per-lane road."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
REF = L.ref_api() or ORA
RGTC1 = L.FMT_RGTC1
FILL = 0x5A


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


def filled(n, where):
    if where == "host":
        return np.full(n, FILL, dtype=np.uint8)
    t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host_bytes(buf):
    return buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)


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


def rgba_carrying(plane):
    """An RGBA8 picture with `plane` in its alpha channel (the colours are there to be ignored)."""
    h, w = plane.shape
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., 0] = 255 - plane
    img[..., 1] = 0x33
    img[..., 2] = plane // 2
    img[..., 3] = plane
    return img


def blocks_of_plane(plane):
    h, w = plane.shape
    return plane.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)


def as_blocks(texture):
    return np.frombuffer(bytes(texture), dtype=np.uint8).reshape(-1, 8)


SHAPES = [(4, 4), (20, 8), (300, 68), (1024, 16)]      # one block; a four-block lane + 1; 75 a row: partial wave, tail of 3
# w: the wide road where w % 16 == 0; w + 4: the narrow road (the wide one for 300); w + 16: padded rows; and the next
# multiple of 16 above w + 16, which puts every shape on the wide road: 20 x 8 its four-block lane plus one, 300 x 68 its
# tail of three, 4 x 4 a tail alone
PITCHES = {"tight": lambda w: w, "plus4": lambda w: w + 4, "plus16": lambda w: w + 16, "wide": lambda w: w + (-w) % 16 + 16}

_cases = {}


def case(w, h):
    """(plane, the oracle's texture of it, random blocks, the oracle's plane of those) for a shape, computed once"""
    if (w, h) not in _cases:
        rng = np.random.default_rng(0xA8 + w * 4099 + h)
        y, x = np.mgrid[0:h, 0:w]
        smooth = ((x * 3 + y * 5) % 256).astype(np.uint8)
        noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
        plane = np.where(((x // 4 + y // 4) % 3) == 0, noise, np.where(((x // 4 + y // 4) % 3) == 1, smooth, smooth // 16 * 16))
        plane = np.ascontiguousarray(plane.astype(np.uint8))
        texture = D.oracle_bc_encode(rgba_carrying(plane), RGTC1)
        blocks = rng.integers(0, 256, ((w // 4) * (h // 4), 8), dtype=np.uint8)
        blocks[::5, 0] = np.minimum(blocks[::5, 0], blocks[::5, 1])          # both palette modes, and equal endpoints
        blocks[::7, 1] = blocks[::7, 0]
        decoded = D.oracle_bc_decode(blocks.tobytes(), RGTC1, w, h)
        for a in (plane, blocks, decoded):
            a.setflags(write=False)
        _cases[(w, h)] = (plane, texture, blocks, decoded)
    return _cases[(w, h)]


def padded(plane, pitch):
    h, w = plane.shape
    buf = np.full((h, pitch), FILL, dtype=np.uint8)
    buf[:, :w] = plane
    return buf


# ------------------------------------------------------------------------------------------------- textures --
def test_compress_alpha_value_sweep(ctx):
    """Every pair lo < hi with every value between (V.ramp_picture): the oracle's blocks, byte for byte."""
    img = V.ramp_picture()
    plane = np.ascontiguousarray(img[..., 3])
    h, w = plane.shape
    (r, got), launches = profiled(ctx, lambda: ctx.compress_alpha(plane, w, h, w))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    first_difference(as_blocks(got), as_blocks(D.oracle_bc_encode(img, RGTC1)), blocks_of_plane(plane), "HapGpuCompressAlpha ramps")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pitch", list(PITCHES))
@pytest.mark.parametrize("w,h", SHAPES)
def test_compress_alpha_shapes_and_roads(ctx, w, h, pitch, where):
    plane, texture, _blocks, _decoded = case(w, h)
    stride = PITCHES[pitch](w)
    src = padded(plane, stride)
    if where == "device":
        src = dev(src)
    (r, got), launches = profiled(ctx, lambda: ctx.compress_alpha(src, w, h, stride))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    first_difference(as_blocks(got), as_blocks(texture), blocks_of_plane(plane), "HapGpuCompressAlpha %dx%d pitch %d %s" % (w, h, stride, where))


def test_decompress_alpha_value_sweep(ctx):
    """All 65 536 endpoint pairs with every code (V.ramp_blocks) as a 1024 x 1024 plane: obc_decode_rgtc1 for every block."""
    blocks = np.ascontiguousarray(V.ramp_blocks())
    w = h = 1024
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_alpha(blocks, w, h))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    got = np.frombuffer(got, dtype=np.uint8).reshape(h, w)
    want = D.oracle_bc_decode(blocks.tobytes(), RGTC1, w, h)
    first_difference(blocks_of_plane(got), blocks_of_plane(want), blocks, "HapGpuDecompressAlpha ramps")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pitch", list(PITCHES))
@pytest.mark.parametrize("w,h", SHAPES)
def test_decompress_alpha_shapes_and_roads(ctx, w, h, pitch, where):
    _plane, _texture, blocks, decoded = case(w, h)
    stride = PITCHES[pitch](w)
    out = filled(h * stride, where)
    tex = dev(blocks) if where == "device" else blocks
    (r, _none), launches = profiled(ctx, lambda: ctx.decompress_alpha(tex, w, h, out=out, row_bytes=stride))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    got = host_bytes(out).reshape(h, stride)
    first_difference(blocks_of_plane(np.ascontiguousarray(got[:, :w])), blocks_of_plane(decoded), blocks,
                     "HapGpuDecompressAlpha %dx%d pitch %d %s" % (w, h, stride, where))
    assert (got[:, w:] == FILL).all(), "bytes between width and rowBytes were written"


# --------------------------------------------------------------------------------------------------- frames --
W, HT = 256, 128
NB = (W // 4) * (HT // 4)


def frame_pictures():
    q = D.quality_images()
    imgs = [np.ascontiguousarray(q["noisy"][0:HT, 0:W]), np.ascontiguousarray(q["smooth"][64:64 + HT, 128:128 + W]),
            np.ascontiguousarray(q["hard_edge"][32:32 + HT, 200:200 + W])]
    return imgs, [np.ascontiguousarray(i[..., 3]) for i in imgs]


def mixed(arrays):
    """host and device mixed: the middle one stays on the host"""
    return [a if i == 1 else dev(a) for i, a in enumerate(arrays)]


def outputs(n, cap):
    b = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("form", ["blocking", "begin_finish"])
@pytest.mark.parametrize("flags", ["none", "index", "fine"])
def test_frames_out(ctx, hap, form, flags):
    f = {"none": 0, "index": hap.ENCODE_FRAGMENT_INDEX, "fine": hap.ENCODE_FINE_CHUNKS}[flags]
    imgs, planes = frame_pictures()
    chunks = 4
    cc = hap.fine_chunk_count(NB * 8, RGTC1) if flags == "fine" else chunks
    cap = hap.HapMaxEncodedLength([NB * 8], [RGTC1], [cc])
    bufs = outputs(3, cap)
    srcs = mixed(planes)
    if form == "blocking":
        r, used, res = ctx.encode_frames_alpha(srcs, W, HT, W, L.COMP_SNAPPY, chunks, bufs, flags=f)
    else:
        assert ctx.encode_frames_alpha_begin(srcs, W, HT, W, L.COMP_SNAPPY, chunks, bufs, flags=f) == 0
        r, used, res = ctx.encode_finish()
    assert r == 0 and res == [0, 0, 0], (r, res)
    rbufs = outputs(3, cap)
    rr, rused, rres = ctx.encode_frames_rgba(mixed(imgs), W, HT, W * 4, [RGTC1], [L.COMP_SNAPPY], [chunks], rbufs, flags=f)
    assert rr == 0 and rres == [0, 0, 0]
    for i, img in enumerate(imgs):
        frame = bufs[i][: used[i]].cpu().numpy().tobytes()
        want = D.oracle_bc_encode(img, RGTC1)
        assert REF.decode(frame, 0, NB * 8) == (0, want, RGTC1), i
        assert REF.texture_count(frame) == (0, 1)
        assert frame == rbufs[i][: rused[i]].cpu().numpy().tobytes(), "frame %d differs from HapGpuEncodeFramesRGBA's" % i


def test_frames_in(ctx, hap):
    imgs, planes = frame_pictures()
    textures = [D.oracle_bc_encode(i, RGTC1) for i in imgs]
    foreign = []
    for t in textures[:2]:
        r, fr = ORA.encode([t], [RGTC1], [L.COMP_SNAPPY], [3])
        assert r == 0
        foreign.append(fr)
    cap = hap.HapMaxEncodedLength([NB * 8], [RGTC1], [4])
    buf = outputs(1, cap)
    r, used, res = ctx.encode_frames_alpha([planes[2]], W, HT, W, L.COMP_SNAPPY, 4, buf)
    assert r == 0 and res == [0]
    ours = buf[0][: used[0]].cpu().numpy().tobytes()
    r, hapq = ORA.encode([D.oracle_bc_encode(imgs[0], L.FMT_YCOCG)], [L.FMT_YCOCG], [L.COMP_SNAPPY], [2])
    assert r == 0
    frames = [foreign[0], foreign[1], ours, ours[:-10], hapq]
    sizes = [len(fr) for fr in frames]
    inputs = [dev(np.frombuffer(fr, dtype=np.uint8)) if i % 2 == 0 else fr for i, fr in enumerate(frames)]
    wheres = ["host", "device", "device", "host", "device"]
    bad_frame, bad_args = hap.HapResult.Bad_Frame, hap.HapResult.Bad_Arguments

    assert REF.decode(ours[:-10], 0, NB * 8)[0] == bad_frame         # HapDecode's code for the broken frame
    pics = [filled(W * HT, wh) for wh in wheres]
    (r, res), launches = profiled(ctx, lambda: ctx.decode_frames_alpha(inputs, sizes, pics, W, HT))
    assert res == [0, 0, 0, bad_frame, bad_args] and r == bad_frame, (r, res)
    assert launches["block_decode"] >= 1, launches
    for i in range(3):
        want = D.oracle_bc_decode(textures[i], RGTC1, W, HT)
        first_difference(blocks_of_plane(host_bytes(pics[i]).reshape(HT, W)), blocks_of_plane(want), as_blocks(textures[i]),
                         "HapGpuDecodeFramesAlpha frame %d" % i)
    for i in (3, 4):
        assert (host_bytes(pics[i]) == FILL).all(), "the picture of failed frame %d was written" % i

    pics = [filled((W + 4) * HT, wh) for wh in wheres]
    r, res = ctx.decode_frames_alpha(inputs, sizes, pics, W + 4, HT, row_bytes=W)
    assert r == bad_args and res == [bad_args] * 5, (r, res)
    r, res = ctx.decode_frames_alpha(inputs[:3], sizes[:3], pics[:3], W + 4, HT, row_bytes=W + 4)      # another geometry
    assert r == bad_args and res == [bad_args] * 3, (r, res)
    for p in pics:
        assert (host_bytes(p) == FILL).all()


# ------------------------------------------------------------------------------------------------ refusals --
def test_refusals(ctx, hap):
    bad, small = hap.HapResult.Bad_Arguments, hap.HapResult.Buffer_Too_Small
    w, h = 32, 16
    nb = (w // 4) * (h // 4)
    plane, texture, _blocks, _decoded = case(1024, 16)
    plane = np.ascontiguousarray(plane[:h, :w + 8])                       # rows of w + 8 bytes: any pitch up to that fits
    texture = D.oracle_bc_encode(rgba_carrying(np.ascontiguousarray(plane[:, :w])), RGTC1)
    r, frame = ORA.encode([texture], [RGTC1], [L.COMP_SNAPPY], [1])
    assert r == 0
    cap = hap.HapMaxEncodedLength([nb * 8], [RGTC1], [1])

    def every_call(width, height, row_bytes, src=plane, out_picture=None):
        """the result of each of the five calls, and the per-frame results of the batched ones"""
        pic = out_picture if out_picture is not None else filled((w + 8) * (h + 4), "host")
        got = {"compress": (ctx.compress_alpha(src, width, height, row_bytes)[0], None),
               "decompress": (ctx.decompress_alpha(texture, width, height, out=pic, row_bytes=row_bytes)[0], None)}
        r, _used, res = ctx.encode_frames_alpha([src], width, height, row_bytes, L.COMP_SNAPPY, 1, outputs(1, cap))
        got["encode_frames"] = (r, res)
        rb = ctx.encode_frames_alpha_begin([src], width, height, row_bytes, L.COMP_SNAPPY, 1, outputs(1, cap))
        rf, _used, res = ctx.encode_finish()
        got["encode_frames_begin"] = (rb or rf, res)
        got["decode_frames"] = ctx.decode_frames_alpha([frame], [len(frame)], [pic], width, height, row_bytes=row_bytes)
        assert (host_bytes(pic) == FILL).all()
        return got

    rules = {"rowBytes below width": (w, h, w - 4), "rowBytes not a multiple of 4": (w, h, w + 2),
             "width not a multiple of 4": (w + 2, h, w + 8), "height not a multiple of 4": (w, h + 2, w + 8)}
    for what, (width, height, row_bytes) in rules.items():
        for call, (r, res) in every_call(width, height, row_bytes).items():
            assert r == bad and res in (None, [bad]), (what, call, r, res)

    # a device picture at an address that is 2 modulo 4, read and written
    off = torch.full(((w + 8) * h + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for call, (r, res) in every_call(w, h, w + 8, src=off[2:], out_picture=off[2:]).items():
        assert r == bad and res in (None, [bad]), ("device picture 2 mod 4", call, r, res)

    # a device texture at an address that is 4 modulo 8, written and read
    dtex = torch.zeros(nb * 8 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compress_alpha(plane, w, h, w + 8, output=dtex[4: 4 + nb * 8])[0] == bad
    assert ctx.decompress_alpha(dtex[4: 4 + nb * 8], w, h)[0] == bad
    assert ctx.compress_alpha(plane, w, h, w + 8, output=dtex[8: 8 + nb * 8]) == (0, nb * 8)
    assert dtex[8: 8 + nb * 8].cpu().numpy().tobytes() == texture

    # an output one byte short, as in HapGpuCompressRGBA
    short = np.zeros(nb * 8 - 1, dtype=np.uint8)
    assert ctx.compress_alpha(plane, w, h, w + 8, output=short)[0] == small
    assert ctx.compress_rgba(rgba_carrying(np.ascontiguousarray(plane[:, :w])), w, h, w * 4, RGTC1, output=short)[0] == small
    # and a texture one byte short
    assert ctx.decompress_alpha(texture[:-1], w, h)[0] == bad

    # the RGBA calls still refuse a lone RGTC1 texture
    assert ctx.decompress_rgba(texture, RGTC1, w, h)[0] == bad
    pic = filled(w * h * 4, "device")
    assert ctx.decode_frames_rgba([frame], [len(frame)], 1, [pic], w, h) == (bad, [bad])
    assert (host_bytes(pic) == FILL).all()


def test_every_call_accepts_what_the_refusals_vary(ctx, hap):
    """The arguments test_refusals starts from are good ones: each call succeeds with them."""
    w, h = 32, 16
    nb = (w // 4) * (h // 4)
    plane, _t, _b, _d = case(1024, 16)
    plane = np.ascontiguousarray(plane[:h, :w + 8])
    texture = D.oracle_bc_encode(rgba_carrying(np.ascontiguousarray(plane[:, :w])), RGTC1)
    want = padded(D.oracle_bc_decode(texture, RGTC1, w, h), w + 8)
    r, frame = ORA.encode([texture], [RGTC1], [L.COMP_SNAPPY], [1])
    assert r == 0
    cap = hap.HapMaxEncodedLength([nb * 8], [RGTC1], [1])
    assert ctx.compress_alpha(plane, w, h, w + 8) == (0, texture)
    pic = filled((w + 8) * h, "host")
    assert ctx.decompress_alpha(texture, w, h, out=pic, row_bytes=w + 8)[0] == 0 and (pic.reshape(h, w + 8) == want).all()
    buf = outputs(1, cap)
    r, used, res = ctx.encode_frames_alpha([plane], w, h, w + 8, L.COMP_SNAPPY, 1, buf)
    assert r == 0 and res == [0] and REF.decode(buf[0][: used[0]].cpu().numpy().tobytes(), 0, nb * 8) == (0, texture, RGTC1)
    pic = filled((w + 8) * h, "device")
    assert ctx.decode_frames_alpha([frame], [len(frame)], [pic], w, h, row_bytes=w + 8) == (0, [0])
    assert (host_bytes(pic).reshape(h, w + 8) == want).all()


# ---------------------------------------------------------------------------------------------- round trip --
@pytest.mark.parametrize("name", sorted(D.quality_images()))
def test_round_trip_quality_equals_the_existing_road(ctx, name):
    """A sanity check, not a definition: the two roads make the same blocks, so the PSNR is the same number."""
    img = D.quality_images()[name]
    h, w = img.shape[:2]
    plane = np.ascontiguousarray(img[..., 3])
    r, tex = ctx.compress_alpha(plane, w, h, w)
    assert r == 0
    r, existing = ctx.compress_rgba(img, w, h, w * 4, RGTC1)
    assert r == 0 and tex == existing
    r, back = ctx.decompress_alpha(tex, w, h)
    assert r == 0
    got = D.psnr(np.frombuffer(back, dtype=np.uint8).reshape(h, w), plane)
    assert got == D.block_quality(existing, RGTC1, img)[0]

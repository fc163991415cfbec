"""Hap frames and block textures straight to NV12 video pictures (HapGpuDecompressNV12, HapGpuDecodeFramesNV12): the
planes are tests/_video_planes.py's definition applied to the CPU oracle's decode of the same textures
(tests/_data.oracle_bc_decode), box-filtered for s = 1, 2 as test_scaled_decode_gpu.box defines it -- and to what
decode_frames_rgba[_scaled] writes in the same run.  Every comparison is byte for byte.

Every shape gives 67 destination blocks a row (one full wavefront and a partial one) and two block rows: source 268 x 8
at s = 0, 536 x 16 at s = 1, 1072 x 32 at s = 2.  The luma pitch is larger than W, the chroma pitch another one, and
everything between the rows and behind the planes keeps its sentinel."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _video_planes as P
from test_scaled_decode_gpu import FORMATS, box, random_texture
from test_value_space_derived_gpu import BLOCK_SOURCES, ids, per_block, source

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
SENTINEL = 0xA7
SHAPES = {0: (268, 8), 1: (536, 16), 2: (1072, 32)}           # source sizes: 67 x 2 destination blocks each
CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")             # Hap, Hap Alpha, Hap Q, Hap Q Alpha


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


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


class Targets:
    """n NV12 pictures of w x h in sentinel-filled device memory: luma rows w + 12 apart, chroma rows w + 20 apart, 64
    bytes behind each set of planes"""

    def __init__(self, n, w, h):
        self.n, self.w, self.h, self.lp, self.cp = n, w, h, w + 12, w + 20
        self.ybuf = torch.full((n * h * self.lp + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.cbuf = torch.full((n * (h // 2) * self.cp + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.luma = [self.ybuf[: n * h * self.lp].view(n, h, self.lp)[f, :, :w] for f in range(n)]
        self.chroma = [self.cbuf[: n * (h // 2) * self.cp].view(n, h // 2, self.cp)[f, :, :w] for f in range(n)]

    def read(self):
        """([y (h, w)], [uv (h / 2, w)], all the bytes that are no sample)"""
        n, w, h = self.n, self.w, self.h
        ya, ca = self.ybuf.cpu().numpy(), self.cbuf.cpu().numpy()
        yb, cb = ya[:-64].reshape(n, h, self.lp), ca[:-64].reshape(n, h // 2, self.cp)
        rest = np.concatenate([yb[:, :, w:].ravel(), cb[:, :, w:].ravel(), ya[-64:], ca[-64:]])
        return [yb[f, :, :w] for f in range(n)], [cb[f, :, :w] for f in range(n)], rest

    def check(self, wanted, what):
        """wanted[f]: the RGBA8 picture whose planes frame f holds under `row`, or None: untouched"""
        ys, uvs, rest = self.read()
        assert (rest == SENTINEL).all(), (what, "bytes that are no sample were written")
        for f, want in enumerate(wanted):
            if want is None:
                assert (ys[f] == SENTINEL).all() and (uvs[f] == SENTINEL).all(), (what, f, "a refused frame's planes were written")
                continue
            wy, wuv = want
            assert np.array_equal(ys[f], wy), (what, f, "luma", np.argwhere(ys[f] != wy)[:4].tolist())
            assert np.array_equal(uvs[f], wuv), (what, f, "chroma", np.argwhere(uvs[f] != wuv)[:4].tolist())


def level(full, s):
    return full if s == 0 else box(full, s)


def textures_of(case, s):
    """(textures [colour(, plane)], formats, the oracle's picture at scale s)"""
    w, h = SHAPES[s]
    tex, plane, full = random_texture(case, w, h)
    textures = [tex] + ([plane] if plane is not None else [])
    return textures, [FORMATS[case]] + ([L.FMT_RGTC1] if plane is not None else []), level(full, s)


def plain_frame(textures, fmts):
    r, frame = ORA.encode(textures, fmts, [L.COMP_SNAPPY] * len(fmts), [2] * len(fmts))
    assert r == 0
    return frame


def table_frame(ctx, hap, textures, fmts):
    """the same textures as a frame with the fragment table"""
    n = len(fmts)
    buf = np.zeros(hap.HapMaxEncodedLength([len(t) for t in textures], fmts, [2] * n) + 4096, dtype=np.uint8)
    r, used, res = ctx.encode_frames([[np.frombuffer(t, np.uint8) for t in textures]], fmts, [L.COMP_SNAPPY] * n, [2] * n,
                                     [buf], flags=hap.ENCODE_FRAGMENT_INDEX)
    assert r == 0 and res == [0]
    return buf[: used[0]].tobytes()


def rgba_of_frames(ctx, frames, count, w, h, s):
    """what decode_frames_rgba[_scaled] writes for the frames, in this run: [(h >> s, w >> s, 4)]"""
    ow, oh = w >> s, h >> s
    pics = [torch.zeros(oh * ow * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    lens = [len(f) if isinstance(f, bytes) else f.numel() for f in frames]
    if s == 0:
        r, res = ctx.decode_frames_rgba(frames, lens, count, pics, w, h)
    else:
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, count, pics, w, h, s)
    assert r == 0 and res == [0] * len(frames)
    return [p.cpu().numpy().reshape(oh, ow, 4) for p in pics]


# ------------------------------------------------------------------------------------------------ the definition --
@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("case", CASES)
def test_frames_of_every_flavour_under_every_row(ctx, hap, case, s):
    """A plain frame in device memory and one with the fragment table in host memory, all four (matrix, range) rows."""
    w, h = SHAPES[s]
    textures, fmts, want = textures_of(case, s)
    plain, table = plain_frame(textures, fmts), table_frame(ctx, hap, textures, fmts)
    frames, lens = [dev(plain), table], [len(plain), len(table)]
    decoded = rgba_of_frames(ctx, frames, len(fmts), w, h, s)
    for d in decoded:
        assert np.array_equal(d[..., :3], want[..., :3])
    for row in P.ROWS:
        t = Targets(2, w >> s, h >> s)
        r, res = ctx.decode_frames_nv12(frames, lens, len(fmts), t.luma, t.chroma, w, h, scale_log2=s, matrix=row[0],
                                        range=row[1])
        assert r == 0 and res == [0, 0], (case, s, row, r, res)
        t.check([P.planes_of_rgba(want, *row)] * 2, (case, s, P.NAMES[row], "oracle"))
        t.check([P.planes_of_rgba(d, *row) for d in decoded], (case, s, P.NAMES[row], "decode_frames_rgba"))


@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("case", CASES[:3])
def test_the_single_texture_call(ctx, case, s):
    w, h = SHAPES[s]
    textures, _fmts, want = textures_of(case, s)
    for turn, tex in enumerate((textures[0], dev(textures[0]))):
        row = P.ROWS[(turn + s) % 4]
        t = Targets(1, w >> s, h >> s)
        r = ctx.decompress_nv12(tex, FORMATS[case], w, h, t.luma[0], t.chroma[0], scale_log2=s, matrix=row[0], range=row[1])
        assert r == 0, (case, s, turn)
        t.check([P.planes_of_rgba(want, *row)], (case, s, turn))


@pytest.mark.parametrize("s", (0, 1, 2))
def test_a_mixed_batch(ctx, hap, s):
    """Hap, Hap Alpha and Hap Q frames in one call (one launch per format present); a Hap Q Alpha frame read with
    textureCount 1 is its colour texture's."""
    w, h = SHAPES[s]
    frames, wanted = [], []
    row = (P.BT601, P.FULL)
    for i, case in enumerate(("ycocg", "dxt1", "dxt5", "ycocg_alpha", "dxt1")):
        textures, fmts, want = textures_of(case, s)
        frame = plain_frame(textures, fmts) if i % 2 else table_frame(ctx, hap, textures, fmts)
        frames.append(dev(frame) if i % 3 == 0 else frame)
        wanted.append(P.planes_of_rgba(want, *row))
    t = Targets(len(frames), w >> s, h >> s)
    lens = [len(f) if isinstance(f, bytes) else f.numel() for f in frames]
    r, res = ctx.decode_frames_nv12(frames, lens, 1, t.luma, t.chroma, w, h, scale_log2=s, matrix=row[0], range=row[1])
    assert r == 0 and res == [0] * len(frames), (r, res)
    t.check(wanted, ("mixed", s))


# ------------------------------------------------------------------------------------------------ the value space --
@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("src", BLOCK_SOURCES[:6], ids=ids(BLOCK_SOURCES[:6]))
def test_the_value_space_sweeps(ctx, src, s):
    """tests/_value_space.py's texture sets (random codes and the edge sets) through the new kernel, which instantiates
    the decode bodies anew.  A mismatch reports the first differing block: its input bytes and both outputs."""
    c = source(*src)
    row = P.ROWS[(BLOCK_SOURCES.index(src) + s) % 4]
    tex, _plane = c.textures(BLOCK_SOURCES.index(src) + s)
    ow, oh = c.w >> s, c.h >> s
    y = torch.zeros((oh, ow), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((oh // 2, ow), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = ctx.decompress_nv12(tex, c.fmt, c.w, c.h, y, uv, scale_log2=s, matrix=row[0], range=row[1])
    assert r == 0
    wy, wuv = P.planes_of_rgba(c.level(s), *row)
    # per destination block: its 4 x 4 Y samples and its 2 x 4 bytes of pairs
    got = np.concatenate([per_block(y.cpu().numpy()[..., None], 0)[..., 0], blocks_of_pairs(uv.cpu().numpy())], axis=1)
    want = np.concatenate([per_block(wy[..., None], 0)[..., 0], blocks_of_pairs(wuv)], axis=1)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    if wrong.size:
        i = int(wrong[0])
        k = 1 << s
        bx, by = i % (ow // 4), i // (ow // 4)
        under = c.inputs.reshape(c.h // 4, c.w // 4, -1)[by * k: by * k + k, bx * k: bx * k + k]
        pytest.fail("HapGpuDecompressNV12 %s %s s = %d %s: %d blocks differ, first %d: inputs %s got %s want %s"
                    % (src + (s, P.NAMES[row], wrong.size, i, under.tolist(), got[i].tolist(), want[i].tolist())))


def blocks_of_pairs(uv):
    """(h / 2, w) -> [destination blocks, 8]: two rows of two pairs each"""
    h2, w = uv.shape
    return uv.reshape(h2 // 2, 2, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 8)


# --------------------------------------------------------------------------------------------- failures of a frame --
def test_a_frame_fails_alone(ctx, hap):
    s = 1
    w, h = SHAPES[s]
    ow, oh = w >> s, h >> s
    row = (P.BT709, P.LIMITED)
    textures, fmts, want = textures_of("ycocg", s)
    good = plain_frame(textures, fmts)
    planes = P.planes_of_rgba(want, *row)
    rng = np.random.default_rng(7)
    bc7 = plain_frame([rng.integers(0, 256, (w // 4) * (h // 4) * 16, dtype=np.uint8).tobytes()], [L.FMT_BC7])
    small = plain_frame([random_texture("ycocg", *SHAPES[0])[0]], [L.FMT_YCOCG])
    frames = [good, bc7, good[: len(good) // 2], small, good, good, good, good, good]
    t = Targets(len(frames), ow, oh)
    luma, chroma = list(t.luma), list(t.chroma)
    luma[4] = None                                                     # no Y plane
    chroma[5] = None                                                   # no CbCr plane
    host_plane = torch.full((oh // 2, ow), SENTINEL, dtype=torch.uint8)
    ya = [None if p is None else p.data_ptr() for p in luma]
    ca = [None if p is None else p.data_ptr() for p in chroma]
    ca[6] = host_plane.data_ptr()                                      # a CbCr plane in host memory
    ya[7] += 2                                                         # a misaligned Y plane
    r, res = ctx.decode_frames_nv12(frames, [len(f) for f in frames], 1, ya, ca, w, h, scale_log2=s, matrix=row[0],
                                    range=row[1], luma_row_bytes=t.lp, chroma_row_bytes=t.cp)
    bad = hap.HapResult.Bad_Arguments
    assert res[0] == 0 and res[8] == 0, res
    assert res[1] == bad and res[3] == bad and res[4:8] == [bad] * 4, res
    assert res[2] != 0, res                                            # HapDecode's code for the broken frame
    assert r == res[1]                                                 # the first failure
    t.check([planes, None, None, None, None, None, None, None, planes], "alone")
    assert (host_plane.numpy() == SENTINEL).all()
    # HAPGPU_DECODE_BPTC_PICTURES is ignored: the Hap R frame is still another format
    t = Targets(2, ow, oh)
    r, res = ctx.decode_frames_nv12([bc7, good], [len(bc7), len(good)], 1, t.luma, t.chroma, w, h, scale_log2=s,
                                    matrix=row[0], range=row[1], flags=hap.DECODE_BPTC_PICTURES)
    assert r == bad and res == [bad, 0], (r, res)
    t.check([None, planes], "flag ignored")


# ---------------------------------------------------------------------------------- failures of the whole call --
def test_whole_call_refusals(ctx, hap):
    s = 1
    w, h = SHAPES[s]
    ow, oh = w >> s, h >> s
    textures, fmts, _want = textures_of("dxt1", s)
    frame = plain_frame(textures, fmts)
    bad, internal = hap.HapResult.Bad_Arguments, hap.HapResult.Internal_Error
    lib = hap._lib.lib
    import ctypes as C
    t = Targets(2, ow, oh)
    keep = [np.frombuffer(frame, np.uint8).copy() for _ in range(2)]
    inputs = (C.c_void_p * 2)(*[k.ctypes.data for k in keep])
    lens = (C.c_ulong * 2)(len(frame), len(frame))
    yp = (C.c_void_p * 2)(*[p.data_ptr() for p in t.luma])
    cp = (C.c_void_p * 2)(*[p.data_ptr() for p in t.chroma])
    order = ["frameCount", "inputBuffers", "inputBuffersBytes", "textureCount", "lumaPlanes", "lumaRowBytes", "chromaPlanes",
             "chromaRowBytes", "matrix", "range", "width", "height", "scaleLog2"]
    base = dict(frameCount=2, inputBuffers=inputs, inputBuffersBytes=lens, textureCount=1, lumaPlanes=yp, lumaRowBytes=t.lp,
                chromaPlanes=cp, chromaRowBytes=t.cp, matrix=P.BT709, range=P.LIMITED, width=w, height=h, scaleLog2=s)
    mistakes = {
        "inputBuffers NULL": dict(inputBuffers=None), "inputBuffersBytes NULL": dict(inputBuffersBytes=None),
        "lumaPlanes NULL": dict(lumaPlanes=None), "chromaPlanes NULL": dict(chromaPlanes=None),
        "scaleLog2 3": dict(scaleLog2=3), "scaleLog2 -1": dict(scaleLog2=0xFFFFFFFF),
        "width no multiple of 8": dict(width=w + 4), "height no multiple of 8": dict(height=h + 4),
        "width 0": dict(width=0), "height 0": dict(height=0),
        "lumaRowBytes short": dict(lumaRowBytes=ow - 4), "lumaRowBytes no multiple of 4": dict(lumaRowBytes=t.lp + 2),
        "chromaRowBytes short": dict(chromaRowBytes=ow - 4), "chromaRowBytes no multiple of 4": dict(chromaRowBytes=t.cp + 2),
        "chromaRowBytes of W / 2": dict(chromaRowBytes=ow // 2),
        "more than 65535 output block rows": dict(height=8 * 65536),
        "matrix 2": dict(matrix=2), "range 2": dict(range=2), "matrix -1": dict(matrix=0xFFFFFFFF),
        "textureCount 0": dict(textureCount=0), "textureCount 3": dict(textureCount=3),
    }
    for case, change in mistakes.items():
        a = dict(base, **change)
        res = (C.c_uint * 3)(77, 78, 79)
        assert lib.HapGpuDecodeFramesNV12(ctx.handle, *[a[k] for k in order], res, 0) == bad, case
        assert list(res) == [bad, bad, 79], case
    t.check([None, None], "refusals")
    assert lib.HapGpuDecodeFramesNV12(ctx.handle, *[base[k] for k in order], None, 0) == bad
    # the single-texture call
    tex = dev(textures[0])
    one = Targets(1, ow, oh)
    for case, change in (("scale 3", dict(scale_log2=3)), ("matrix 2", dict(matrix=2)), ("range 2", dict(range=2))):
        assert ctx.decompress_nv12(tex, L.FMT_DXT1, w, h, one.luma[0].data_ptr(), one.chroma[0].data_ptr(), luma_row_bytes=one.lp,
                                   chroma_row_bytes=one.cp, **dict(dict(scale_log2=s), **change)) == bad, case
    assert ctx.decompress_nv12(tex, L.FMT_BC7, w, h, one.luma[0], one.chroma[0], scale_log2=s) == bad
    assert ctx.decompress_nv12(tex, L.FMT_RGTC1, w, h, one.luma[0], one.chroma[0], scale_log2=s) == bad
    assert ctx.decompress_nv12(tex, L.FMT_DXT1, w + 4, h, one.luma[0].data_ptr(), one.chroma[0].data_ptr(), scale_log2=s,
                               luma_row_bytes=one.lp, chroma_row_bytes=one.cp) == bad
    assert ctx.decompress_nv12(tex, L.FMT_DXT1, w, h, one.luma[0].data_ptr() + 1, one.chroma[0], scale_log2=s,
                               luma_row_bytes=one.lp) == bad
    assert ctx.decompress_nv12(tex, L.FMT_DXT1, w, h, one.luma[0], torch.zeros((oh // 2, ow), dtype=torch.uint8).data_ptr(),
                               scale_log2=s, chroma_row_bytes=ow) == bad
    one.check([None], "single refusals")
    # a context between a ...Begin and HapGpuEncodeFramesFinish takes no other call
    rgba = torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.encode_frames_rgba_begin([rgba], 8, 8, 32, [L.FMT_DXT1], [L.COMP_SNAPPY], [1], [out]) == 0
    r, res = ctx.decode_frames_nv12([frame, frame], [len(frame)] * 2, 1, t.luma, t.chroma, w, h, scale_log2=s)
    assert r == internal and res == [internal] * 2
    assert ctx.decompress_nv12(tex, L.FMT_DXT1, w, h, one.luma[0], one.chroma[0], scale_log2=s) == internal
    r, _used, res = ctx.encode_finish()
    assert r == 0 and res == [0]
    t.check([None, None], "busy")
    one.check([None], "busy single")
    # ... and afterwards it does
    r, res = ctx.decode_frames_nv12([frame, frame], [len(frame)] * 2, 1, t.luma, t.chroma, w, h, scale_log2=s)
    assert r == 0 and res == [0, 0]

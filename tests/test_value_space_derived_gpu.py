"""The value-space sweeps (tests/_value_space.py, tests/_bptc_value_space.py) through every other launch that runs the
block decoders' texel code: each instantiates bc_decode_body, bc_decode_scaled_body or bptc_decode_kernel anew (at half
and quarter size with arithmetic of its own: pick counts from popcounts under masks, v_dot4 against the palette, a
third selector layout for the alpha rows, packed 16-bit sums for Hap Q), and random blocks reach a few per cent of the
input space.

  scaled RGBA    HapGpuDecompressRGBAScaled, HapGpuDecodeFramesRGBAScaled              s = 1, 2        BC7 included
  region         HapGpuDecompressRGBARegion, all but one block on every side          s = 0           BC7 included
  planes         HapGpuDecompressPlanes, HapGpuDecompressPlanesRegion (the same rectangle),
                 HapGpuDecompressPlanesResized (crop = output: every tap has weight 0)  s = 0, 1, 2
  composite      HapGpuCompositeTextures, the one layer at opacity 255                 s = 0
  measure        HapGpuMeasureTexture against the expected picture: all sums zero      s = 0

Two sweeps per format: the rotating codes of test_value_space_gpu.py (every c0 == c1; but every region of a block
holds every index equally often, so the region sums are even) and the *_scaled_sweep() forms with random codes and flat
blocks (every residue of the region sums: tests/test_value_space.py).  No expected value comes from the library: it is
the oracle's full-size picture (tests/_data.oracle_bc_decode; BC7: _bptc_value_space.decode_bc7_blocks), box-filtered
with numpy's integers as test_scaled_decode_gpu.box defines it.  Planes are float16 with scale 1 and bias 0, where
bytes are exact, so the compare is the texel's.  Everything is compared by equality; a mismatch reports the first
differing block: its input bytes and both outputs.  Textures lie in host and in device memory in turn."""
import functools

import numpy as np
import pytest

import _bptc_value_space as B
import _composite as K
import _data as D
import _libs as L
import _value_space as V
from test_planes_decode_gpu import CONSTANTS, definition
from test_scaled_decode_gpu import box
from test_value_space_gpu import first_difference, profiled

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
INTEGERS = CONSTANTS["integers"]
BACKGROUND = (17, 34, 51, 128)
CASES = ("dxt1", "dxt5", "hapq", "hapq_alpha")
BLOCK_SOURCES = [(case, sweep) for case in CASES for sweep in ("random_codes", "rotating_codes")]
ALL_SOURCES = BLOCK_SOURCES + [("bc7", "sets")]


def ids(sources):
    return ["%s-%s" % s for s in sources]


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


class Source:
    """A sweep as a texture: blocks [n, b], format, RGTC1 plane [n, 8] | None, w, h and the expected full-size picture
    [h, w, 4] (read-only)"""

    def __init__(self, blocks, fmt, plane, w, h, full):
        self.blocks, self.fmt, self.plane, self.w, self.h, self.full = np.ascontiguousarray(blocks), fmt, plane, w, h, full
        self.full.setflags(write=False)
        self.inputs = self.blocks if plane is None else np.concatenate([self.blocks, plane], axis=1)
        self._device = None

    def textures(self, turn):
        """(texture, plane | None): in host memory on even turns, in device memory on odd ones"""
        if turn % 2 == 0:
            return self.blocks.tobytes(), None if self.plane is None else self.plane.tobytes()
        if self._device is None:
            self._device = (torch.from_numpy(self.blocks).cuda(), None if self.plane is None else torch.from_numpy(self.plane).cuda())
            torch.cuda.synchronize()
        return self._device

    def level(self, s):
        return self.full if s == 0 else box(self.full, s)

    @property
    def inset(self):
        """all but one block on every side: first != 0 and texture_blocks_x != blocks_x in the kernels"""
        return 4, 4, self.w - 8, self.h - 8

    def inset_inputs(self):
        rows = self.inputs.reshape(self.h // 4, self.w // 4, -1)
        return rows[1:-1, 1:-1].reshape(-1, rows.shape[-1])


@functools.lru_cache(maxsize=None)
def source(case, sweep):
    if case == "bc7":
        blocks, w, h = B.texture_of_sets(B.bc7_decode_sets())
        return Source(blocks, L.FMT_BC7, None, w, h, V.picture_of_blocks(B.decode_bc7_blocks(blocks), row=w // 4))
    random_codes = sweep == "random_codes"
    plane = None
    if case == "dxt1":
        blocks, fmt = V.dxt1_scaled_sweep() if random_codes else V.pad_blocks(V.colour_blocks()), L.FMT_DXT1
    elif case == "dxt5":
        blocks, fmt = V.dxt5_scaled_sweep() if random_codes else V.dxt5_sweep(), L.FMT_DXT5
    else:
        blocks, plane = V.hapq_scaled_sweep() if random_codes else V.hapq_sweep()
        fmt = L.FMT_YCOCG
        plane = np.ascontiguousarray(plane) if case == "hapq_alpha" else None
    w, h = 4 * V.BLOCK_ROW, 4 * len(blocks) // V.BLOCK_ROW
    full = D.oracle_bc_decode(np.ascontiguousarray(blocks).tobytes(), fmt, w, h)
    if plane is not None:
        full[..., 3] = D.oracle_bc_decode(plane.tobytes(), L.FMT_RGTC1, w, h)
    return Source(blocks, fmt, plane, w, h, full)


def per_block(img, s):
    """[h, w, c] of a level -> [n, texels of a block at that level, c], block by block"""
    k = 4 >> s
    h, w, c = img.shape
    return img.reshape(h // k, k, w // k, k, c).transpose(0, 2, 1, 3, 4).reshape(-1, k * k, c)


def crop(img, region, s=0):
    x, y, w, h = (v >> s for v in region)
    return img[y: y + h, x: x + w]


def picture_of(buf, w, h):
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.frombuffer(buf, dtype=np.uint8)
    return a[: h * w * 4].reshape(h, w, 4)


def planes_target(w, h):
    t = torch.zeros((4, h, w), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    return t


def planes_bits(t):
    """float16 (4, h, w) -> bit patterns [h, w, 4]"""
    return t.cpu().view(torch.int16).numpy().view(np.uint16).transpose(1, 2, 0)


def expected_bits(picture):
    return definition(picture, "f16", 4, INTEGERS).transpose(1, 2, 0)


def turn_of(*keys):
    """0 or 1 from a case's parameters: where its textures lie"""
    return sum(ALL_SOURCES.index(k) if isinstance(k, tuple) else int(k) for k in keys)


def test_float16_holds_every_byte():
    want = definition(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(4, axis=2), "f16", 4, INTEGERS)
    assert np.array_equal(want.view(np.float16).astype(np.int64), np.arange(256).reshape(1, 16, 16).repeat(4, axis=0))
    assert len(np.unique(want[0])) == 256


# ---------------------------------------------------------------------------------------------- scaled RGBA --
@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("src", ALL_SOURCES, ids=ids(ALL_SOURCES))
def test_decompress_rgba_scaled_sweeps(ctx, src, s):
    c = source(*src)
    tex, plane = c.textures(turn_of(src, s))
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_rgba_scaled(tex, c.fmt, c.w, c.h, s, alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(per_block(picture_of(got, c.w >> s, c.h >> s), s), per_block(c.level(s), s), c.inputs,
                     "HapGpuDecompressRGBAScaled %s %s s = %d" % (src + (s,)))


FRAME_CASES = CASES + ("bc7",)


@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("case", FRAME_CASES)
def test_decode_frames_rgba_scaled_sweeps(ctx, hap, case, s):
    """The batch kernel on two frames of the sweep (one in HBM, one on the host), pictures in HBM."""
    c = source(case, "sets" if case == "bc7" else "random_codes")
    textures = [c.blocks.tobytes()] + ([c.plane.tobytes()] if c.plane is not None else [])
    fmts = [c.fmt] + ([L.FMT_RGTC1] if c.plane is not None else [])
    T = len(fmts)
    r, frame = ORA.encode(textures, fmts, [L.COMP_SNAPPY] * T, [4] * T)
    assert r == 0
    frames = [torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda(), frame]
    ow, oh = c.w >> s, c.h >> s
    pics = [torch.zeros(oh * ow * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    flags = hap.DECODE_BPTC_PICTURES if case == "bc7" else 0
    (r, res), launches = profiled(ctx, lambda: ctx.decode_frames_rgba_scaled(frames, [len(frame)] * 2, T, pics, c.w, c.h, s,
                                                                             flags=flags))
    assert r == 0 and res == [0, 0] and launches["block_decode"] >= 1, (r, res, launches)
    want = per_block(c.level(s), s)
    for i, pic in enumerate(pics):
        first_difference(per_block(picture_of(pic, ow, oh), s), want, c.inputs,
                         "HapGpuDecodeFramesRGBAScaled %s s = %d frame %d" % (case, s, i))


# --------------------------------------------------------------------------------------------------- region --
@pytest.mark.parametrize("src", ALL_SOURCES, ids=ids(ALL_SOURCES))
def test_decompress_rgba_region_sweeps(ctx, src):
    c = source(*src)
    tex, plane = c.textures(turn_of(src))
    (r, got), launches = profiled(ctx, lambda: ctx.decompress_rgba_region(tex, c.fmt, c.w, c.h, c.inset, alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(per_block(picture_of(got, c.w - 8, c.h - 8), 0), per_block(crop(c.full, c.inset), 0), c.inset_inputs(),
                     "HapGpuDecompressRGBARegion %s %s" % src)


# --------------------------------------------------------------------------------------------------- planes --
@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("src", BLOCK_SOURCES, ids=ids(BLOCK_SOURCES))
def test_decompress_planes_sweeps(ctx, src, s):
    c = source(*src)
    tex, plane = c.textures(turn_of(src, s, 1))
    out = planes_target(c.w >> s, c.h >> s)
    r, launches = profiled(ctx, lambda: ctx.decompress_planes(tex, c.fmt, c.w, c.h, out, scale_log2=s, scale=INTEGERS[0],
                                                               bias=INTEGERS[1], alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(per_block(planes_bits(out), s), per_block(expected_bits(c.level(s)), s), c.inputs,
                     "HapGpuDecompressPlanes (float16 bit patterns) %s %s s = %d" % (src + (s,)))


@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("src", BLOCK_SOURCES, ids=ids(BLOCK_SOURCES))
def test_decompress_planes_region_sweeps(ctx, src, s):
    c = source(*src)
    tex, plane = c.textures(turn_of(src, s))
    out = planes_target((c.w - 8) >> s, (c.h - 8) >> s)
    r, launches = profiled(ctx, lambda: ctx.decompress_planes_region(tex, c.fmt, c.w, c.h, c.inset, out, scale_log2=s,
                                                                      scale=INTEGERS[0], bias=INTEGERS[1], alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(per_block(planes_bits(out), s), per_block(expected_bits(crop(c.level(s), c.inset, s)), s),
                     c.inset_inputs(), "HapGpuDecompressPlanesRegion (float16 bit patterns) %s %s s = %d" % (src + (s,)))


@pytest.mark.parametrize("s", (0, 1, 2))
@pytest.mark.parametrize("src", BLOCK_SOURCES, ids=ids(BLOCK_SOURCES))
def test_decompress_planes_resized_sweeps(ctx, src, s):
    """A crop of the whole level to its own size: every tap has weight 0, the resampler is the identity."""
    c = source(*src)
    tex, plane = c.textures(turn_of(src, s, 1))
    ow, oh = c.w >> s, c.h >> s
    out = planes_target(ow, oh)
    r, launches = profiled(ctx, lambda: ctx.decompress_planes_resized(tex, c.fmt, c.w, c.h, (0, 0, ow, oh), out, scale_log2=s,
                                                                       scale=INTEGERS[0], bias=INTEGERS[1], alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    first_difference(per_block(planes_bits(out), s), per_block(expected_bits(c.level(s)), s), c.inputs,
                     "HapGpuDecompressPlanesResized (float16 bit patterns) %s %s s = %d" % (src + (s,)))


# ------------------------------------------------------------------------------------- composite and measure --
@pytest.mark.parametrize("src", BLOCK_SOURCES, ids=ids(BLOCK_SOURCES))
def test_composite_textures_sweeps(ctx, src):
    """One layer at opacity 255: an opaque one (DXT1, Hap Q) replaces the canvas, one with alpha blends over it."""
    c = source(*src)
    tex, plane = c.textures(turn_of(src, 1))
    (r, got), launches = profiled(ctx, lambda: ctx.composite_textures([(tex, c.fmt, plane)], c.w, c.h, opacities=[255],
                                                                       background=BACKGROUND))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    if src[0] in ("dxt1", "hapq"):
        assert (c.full[..., 3] == 255).all()
        want = c.full
    else:
        want = K.composite([c.full], [255], BACKGROUND)
        assert not np.array_equal(want, c.full)
    first_difference(per_block(picture_of(got, c.w, c.h), 0), per_block(want, 0), c.inputs, "HapGpuCompositeTextures %s %s" % src)


@pytest.mark.parametrize("src", BLOCK_SOURCES, ids=ids(BLOCK_SOURCES))
def test_measure_texture_sweeps(ctx, src):
    """sse == 0 holds only if every texel is right.  Then one byte of the last block's reference changes."""
    c = source(*src)
    tex, plane = c.textures(turn_of(src))
    reference = torch.from_numpy(np.array(c.full)).cuda()             # (a writable copy: torch refuses read-only arrays)
    torch.cuda.synchronize()
    (r, error), launches = profiled(ctx, lambda: ctx.measure_texture(tex, c.fmt, c.w, c.h, reference, alpha=plane))
    assert r == 0 and launches["block_decode"] >= 1, (r, launches)
    assert (error.sse, error.sad, error.texels) == ((0,) * 4, (0,) * 4, c.w * c.h), (src, error.sse, error.sad)
    touched = np.array(c.full)
    y, x = c.h - 2, c.w - 3
    touched[y, x, 1] = int(touched[y, x, 1]) + (3 if touched[y, x, 1] <= 252 else -3)
    reference = torch.from_numpy(touched).cuda()
    torch.cuda.synchronize()
    r, error = ctx.measure_texture(tex, c.fmt, c.w, c.h, reference, alpha=plane)
    assert r == 0 and (error.sse, error.sad, error.texels) == ((0, 9, 0, 0), (0, 3, 0, 0), c.w * c.h), (src, error.sse, error.sad)

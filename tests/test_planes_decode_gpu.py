"""Normalised planar float tensors straight from block textures and Hap frames (HapGpuDecompressPlanes,
HapGpuDecodeFramesPlanes).  The definition is exact: for the byte v of the full-size, half-size or quarter-size RGBA8
picture, element = float32(v) * float32(scale[c]) + float32(bias[c]) (two roundings), then rounded to nearest even to
half, bfloat16 or kept.  Every expected tensor is computed on the CPU -- the checker's full-size decode
(tests/_data.oracle_bc_decode), box-filtered with numpy, numpy's float arithmetic, numpy's float16 and torch-CPU's
bfloat16 -- and every comparison is on bit patterns: every bit must match, and every byte that is not a written element
must still hold the sentinel."""
import ctypes as C
import functools

import numpy as np
import pytest

import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
SCALES = (0, 1, 2)
CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
# one lane; the smallest two-lane grids; exactly 64 blocks a row; 65 a row (a wave crosses a block row, 195 blocks: less
# than a workgroup); 387 blocks (a partly filled second workgroup)
GEOMETRIES = ((4, 4), (8, 4), (4, 8), (256, 8), (260, 12), (516, 12))
KINDS = {"f16": (torch.float16, np.uint16), "bf16": (torch.bfloat16, np.uint16), "f32": (torch.float32, np.uint32)}
PAD = 64                                                    # sentinel bytes in front of and behind every tensor

STD = (0.229, 0.224, 0.225, 1.0)
MEAN = (0.485, 0.456, 0.406, 0.0)
CONSTANTS = {
    "integers": ((1.0,) * 4, (0.0,) * 4),                   # exact integers
    "imagenet": (tuple(1.0 / (255.0 * s) for s in STD), tuple(-m / s for m, s in zip(MEAN, STD))),
    "subnormal_halves": ((2.0 ** -20,) * 4, (0.0,) * 4),    # bytes 1 to 63 become subnormal halves
}
DEFAULT = ((1.0 / 255.0,) * 4, (0.0,) * 4)                  # what the Python methods pass when given none


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


def box(img, s):
    """[h, w, c] uint8 -> [h >> s, w >> s, c]: (sum + (1 << (2s - 1))) >> 2s"""
    if s == 0:
        return img
    k = 1 << s
    h, w, c = img.shape
    sums = img.astype(np.uint32).reshape(h // k, k, w // k, k, c).sum(axis=(1, 3))
    return ((sums + (1 << (2 * s - 1))) >> (2 * s)).astype(np.uint8)


def definition(picture, kind, channels, constants):
    """The bit patterns [channels, h, w] the definition gives for an RGBA8 picture [h, w, 4] of the output's size"""
    scale, bias = constants
    planes = np.empty((channels,) + picture.shape[:2], dtype=np.float32)
    for c in range(channels):
        planes[c] = picture[..., c].astype(np.float32) * np.float32(scale[c]) + np.float32(bias[c])
    if kind == "f32":
        return planes.view(np.uint32)
    if kind == "f16":
        return planes.astype(np.float16).view(np.uint16)
    return torch.from_numpy(planes).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def full_size(case, tex, plane, w, h):
    """What the CPU checker makes of a texture (and its RGTC1 plane) at full size."""
    pic = D.oracle_bc_decode(tex, FORMATS[case], w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(plane, L.FMT_RGTC1, w, h)
    return pic


@functools.lru_cache(maxsize=None)
def random_texture(case, w, h):
    """Seeded random bytes: any 8 / 16 bytes are a block.  (texture, plane | None, full-size picture); made once"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([CASES.index(case), w, h])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    pic = full_size(case, tex, plane, w, h)
    pic.setflags(write=False)
    return tex, plane, pic


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


class Target:
    """A sentinel-filled device buffer and a tensor (channels, oh, ow) of `kind` somewhere in it: `first` elements
    behind PAD bytes, planes `plane` and rows `row` elements apart."""

    def __init__(self, kind, channels, oh, ow, row=None, plane=None, first=0, planes_held=None):
        dtype, self.bits = KINDS[kind]
        self.e = np.dtype(self.bits).itemsize
        self.shape = (channels, oh, ow)
        self.row = row or ow
        self.plane = plane or self.row * oh
        self.start = PAD + first * self.e
        nbytes = self.start + (planes_held or channels) * self.plane * self.e + PAD
        self.buffer = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        elements = self.buffer[self.start: self.start + (nbytes - self.start) // self.e * self.e].view(dtype)
        self.tensor = torch.as_strided(elements, self.shape, (self.plane, self.row, 1))
        torch.cuda.synchronize()

    def read(self):
        """(the elements' bit patterns [channels, oh, ow], every other byte of the buffer)"""
        raw = self.buffer.cpu().numpy()
        channels, oh, ow = self.shape
        offsets = (self.start + self.e * (np.arange(channels)[:, None, None] * self.plane
                                          + np.arange(oh)[None, :, None] * self.row + np.arange(ow)[None, None, :]))
        written = np.zeros(raw.size, dtype=bool)
        got = np.zeros(self.shape, dtype=self.bits)
        for b in range(self.e):                              # (little endian)
            written[offsets + b] = True
            got |= raw[offsets + b].astype(self.bits) << (8 * b)
        return got, raw[~written]

    def untouched(self):
        return bool((self.buffer.cpu().numpy() == SENTINEL).all())


def check(target, want, note):
    got, rest = target.read()
    assert np.array_equal(got, want), (note, np.argwhere(got != want)[:4].tolist())
    assert (rest == SENTINEL).all(), note


def test_the_constants_are_finite_and_normal():
    tiny = np.finfo(np.float32).tiny
    for name, (scale, bias) in list(CONSTANTS.items()) + [("default", DEFAULT)]:
        for v in scale + bias:
            f = np.float32(v)
            assert np.isfinite(f) and (f == 0 or abs(f) >= tiny), (name, v)
    # ... and what the third set is for: bytes 1 to 63 are subnormal halves, none of them zero
    halves = (np.arange(1, 64).astype(np.float32) * np.float32(2.0 ** -20)).astype(np.float16).view(np.uint16)
    assert ((halves & 0x7C00) == 0).all() and ((halves & 0x03FF) != 0).all()


# ------------------------------------------------------------------ 1. every block pattern, every edge of the grid --
@pytest.mark.parametrize("size", GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_random_blocks_at_every_edge_of_the_grid(ctx, case, size):
    w, h = size
    tex, plane, full = random_texture(case, w, h)
    dtex, dplane = dev(tex), dev(plane) if plane else None
    for s in SCALES:
        want = definition(box(full, s), "f16", 4, DEFAULT)
        for t, p in ((tex, plane), (dtex, dplane)):
            target = Target("f16", 4, h >> s, w >> s)
            assert ctx.decompress_planes(t, FORMATS[case], w, h, target.tensor, scale_log2=s, alpha=p) == 0, s
            check(target, want, s)


# ------------------------------------------------------------------------------------------------ 2. the conversion --
@pytest.mark.parametrize("constants", sorted(CONSTANTS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_conversion_is_exact(ctx, kind, constants):
    w, h = 260, 12
    tex, plane, full = random_texture("ycocg_alpha", w, h)
    scale, bias = CONSTANTS[constants]
    assert set(range(1, 64)) <= set(np.unique(full).tolist())
    for s in SCALES:
        for channels in (3, 4):
            want = definition(box(full, s), kind, channels, CONSTANTS[constants])
            if constants == "subnormal_halves" and kind == "f16" and s == 0:
                assert (((want & 0x7C00) == 0) & ((want & 0x03FF) != 0)).any()          # kept, not flushed
            # (four planes held, three written: the fourth stays as it was)
            target = Target(kind, channels, h >> s, w >> s, planes_held=4)
            r = ctx.decompress_planes(tex, L.FMT_YCOCG, w, h, target.tensor, scale_log2=s, scale=scale[:channels],
                                      bias=bias[:channels], alpha=plane)
            assert r == 0, (s, channels)
            check(target, want, (s, channels))


# ---------------------------------------------------------------------------------------- 3. strides and alignment --
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("s", (0, 2))
def test_a_tensor_sliced_out_of_a_larger_one(ctx, kind, s):
    w, h = 260, 12
    tex, plane, full = random_texture("ycocg_alpha", w, h)
    oh, ow = h >> s, w >> s
    dtype, bits = KINDS[kind]
    e = np.dtype(bits).itemsize
    big = torch.full((5 * (oh + 3) * (ow + 8) * e,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype)
    big = big.view(5, oh + 3, ow + 8)
    out = big[1:5, 1: 1 + oh, 4: 4 + ow]
    assert out.stride() == ((oh + 3) * (ow + 8), ow + 8, 1) and not out.is_contiguous()
    assert ctx.decompress_planes(tex, L.FMT_YCOCG, w, h, out, scale_log2=s, scale=CONSTANTS["imagenet"][0],
                                 bias=CONSTANTS["imagenet"][1], alpha=plane) == 0
    want = definition(box(full, s), kind, 4, CONSTANTS["imagenet"])
    raw = big.cpu().view({2: torch.int16, 4: torch.int32}[e]).numpy().view(bits)
    assert np.array_equal(raw[1:5, 1: 1 + oh, 4: 4 + ow], want)
    sentinel = np.frombuffer(bytes([SENTINEL]) * e, dtype=bits)[0]
    raw = raw.copy()
    raw[1:5, 1: 1 + oh, 4: 4 + ow] = sentinel
    assert (raw == sentinel).all()                          # row tails, plane gaps, the plane in front


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_alignment_rule(ctx, hap, kind):
    w, h = 260, 12
    tex, plane, full = random_texture("ycocg_alpha", w, h)
    # one element off at full size: a lane's four elements are no longer aligned
    target = Target(kind, 4, h, w, first=1)
    assert ctx.decompress_planes(tex, L.FMT_YCOCG, w, h, target.tensor, alpha=plane) == hap.HapResult.Bad_Arguments
    assert target.untouched()
    # ... at quarter size a lane stores one element: legal
    target = Target(kind, 4, h >> 2, w >> 2, first=1)
    assert ctx.decompress_planes(tex, L.FMT_YCOCG, w, h, target.tensor, scale_log2=2, alpha=plane) == 0
    check(target, definition(box(full, 2), kind, 4, DEFAULT), kind)


def test_sources_out_of_scope_are_refused(ctx, hap):
    target = Target("f16", 4, 4, 4)
    for fmt in (L.FMT_BC7, L.FMT_RGTC1, 0x8E8F, 0x8E8E):
        assert ctx.decompress_planes(bytes(16), fmt, 4, 4, target.tensor) == hap.HapResult.Bad_Arguments, fmt
    assert target.untouched()


# ---------------------------------------------------------------------------------------------------- 4. frames --
W, H = 64, 32
NB = (W // 4) * (H // 4)


def frames_of(ctx, hap, fmts, pictures, w, h, flags=0):
    """One Hap frame per RGBA picture (textures of `fmts`), made by encode_frames_rgba: list of bytes"""
    sizes = [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]
    chunks = [2] * len(fmts)
    bufs = [np.zeros(hap.HapMaxEncodedLength(sizes, fmts, chunks), dtype=np.uint8) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba([np.ascontiguousarray(p) for p in pictures], w, h, w * 4, fmts, [1] * len(fmts),
                                          chunks, bufs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return [b[:u].tobytes() for b, u in zip(bufs, used)]


def hap_encode(hap, textures, fmts):
    r, frame = hap.HapEncode(list(textures), list(fmts), [1] * len(fmts), [2] * len(fmts))
    assert r == 0
    return frame


def textures_of(ctx, frames, index, cap):
    """What decode_frames yields for every frame: list of (result, texture bytes, format)"""
    outs = [np.zeros(cap, dtype=np.uint8) for _ in frames]
    _r, used, fmts, res = ctx.decode_frames(frames, [len(f) for f in frames], index, outs)
    return [(res[i], outs[i][: used[i]].tobytes(), fmts[i]) for i in range(len(frames))]


def oracle_pictures(ctx, frames, texture_count, good):
    """frame index -> full-size picture, from the textures decode_frames yields (texture_count 1: the first alone)"""
    first = textures_of(ctx, frames, 0, NB * 16)
    second = textures_of(ctx, frames, 1, NB * 8) if texture_count == 2 else None
    out = {}
    for i in good:
        code, tex, fmt = first[i]
        assert code == 0 and len(tex) == NB * D.BLOCK_BYTES[fmt], i
        case = {L.FMT_DXT1: "dxt1", L.FMT_DXT5: "dxt5", L.FMT_YCOCG: "ycocg"}[fmt]
        plane = None
        if second:
            code, plane, pfmt = second[i]
            assert code == 0 and pfmt == L.FMT_RGTC1 and len(plane) == NB * 8, i
        out[i] = full_size(case, tex, plane, W, H)
    return out


@pytest.fixture(scope="module")
def batches(ctx, hap):
    """name -> (frames, texture_count, full-size CPU pictures by frame); made once.  Frames by HapEncode (of random
    blocks) and by encode_frames_rgba with the fragment table."""
    table = hap.ENCODE_FRAGMENT_INDEX
    out = {}
    mixed = [hap_encode(hap, [random_texture("dxt1", W, H)[0]], [L.FMT_DXT1]),
             frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1)], W, H, flags=table)[0],
             hap_encode(hap, [random_texture("ycocg", W, H)[0]], [L.FMT_YCOCG]),
             frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3)], W, H, flags=table)[0],
             frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 4)], W, H)[0]]
    out["mixed"] = (mixed, 1, oracle_pictures(ctx, mixed, 1, range(5)))
    assert np.array_equal(out["mixed"][2][0], random_texture("dxt1", W, H)[2])
    tex, plane, _full = random_texture("ycocg_alpha", W, H)
    qa = ([hap_encode(hap, [tex, plane], [L.FMT_YCOCG, L.FMT_RGTC1])]
          + frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 5), D.rgba(W, H, 6)], W, H, flags=table)
          + frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 7)], W, H))
    out["hap_q_alpha"] = (qa, 2, oracle_pictures(ctx, qa, 2, range(4)))
    assert np.array_equal(out["hap_q_alpha"][2][0], random_texture("ycocg_alpha", W, H)[2])
    return out


def sibling_pictures(ctx, frames, count, s):
    """What decode_frames_rgba (s 0) or decode_frames_rgba_scaled writes for the frames: [n, H >> s, W >> s, 4]"""
    n = len(frames)
    pics = [np.zeros((H >> s) * (W >> s) * 4, dtype=np.uint8) for _ in range(n)]
    lens = [len(f) for f in frames]
    if s == 0:
        r, res = ctx.decode_frames_rgba(frames, lens, count, pics, W, H)
    else:
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, count, pics, W, H, s)
    assert r == 0 and res == [0] * n
    return [p.reshape(H >> s, W >> s, 4) for p in pics]


def test_a_mixed_batch_into_one_tensor(ctx, batches):
    frames, count, full = batches["mixed"]
    s, kind, constants = 1, "f16", CONSTANTS["imagenet"]
    # one (5, 3, H, W) tensor: frame f's planes behind frame f - 1's
    target = Target(kind, 5 * 3, H >> s, W >> s)
    out = target.tensor.view(5, 3, H >> s, W >> s)
    r, res = ctx.decode_frames_planes(frames, [len(f) for f in frames], count, out, W, H, scale_log2=s,
                                      scale=constants[0][:3], bias=constants[1][:3])
    assert r == 0 and res == [0] * 5
    want = np.concatenate([definition(box(full[i], s), kind, 3, constants) for i in range(5)])
    check(target, want, "definition")
    long_way = np.concatenate([definition(p, kind, 3, constants) for p in sibling_pictures(ctx, frames, count, s)])
    check(target, long_way, "sibling")


@pytest.mark.parametrize("s,kind,channels", ((0, "bf16", 4), (1, "f32", 4), (2, "f16", 4), (0, "f16", 3)))
def test_hap_q_alpha_frames(ctx, batches, s, kind, channels):
    frames, count, full = batches["hap_q_alpha"]
    n, constants = len(frames), CONSTANTS["imagenet"]
    # a list of tensors with longer rows and planes, sharing their strides
    ow, oh = W >> s, H >> s
    targets = [Target(kind, channels, oh, ow, row=ow + 4, plane=(ow + 4) * (oh + 1)) for _ in range(n)]
    r, res = ctx.decode_frames_planes(frames, [len(f) for f in frames], count, [t.tensor for t in targets], W, H,
                                      scale_log2=s, scale=constants[0][:channels], bias=constants[1][:channels])
    assert r == 0 and res == [0] * n
    siblings = sibling_pictures(ctx, frames, count, s)
    for i in range(n):
        check(targets[i], definition(box(full[i], s), kind, channels, constants), ("definition", i))
        check(targets[i], definition(siblings[i], kind, channels, constants), ("sibling", i))


@pytest.mark.parametrize("s", SCALES)
def test_one_launch_per_format_present_in_the_existing_class(ctx, batches, s):
    frames, count, _full = batches["mixed"]
    out = torch.empty((5, 3, H >> s, W >> s), dtype=torch.float16, device="cuda")
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.decode_frames_planes(frames, [len(f) for f in frames], count, out, W, H, scale_log2=s)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 3, prof["block_decode"]


# ---------------------------------------------------------------------------------------- 5. per-frame failures --
@pytest.mark.parametrize("bptc_flag", (False, True))
def test_a_bad_frame_fails_alone(ctx, hap, batches, bptc_flag):
    good, _count, full = batches["mixed"]
    bad, broken = hap.HapResult.Bad_Arguments, hap.HapResult.Bad_Frame
    hap_r = frames_of(ctx, hap, [L.FMT_BC7], [D.rgba(W, H, 8)], W, H, flags=hap.ENCODE_BPTC_BLOCKS)[0]
    small = frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(32, 32, 9)], 32, 32)[0]
    #         good     Hap R  good     other size  truncated      good     no tensor  good
    frames = [good[0], hap_r, good[1], small, good[2][:-3], good[3], good[4], good[2]]
    source = [0, None, 1, None, None, 3, None, 2]
    expect = [0, bad, 0, bad, broken, 0, bad, 0]
    s, kind, constants = 1, "bf16", CONSTANTS["imagenet"]
    targets = [Target(kind, 3, H >> s, W >> s) for _ in frames]
    out = [None if i == 6 else t.tensor for i, t in enumerate(targets)]
    r, res = ctx.decode_frames_planes(frames, [len(f) for f in frames], 1, out, W, H, scale_log2=s, scale=constants[0][:3],
                                      bias=constants[1][:3], flags=hap.DECODE_BPTC_PICTURES if bptc_flag else 0)
    assert res == expect and r == bad
    for i, t in enumerate(targets):
        if source[i] is None:
            assert t.untouched(), i
        else:
            check(t, definition(box(full[source[i]], s), kind, 3, constants), i)


# --------------------------------------------------------------------------------------- 6. whole-call refusals --
def test_whole_call_refusals(ctx, hap, batches):
    frames, count, _full = batches["mixed"]
    lib = hap._lib.lib
    n, bad = len(frames), hap.HapResult.Bad_Arguments
    e, row, plane = 2, W * 2, W * H * 2                     # half elements at full size: a lane stores 8 bytes a row
    targets = [Target("f16", 4, H, W) for _ in frames]
    keep = [np.frombuffer(f, dtype=np.uint8) for f in frames]
    ptrs = (C.c_void_p * n)(*[k.ctypes.data for k in keep])
    lens = (C.c_ulong * n)(*[len(f) for f in frames])
    outs = (C.c_void_p * n)(*[t.tensor.data_ptr() for t in targets])
    scale, bias = (C.c_float * 4)(*DEFAULT[0]), (C.c_float * 4)(*DEFAULT[1])

    def call(width=W, height=H, s=0, channels=4, element=0, plane_bytes=plane, row_bytes=row, arrays=None):
        a = dict(ptrs=ptrs, lens=lens, outs=outs, scale=scale, bias=bias)
        a.update(arrays or {})
        res = (C.c_uint * n)(*([77] * n))
        r = lib.HapGpuDecodeFramesPlanes(ctx.handle, n, a["ptrs"], a["lens"], count, a["outs"], width, height, s, channels,
                                         element, plane_bytes, row_bytes, a["scale"], a["bias"], res, 0)
        return r, list(res)

    refusals = {
        "channels 2": dict(channels=2), "channels 5": dict(channels=5), "element 3": dict(element=3),
        "scaleLog2 3": dict(s=3), "width 6": dict(width=6),
        "rowBytes too short": dict(row_bytes=row - 8), "planeBytes too short": dict(plane_bytes=plane - 8),
        "rowBytes off the unit": dict(row_bytes=row + e), "planeBytes off the unit": dict(plane_bytes=plane + e),
        "no frames": dict(arrays=dict(ptrs=None)), "no sizes": dict(arrays=dict(lens=None)),
        "no tensors": dict(arrays=dict(outs=None)), "no scale": dict(arrays=dict(scale=None)),
        "no bias": dict(arrays=dict(bias=None)),
    }
    for name, arguments in refusals.items():
        assert call(**arguments) == (bad, [bad] * n), name
        assert all(t.untouched() for t in targets), name
    # ... and the same call with nothing wrong
    assert call() == (0, [0] * n)
    assert not any(t.untouched() for t in targets)

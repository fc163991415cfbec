"""A crop per frame of block textures and Hap frames, at any texel position and size, resized to one output size and
written as planar float tensors (HapGpuDecompressPlanesResized, HapGpuDecodeFramesPlanesResized).  No expected value comes
from the calls under test: the picture P is the CPU checker's full-size decode box-filtered with numpy (textures) or what
decode_frames_rgba / decode_frames_rgba_scaled write (frames), the resized crop is tests/_resample.py's numpy definition
of it, and the elements are test_planes_decode_gpu.definition's -- compared as raw bits, in sentinel-filled buffers whose
other bytes must stay sentinel.  Where the crop equals the output and lies on the block grid the bits are also
decompress_planes_region's.

The kernel's output tile is 64 x 4 elements: 65 x 5 outputs cross a tile seam in both axes, and a 516 x 20 texture taken
whole to 129 x 5 makes the first tile's footprint 65 x 5 blocks, more than the 256 a pass of its first phase holds."""
import ctypes as C

import numpy as np
import pytest

import _data as D
import _libs as L
import _resample as S
import test_planes_decode_gpu as P
import test_region_decode_gpu as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = P.SENTINEL
CONSTANTS = P.CONSTANTS["imagenet"]
ELEMENT = {"f16": 0, "bf16": 1, "f32": 2}                       # HapGpuPlaneElement
KINDS = sorted(P.KINDS)
RATIO = 4                                                       # a crop is at most 4 x the output per axis


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


def constants_for(channels):
    return CONSTANTS[0][:channels], CONSTANTS[1][:channels]


def padded_target(kind, channels, out_size):
    """A tensor of the output's size inside a larger sentinel-filled one: a first element one element in, rows 3 elements
    longer, planes a row longer -- the plain rule asks for multiples of the element only"""
    ow, oh = out_size
    return P.Target(kind, channels, oh, ow, row=ow + 3, plane=(ow + 3) * (oh + 1), first=1)


def expected(picture, crop, out_size, kind, channels):
    """The definition's bits for the crop of picture [h, w, 4] (the level's) resized to out_size"""
    return P.definition(S.resample(picture, crop, out_size), kind, channels, constants_for(channels))


def within_cap(crop, out_size):
    return crop[2] <= RATIO * out_size[0] and crop[3] <= RATIO * out_size[1]


# ------------------------------------------------------------------------------------- 1. the identity: an exact crop --
@pytest.mark.parametrize("size", ((260, 12), (516, 12)), ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", P.CASES)
def test_a_crop_of_the_output_size_is_the_region_call_bit_for_bit(ctx, case, size):
    w, h = size
    tex, plane, full = P.random_texture(case, w, h)
    dtex, dplane = P.dev(tex), P.dev(plane) if plane else None
    fmt = P.FORMATS[case]
    for s in P.SCALES:
        level = P.box(full, s)
        for k, kind in enumerate(KINDS):
            channels = 3 + (k + s) % 2
            scale, bias = constants_for(channels)
            for region in R.edge_regions(w, h):
                crop = tuple(v >> s for v in region)
                out_size = crop[2:]
                note = (s, kind, channels, region)
                theirs = P.Target(kind, channels, out_size[1], out_size[0])
                assert ctx.decompress_planes_region(dtex, fmt, w, h, region, theirs.tensor, scale_log2=s, scale=scale,
                                                    bias=bias, alpha=dplane) == 0, note
                want = theirs.read()[0]
                assert np.array_equal(want, expected(level, crop, out_size, kind, channels)), note
                host = kind == "f16"                          # (textures on the host for one kind, in device memory otherwise)
                target = padded_target(kind, channels, out_size)
                r = ctx.decompress_planes_resized(tex if host else dtex, fmt, w, h, crop, target.tensor, scale_log2=s,
                                                  scale=scale, bias=bias, alpha=plane if host else dplane)
                assert r == 0, note
                P.check(target, want, note)


# ---------------------------------------------------------------------------------------------------- 2. sampling --
def crops_of(lw, lh):
    """Crops off the grid of a level of lw x lh texels: the issue's, cut to the level where it is smaller"""
    return [(1, 1, min(255, lw - 1), min(9, lh - 1)), (3, 2, min(5, lw - 3), min(7, lh - 2)), (lw - 1, lh - 1, 1, 1),
            (0, 0, lw, lh)]


def out_sizes_of(crop):
    cw, ch = crop[2:]
    return [(1, 1), (2 * cw + 1, 2 * ch + 1), (-(-cw // 4), -(-ch // 4)), (-(-cw // 3), ch), (65, 5)]


def sample_texture(ctx, hap, case, w, h, s, pairs):
    """Every (crop, out size) of `pairs` at level s, kinds, channel counts and where the texture lives taking turns; a pair
    over the ratio cap is refused and nothing written"""
    tex, plane, full = P.random_texture(case, w, h)
    dtex, dplane = P.dev(tex), P.dev(plane) if plane else None
    level = P.box(full, s)
    for j, (crop, out_size) in enumerate(pairs):
        kind, channels, host = KINDS[j % 3], 3 + j % 2, j % 5 == 0
        scale, bias = constants_for(channels)
        note = (case, s, crop, out_size, kind, channels)
        target = padded_target(kind, channels, out_size)
        r = ctx.decompress_planes_resized(tex if host else dtex, P.FORMATS[case], w, h, crop, target.tensor, scale_log2=s,
                                          scale=scale, bias=bias, alpha=plane if host else dplane)
        if not within_cap(crop, out_size):
            assert r == hap.HapResult.Bad_Arguments and target.untouched(), note
            continue
        assert r == 0, note
        P.check(target, expected(level, crop, out_size, kind, channels), note)


@pytest.mark.parametrize("size", ((260, 12), (516, 12)), ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", P.CASES)
def test_crops_off_the_grid_at_every_ratio(ctx, hap, case, size):
    w, h = size
    taken = 0
    for s in P.SCALES:
        pairs = [(crop, out_size) for crop in crops_of(w >> s, h >> s) for out_size in out_sizes_of(crop)]
        taken += sum(within_cap(*p) for p in pairs)
        sample_texture(ctx, hap, case, w, h, s, pairs)
    assert taken >= 40                                          # (most pairs are within the cap: the refusals are the rest)


@pytest.mark.parametrize("case", P.CASES)
def test_a_footprint_of_more_blocks_than_one_pass_holds(ctx, hap, case):
    # 129 x 5 outputs of 516 x 20 texels: ratio 4 in both axes, the first tile 255 x 15 texels -- 65 x 5 blocks at full
    # size, 255 x 15 at quarter size of a texture four times the size
    sample_texture(ctx, hap, case, 516, 20, 0, [((0, 0, 516, 20), (129, 5)), ((1, 1, 515, 19), (129, 5))])
    sample_texture(ctx, hap, case, 2064, 80, 2, [((0, 0, 516, 20), (129, 5))])
    sample_texture(ctx, hap, case, 1032, 40, 1, [((0, 0, 516, 20), (129, 5))])


# -------------------------------------------------------------------------------------------------------- 3. frames --
W, H = R.W, R.H                                   # 64 x 32, two chunks
OUT = {0: (12, 6), 1: (6, 3), 2: (3, 2)}          # the output per level: the cap is a crop of 48 x 24, 24 x 12, 12 x 8
GOOD_CROPS = ((1, 1, 33, 17), (16, 8, 48, 24), (63, 31, 1, 1), (5, 3, 20, 9), (30, 2, 7, 23))    # at full size


def level_pictures(ctx, frames, count, w, h, s, flags=0):
    """The pictures P of the definition: what decode_frames_rgba (s 0) or decode_frames_rgba_scaled writes, [n, h >> s, w >> s, 4]"""
    pics = [np.zeros((h >> s) * (w >> s) * 4, dtype=np.uint8) for _ in frames]
    lens = [len(f) for f in frames]
    if s == 0:
        r, res = ctx.decode_frames_rgba(frames, lens, count, pics, w, h, flags=flags)
    else:
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, count, pics, w, h, s, flags=flags)
    assert r == 0 and res == [0] * len(frames), res
    return np.stack(pics).reshape(len(frames), h >> s, w >> s, 4)


def resized_frames(ctx, frames, count, w, h, crops, out_size, s, kind, channels, flags=0):
    """decode_frames_planes_resized into padded targets: (result, results, targets)"""
    targets = [padded_target(kind, channels, out_size) for _ in frames]
    scale, bias = constants_for(channels)
    r, res = ctx.decode_frames_planes_resized(frames, [len(f) for f in frames], count, [t.tensor for t in targets], w, h,
                                              crops, out_size, scale_log2=s, scale=scale, bias=bias, flags=flags)
    return r, res, targets


@pytest.mark.parametrize("s", P.SCALES)
def test_mixed_frames_with_a_crop_each_and_the_ones_that_fail_alone(ctx, hap, s):
    bad = hap.HapResult.Bad_Arguments
    kind, channels = KINDS[s], 3 + s % 2
    pictures = [D.rgba(W, H, i) for i in range(5)]
    hapq_alpha = R.frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], pictures[2:3], W, H)
    good = (R.frames_of(ctx, hap, [L.FMT_DXT1], pictures[0:1], W, H) + R.frames_of(ctx, hap, [L.FMT_YCOCG], pictures[1:2], W, H)
            + hapq_alpha + R.frames_of(ctx, hap, [L.FMT_DXT5], pictures[3:4], W, H)
            + R.frames_of(ctx, hap, [L.FMT_YCOCG], pictures[4:5], W, H))
    # (read with textureCount 1 a Hap Q Alpha frame is its colour texture alone)
    level = level_pictures(ctx, good, 1, W, H, s)
    lw, lh = W >> s, H >> s
    out_size = OUT[s]
    crops = [(x >> s, y >> s, max(w >> s, 1), max(h >> s, 1)) for x, y, w, h in GOOD_CROPS]
    assert all(x + w <= lw and y + h <= lh and within_cap((x, y, w, h), out_size) for x, y, w, h in crops)
    over = (0, 0, RATIO * out_size[0] + 1, out_size[1])
    assert over[2] <= lw
    #          good  good  past the right edge  good  over the cap  good  broken        good
    frames = [good[0], good[1], good[2], good[2], good[3], good[3], good[1][:-3], good[4]]
    source = [0, 1, None, 2, None, 3, None, 4]
    call_crops = [crops[0], crops[1], (lw - 3, 0, 4, 4), crops[2], over, crops[3], crops[1], crops[4]]
    n = len(frames)
    # what the whole-frame call says of the broken frame: its crop reaches the last rows, so this call says it too
    whole = torch.zeros((n, channels, lh, lw), dtype=P.KINDS[kind][0], device="cuda")
    _r, full_res = ctx.decode_frames_planes(frames, [len(f) for f in frames], 1, whole, W, H, scale_log2=s)
    assert full_res[6] not in (0, bad) and [full_res[i] for i in range(n) if i != 6] == [0] * (n - 1), full_res
    expect = [0, 0, bad, 0, bad, 0, full_res[6], 0]
    r, res, targets = resized_frames(ctx, frames, 1, W, H, call_crops, out_size, s, kind, channels)
    assert res == expect and r == bad, res
    for i, t in enumerate(targets):
        if source[i] is None:
            assert t.untouched(), i
        else:
            P.check(t, expected(level[source[i]], call_crops[i], out_size, kind, channels), (s, i))
    # the alpha plane where there are two textures and four planes
    if channels == 4:
        both = level_pictures(ctx, hapq_alpha, 2, W, H, s)
        r, res, targets = resized_frames(ctx, hapq_alpha, 2, W, H, [crops[3]], out_size, s, kind, 4)
        assert r == 0 and res == [0]
        P.check(targets[0], expected(both[0], crops[3], out_size, kind, 4), s)
    # a context between ...Begin and ...Finish
    busy = hap.Context(0)
    try:
        picture = np.ascontiguousarray(D.rgba(W, H, 1))
        buf = np.zeros(hap.HapMaxEncodedLength([R.NB * 16], [L.FMT_DXT5], [1]) + 4096, dtype=np.uint8)
        assert busy.encode_frames_rgba_begin([picture], W, H, W * 4, [L.FMT_DXT5], [1], [1], [buf]) == 0
        keep_alive = (picture, buf)
        r, res, targets = resized_frames(busy, good, 1, W, H, crops, out_size, s, kind, channels)
        internal = hap.HapResult.Internal_Error
        assert r == internal and res == [internal] * len(good) and all(t.untouched() for t in targets)
        busy.encode_finish()
        del keep_alive
    finally:
        busy.close()


# ------------------------------------------------------------------------------------------------------ 4. skipping --
FW, FH = R.FW, R.FH                               # 512 x 32, four chunks: a chunk is two block rows
# the two frames' crops at full size and the rectangle of blocks each rounds outward to: one size, so that one
# decode_frames_planes_region call takes both
SKIP_CROPS = {0: ((1, 1, 250, 6), (257, 25, 251, 7)), 1: ((1, 1, 125, 3), (129, 12, 125, 4)), 2: ((0, 0, 63, 2), (64, 6, 63, 2))}
SKIP_ORIGINS, SKIP_SIZE = ((0, 0), (256, 24)), (252, 8)
SKIP_OUT = (70, 3)


def rounded_outward(crop, s):
    x, y, w, h = crop
    x0, y0 = (x << s) & ~3, (y << s) & ~3
    return x0, y0, ((((x + w) << s) + 3) & ~3) - x0, ((((y + h) << s) + 3) & ~3) - y0


@pytest.mark.parametrize("kind", ("table", "plain"))
def test_what_holds_none_of_a_crops_blocks_stays_undecoded(ctx, hap, kind):
    fmts = [L.FMT_YCOCG]
    made = R.make_frames(ctx, hap, kind, fmts, [R.gradient(FW, FH, 1), D.rgba(FW, FH, 2)], FW, FH, 4)
    # other frames of the same geometry, decoded through the same context in front of every call: what a wrongly skipped
    # piece would leave in the scratch is theirs, not a copy of the right answer
    decoys = R.make_frames(ctx, hap, kind, fmts, [R.gradient(FW, FH, 7), D.rgba(FW, FH, 8)], FW, FH, 4)
    frames = [made[0], R.dev(made[1])]                                   # one frame on the host, one in device memory
    for s in P.SCALES:
        element, channels = KINDS[s], 3
        crops = SKIP_CROPS[s]
        assert [rounded_outward(c, s) for c in crops] == [o + SKIP_SIZE for o in SKIP_ORIGINS]
        level = level_pictures(ctx, frames, 1, FW, FH, s)
        want = [expected(level[i], crops[i], SKIP_OUT, element, channels) for i in (0, 1)]
        for flags in (0, hap.DECODE_IGNORE_FRAGMENT_INDEX):
            level_pictures(ctx, decoys, 1, FW, FH, s)
            before = ctx.skipped_texture_bytes()
            region_out = torch.zeros((2, channels, SKIP_SIZE[1] >> s, SKIP_SIZE[0] >> s), dtype=P.KINDS[element][0], device="cuda")
            r, res = ctx.decode_frames_planes_region(frames, [len(f) for f in frames], 1, region_out, FW, FH, SKIP_ORIGINS,
                                                     SKIP_SIZE, scale_log2=s, flags=flags)
            assert r == 0 and res == [0, 0]
            theirs = ctx.skipped_texture_bytes() - before
            level_pictures(ctx, decoys, 1, FW, FH, s)
            before = ctx.skipped_texture_bytes()
            r, res, targets = resized_frames(ctx, frames, 1, FW, FH, crops, SKIP_OUT, s, element, channels, flags)
            skipped = ctx.skipped_texture_bytes() - before
            note = (kind, s, flags)
            print("%s: skipped %d, the region call %d" % (note, skipped, theirs))
            assert r == 0 and res == [0, 0], (note, res)
            for i in (0, 1):
                P.check(targets[i], want[i], note + (i,))
            assert skipped == theirs and skipped > 0, (note, skipped, theirs)


def test_more_frames_than_one_slice_holds(ctx, hap):
    """A call decodes its frames 32768 textures at a time; the crop arrays are the call's.  32768 + 40 frames of 16 x 8
    texels, cycling through 5 frames of random blocks and 7 crops: 32768 is 1 modulo 7, so a crop looked up by a frame's
    place in its slice is another frame's."""
    w, h, out_size = 16, 8, (4, 2)                                  # (the widest crop is 4 x the output)
    n = 32768 + 40
    rng = np.random.default_rng(4)
    made = [P.hap_encode(hap, [rng.integers(0, 256, 8 * 8, dtype=np.uint8).tobytes()], [L.FMT_DXT1]) for _ in range(5)]
    places = [(0, 0, 16, 8), (1, 1, 3, 2), (5, 0, 11, 7), (15, 7, 1, 1), (2, 3, 12, 5), (0, 6, 7, 2), (9, 1, 6, 6)]
    level = level_pictures(ctx, made, 1, w, h, 0)
    want = np.stack([np.stack([expected(level[i], p, out_size, "f16", 3) for p in places]) for i in range(5)])   # [5, 7, 3, 2, 4]
    assert len({want[i, p].tobytes() for i in range(5) for p in range(7)}) == 35
    step = 256                                                      # the frames in device memory, 256 bytes apart
    assert max(len(f) for f in made) <= step
    store = np.zeros(5 * step, dtype=np.uint8)
    for i, f in enumerate(made):
        store[i * step: i * step + len(f)] = np.frombuffer(f, np.uint8)
    store = torch.from_numpy(store).cuda()
    frames = [store[(f % 5) * step: (f % 5 + 1) * step] for f in range(n)]
    out = torch.zeros((n, 3, out_size[1], out_size[0]), dtype=torch.float16, device="cuda")
    r, res = ctx.decode_frames_planes_resized(frames, [len(made[f % 5]) for f in range(n)], 1, out, w, h,
                                              [places[f % 7] for f in range(n)], out_size, scale=CONSTANTS[0][:3],
                                              bias=CONSTANTS[1][:3])
    assert r == 0 and res == [0] * n
    f = np.arange(n)
    got = out.view(torch.int16).cpu().numpy().view(np.uint16)
    wrong = np.argwhere((got != want[f % 5, f % 7]).reshape(n, -1).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()


# ----------------------------------------------------------------------------------------------- 5. whole-call refusals --
def test_whole_call_refusals_and_the_tensor_rules(ctx, hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    frames = (R.frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 0)], W, H)
              + R.frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3), D.rgba(W, H, 4)], W, H))
    n = len(frames)
    ow, oh = 9, 5
    e, row, plane = 2, ow * 2, ow * oh * 2
    targets = [P.Target("f16", 4, oh, ow) for _ in frames]
    keep = [np.frombuffer(f, dtype=np.uint8) for f in frames]
    ptrs = (C.c_void_p * n)(*[k.ctypes.data for k in keep])
    lens = (C.c_ulong * n)(*[len(f) for f in frames])
    outs = (C.c_void_p * n)(*[t.tensor.data_ptr() for t in targets])
    xs, ys = (C.c_uint * n)(0, 17, 33), (C.c_uint * n)(0, 9, 13)
    ws, hs = (C.c_uint * n)(31, 19, 5), (C.c_uint * n)(7, 20, 11)
    scale, bias = (C.c_float * 4)(*P.DEFAULT[0]), (C.c_float * 4)(*P.DEFAULT[1])

    def call(width=W, height=H, out_w=ow, out_h=oh, s=0, channels=4, element=0, plane_bytes=plane, row_bytes=row, arrays=None):
        a = dict(ptrs=ptrs, lens=lens, outs=outs, scale=scale, bias=bias, xs=xs, ys=ys, ws=ws, hs=hs)
        a.update(arrays or {})
        res = (C.c_uint * n)(*([77] * n))
        r = lib.HapGpuDecodeFramesPlanesResized(ctx.handle, n, a["ptrs"], a["lens"], 1, a["outs"], width, height, s, a["xs"],
                                                a["ys"], a["ws"], a["hs"], out_w, out_h, channels, element, plane_bytes,
                                                row_bytes, a["scale"], a["bias"], res, 0)
        return r, list(res)

    refusals = {
        # what the planes call refuses
        "channels 2": dict(channels=2), "channels 5": dict(channels=5), "element 3": dict(element=3),
        "scaleLog2 3": dict(s=3), "width 6": dict(width=6), "height 30": dict(height=30),
        "rowBytes too short": dict(row_bytes=row - e), "planeBytes too short": dict(plane_bytes=plane - e),
        "rowBytes off the element": dict(row_bytes=row + 1), "planeBytes off the element": dict(plane_bytes=plane + 1),
        "no frames": dict(arrays=dict(ptrs=None)), "no sizes": dict(arrays=dict(lens=None)),
        "no tensors": dict(arrays=dict(outs=None)), "no scale": dict(arrays=dict(scale=None)),
        "no bias": dict(arrays=dict(bias=None)),
        # the crop arrays and the output's size
        "no cropXs": dict(arrays=dict(xs=None)), "no cropYs": dict(arrays=dict(ys=None)),
        "no cropWidths": dict(arrays=dict(ws=None)), "no cropHeights": dict(arrays=dict(hs=None)),
        "outWidth 0": dict(out_w=0), "outHeight 0": dict(out_h=0), "outWidth 16385": dict(out_w=16385, row_bytes=16385 * e,
                                                                                         plane_bytes=16385 * e * oh),
        "outHeight 16385": dict(out_h=16385, plane_bytes=row * 16385),
    }
    for name, arguments in refusals.items():
        assert call(**arguments) == (bad, [bad] * n), name
        assert all(t.untouched() for t in targets), name
    # ... and the same call with nothing wrong; rows and planes an odd number of elements apart are in order
    assert call() == (0, [0] * n)
    assert not any(t.untouched() for t in targets)
    odd = [P.Target("f16", 4, oh, ow, row=ow + 1, plane=(ow + 1) * oh + 1, first=1) for _ in frames]
    assert call(row_bytes=(ow + 1) * e, plane_bytes=((ow + 1) * oh + 1) * e,
                arrays=dict(outs=(C.c_void_p * n)(*[t.tensor.data_ptr() for t in odd]))) == (0, [0] * n)
    # a tensor in host memory and one at an address that is no multiple of the element fail alone
    mine = [P.Target("f16", 4, oh, ow) for _ in frames]
    host = np.full(4 * oh * ow * e, SENTINEL, dtype=np.uint8)
    addresses = [host.ctypes.data, mine[1].tensor.data_ptr() + 1, mine[2].tensor.data_ptr()]
    assert call(arrays=dict(outs=(C.c_void_p * n)(*addresses))) == (bad, [bad, bad, 0])
    assert (host == SENTINEL).all() and mine[0].untouched() and mine[1].untouched() and not mine[2].untouched()
    # one texture: the same rules
    tex = P.random_texture("dxt5", 260, 12)[0][: R.NB * 16]
    one = dict(scale=(C.c_float * 3)(1, 1, 1), bias=(C.c_float * 3)(0, 0, 0))

    def single(crop, out_size, address, s=0, element=0, fmt=L.FMT_DXT5, row_bytes=None, plane_bytes=None):
        ow1, oh1 = out_size
        size = 4 if element == 2 else 2
        return lib.HapGpuDecompressPlanesResized(ctx.handle, tex, len(tex), fmt, None, 0, W, H, s, *crop, ow1, oh1, 3, element,
                                                 address, plane_bytes or ow1 * oh1 * size, row_bytes or ow1 * size,
                                                 one["scale"], one["bias"])

    target = P.Target("f16", 3, 5, 9)
    at = target.tensor.data_ptr()
    refused = {
        "empty": ((0, 0, 0, 4), (9, 5)), "no rows": ((0, 0, 4, 0), (9, 5)), "past the right": ((W - 3, 0, 4, 4), (9, 5)),
        "past the bottom": ((0, H - 3, 4, 4), (9, 5)), "wraps": ((0xFFFFFFFF, 0, 2, 2), (9, 5)),
        "width wraps": ((2, 0, 0xFFFFFFFF, 2), (9, 5)), "over the cap in x": ((0, 0, 37, 4), (9, 5)),
        "over the cap in y": ((0, 0, 4, 21), (9, 5)), "outWidth 0": ((0, 0, 4, 4), (0, 5)), "outHeight 0": ((0, 0, 4, 4), (9, 0)),
    }
    for name, (crop, out_size) in refused.items():
        assert single(crop, out_size, at) == bad and target.untouched(), name
    assert single((0, 0, 4, 4), (16385, 1), at, row_bytes=16385 * 2) == bad and target.untouched()
    assert single((0, 0, 36, 20), (9, 5), at, fmt=L.FMT_BC7) == bad and target.untouched()      # BC7 is no source
    assert single((0, 0, 36, 20), (9, 5), at + 1) == bad and target.untouched()                 # off the element
    assert single((0, 0, 36, 20), (9, 5), at, row_bytes=17) == bad and target.untouched()
    assert single((0, 0, 36, 20), (9, 5), at, row_bytes=16) == bad and target.untouched()
    assert single((0, 0, 36, 20), (9, 5), at, s=1) == bad and target.untouched()                # (32 x 16 at half size)
    host = np.full(3 * 5 * 9 * 2, SENTINEL, dtype=np.uint8)
    assert single((0, 0, 36, 20), (9, 5), host.ctypes.data) == bad and (host == SENTINEL).all()
    assert single((0, 0, 36, 20), (9, 5), at) == 0 and not target.untouched()

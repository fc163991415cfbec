"""A crop per frame of block textures and Hap frames straight to planar float tensors (HapGpuDecompressPlanesRegion,
HapGpuDecodeFramesPlanesRegion), and what the second stage leaves undecoded for it, frame by frame.  The expected value
everywhere is the crop of the tensor the whole-frame call writes (HapGpuDecompressPlanes, HapGpuDecodeFramesPlanes:
tests/test_planes_decode_gpu.py pins that one against numpy and the oracle), rows [y >> s, (y + h) >> s) and columns
[x >> s, (x + w) >> s) of every plane, compared as raw bits; every tensor sits in a sentinel-filled buffer whose other
bytes must stay sentinel."""
import ctypes as C

import numpy as np
import pytest

import _data as D
import _libs as L
import test_planes_decode_gpu as P
import test_region_decode_gpu as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = P.SENTINEL
CONSTANTS = P.CONSTANTS["imagenet"]
ELEMENT = {"f16": 0, "bf16": 1, "f32": 2}                       # HapGpuPlaneElement
COMBOS = ((0, "f16", 3), (1, "bf16", 4), (2, "f32", 4))          # (scaleLog2, element, channels) of the frame tests


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


def bits_of(tensor, kind):
    """The elements' bit patterns, as numpy"""
    wide = torch.int32 if kind == "f32" else torch.int16
    return tensor.contiguous().view(wide).cpu().numpy().view(P.KINDS[kind][1])


def crop(full, origin, size, s):
    """Rows [y >> s, (y + h) >> s) and columns [x >> s, (x + w) >> s) of every plane of [..., H >> s, W >> s]"""
    (x, y), (w, h) = origin, size
    return full[..., y >> s: (y + h) >> s, x >> s: (x + w) >> s]


def padded_target(kind, channels, size, s):
    """A tensor of the rectangle's scaled size inside a larger sentinel-filled one: a first element 4 elements in, rows 4
    elements longer, planes a row longer"""
    ow, oh = size[0] >> s, size[1] >> s
    return P.Target(kind, channels, oh, ow, row=ow + 4, plane=(ow + 4) * (oh + 1), first=4)


def constants_for(channels):
    return CONSTANTS[0][:channels], CONSTANTS[1][:channels]


def whole_frames(ctx, frames, count, w, h, s, kind, channels, flags=0):
    """What decode_frames_planes writes for the frames: bit patterns [n, channels, h >> s, w >> s]"""
    out = torch.zeros((len(frames), channels, h >> s, w >> s), dtype=P.KINDS[kind][0], device="cuda")
    scale, bias = constants_for(channels)
    r, res = ctx.decode_frames_planes(frames, [len(f) for f in frames], count, out, w, h, scale_log2=s, scale=scale,
                                      bias=bias, flags=flags)
    assert r == 0 and res == [0] * len(frames), res
    return bits_of(out, kind)


def region_frames(ctx, frames, count, w, h, origins, size, s, kind, channels, flags=0):
    """decode_frames_planes_region into padded targets: (result, results, targets)"""
    targets = [padded_target(kind, channels, size, s) for _ in frames]
    scale, bias = constants_for(channels)
    r, res = ctx.decode_frames_planes_region(frames, [len(f) for f in frames], count, [t.tensor for t in targets], w, h,
                                             origins, size, scale_log2=s, scale=scale, bias=bias, flags=flags)
    return r, res, targets


# ------------------------------------------------------------------------------ 1. textures, every edge of the rectangle --
@pytest.mark.parametrize("size", ((260, 12), (516, 12)), ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", P.CASES)
def test_random_blocks_at_every_edge_of_the_rectangle(ctx, case, size):
    w, h = size
    tex, plane, _full = P.random_texture(case, w, h)
    dtex, dplane = P.dev(tex), P.dev(plane) if plane else None
    fmt = P.FORMATS[case]
    for s in P.SCALES:
        for kind in sorted(P.KINDS):
            for channels in (3, 4):
                scale, bias = constants_for(channels)
                whole = torch.zeros((channels, h >> s, w >> s), dtype=P.KINDS[kind][0], device="cuda")
                assert ctx.decompress_planes(dtex, fmt, w, h, whole, scale_log2=s, scale=scale, bias=bias, alpha=dplane) == 0
                whole = bits_of(whole, kind)
                for region in R.edge_regions(w, h):
                    want = crop(whole, region[:2], region[2:], s)
                    # (textures on the host once per rectangle, in device memory otherwise)
                    host = kind == "f16" and channels == 4
                    target = padded_target(kind, channels, region[2:], s)
                    r = ctx.decompress_planes_region(tex if host else dtex, fmt, w, h, region, target.tensor, scale_log2=s,
                                                     scale=scale, bias=bias, alpha=plane if host else dplane)
                    assert r == 0, (s, kind, channels, region)
                    P.check(target, want, (s, kind, channels, region))


def test_textures_refuse_what_the_rules_refuse(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    w, h = R.W, R.H
    tex = P.random_texture("dxt5", 260, 12)[0][: R.NB * 16]
    for region in R.REFUSED:
        rw, rh = (region[2] if 0 < region[2] <= w else 4), (region[3] if 0 < region[3] <= h else 4)
        target = P.Target("f16", 3, rh, rw)
        r = hap._lib.lib.HapGpuDecompressPlanesRegion(
            ctx.handle, tex, len(tex), L.FMT_DXT5, None, 0, w, h, *region, 0, 3, 0, target.tensor.data_ptr(), rw * rh * 2,
            rw * 2, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
        assert r == bad and target.untouched(), region
    # the tensor rules, at the rectangle's size: misaligned address, rows and planes; a host tensor
    region = (8, 4, 16, 8)
    for s, kind in ((0, "f16"), (1, "f32"), (2, "bf16")):
        good = padded_target(kind, 4, region[2:], s)
        assert ctx.decompress_planes_region(tex, L.FMT_DXT5, w, h, region, good.tensor, scale_log2=s) == 0
        ow, oh = region[2] >> s, region[3] >> s
        if s < 2:
            for layout in (dict(first=1), dict(row=ow + 1), dict(plane=ow * oh + 1, row=ow)):
                target = P.Target(kind, 4, oh, ow, **layout)
                r = ctx.decompress_planes_region(tex, L.FMT_DXT5, w, h, region, target.tensor, scale_log2=s)
                assert r == bad and target.untouched(), (s, kind, layout)
        host = np.full(4 * oh * ow * 4, SENTINEL, dtype=np.uint8)
        e = good.e
        r = hap._lib.lib.HapGpuDecompressPlanesRegion(ctx.handle, tex, len(tex), L.FMT_DXT5, None, 0, w, h, *region, s, 4,
                                                      ELEMENT[kind],
                                                      host.ctypes.data, ow * oh * e, ow * e, (C.c_float * 4)(1, 1, 1, 1),
                                                      (C.c_float * 4)(0, 0, 0, 0))
        assert r == bad and (host == SENTINEL).all(), (s, kind)
    # BC7 is no source
    bc7 = bytes(R.NB * 16)
    target = P.Target("f16", 3, 8, 16)
    assert ctx.decompress_planes_region(bc7, L.FMT_BC7, w, h, region, target.tensor) == bad and target.untouched()


# ------------------------------------------------------------------------ 2. frames with a different rectangle each --
FW, FH = R.FW, R.FH                               # 512 x 32, four chunks: a chunk is two block rows
FRAME_FORMATS = {k: R.FRAME_FORMATS[k] for k in ("hap", "hap_q", "hap_q_alpha")}
# name -> (origins of the two frames, the rectangles' size): disjoint chunks for the two frames; a left and a right tile
FRAME_ORIGINS = {"bands": (((0, 0), (0, 24)), (512, 8)), "tiles": (((0, 0), (256, 0)), (256, 32)),
                 "inner": (((128, 8), (252, 16)), (256, 16)), "whole": (((0, 0), (0, 0)), (512, 32))}


def layouts_of(hap, frame, fmts, chunks):
    """(block bytes, chunk offsets) of every texture of a frame"""
    out = []
    for t, f in enumerate(fmts):
        r, offsets = hap.HapGpuGetFrameTextureChunkLayout(frame, t)
        assert r == 0 and len(offsets) == chunks + 1, offsets
        out.append((R.BLOCK_BYTES[f], offsets))
    return out


@pytest.mark.parametrize("name", tuple(FRAME_FORMATS))
@pytest.mark.parametrize("kind", ("table", "plain", "reference"))
def test_frames_to_a_rectangle_each_and_what_is_skipped(ctx, hap, kind, name):
    fmts = FRAME_FORMATS[name]
    count = len(fmts)
    made = R.make_frames(ctx, hap, kind, fmts, [R.gradient(FW, FH, 1), R.gradient(FW, FH, 2)], FW, FH, 4)
    # other frames of the same geometry, decoded through the same context in front of every call: what a wrongly skipped
    # piece would leave in the scratch is theirs, not a copy of the right answer
    decoys = R.make_frames(ctx, hap, kind, fmts, [R.gradient(FW, FH, 7), D.rgba(FW, FH, 8)], FW, FH, 4)
    layouts = [layouts_of(hap, frame, fmts, 4) for frame in made]
    for frame in made:
        for t in range(count):
            assert R.chunk_compressors(frame, t) == [0x0B] * 4, (kind, name, t)
    frames = [made[0], R.dev(made[1])]                                   # one frame on the host, one in device memory
    texture_bytes = sum(offsets[-1] for per_frame in layouts for _bb, offsets in per_frame)
    every = (0, hap.DECODE_IGNORE_FRAGMENT_INDEX, hap.DECODE_NO_BLOCK_SCAN,
             hap.DECODE_IGNORE_FRAGMENT_INDEX | hap.DECODE_NO_BLOCK_SCAN)
    for s, element, channels in COMBOS:
        whole = {flags: whole_frames(ctx, frames, count, FW, FH, s, element, channels, flags) for flags in every}
        assert all(np.array_equal(whole[0], whole[flags]) for flags in every)
        for oname, (origins, size) in FRAME_ORIGINS.items():
            regions = [o + size for o in origins]
            want = [crop(whole[0][i], origins[i], size, s) for i in (0, 1)]
            by_chunks = sum(R.pieces_without(hap, FW, bb, regions[i], offsets)
                            for i in (0, 1) for bb, offsets in layouts[i])
            by_fragments = sum(R.pieces_without(hap, FW, bb, regions[i], list(range(0, offsets[-1] + 1, 1024)))
                               for i in (0, 1) for bb, offsets in layouts[i])
            region_bytes = sum((size[0] // 4) * (size[1] // 4) * bb for i in (0, 1) for bb, _o in layouts[i])
            if oname == "bands":
                assert by_chunks > 0                 # three of four chunks of every texture, other ones for each frame
            fallbacks = ctx.table_fallbacks()
            for flags in every:
                whole_frames(ctx, decoys, count, FW, FH, s, element, channels, flags)
                before = ctx.skipped_texture_bytes()
                r, res, targets = region_frames(ctx, frames, count, FW, FH, origins, size, s, element, channels, flags)
                skipped = ctx.skipped_texture_bytes() - before
                note = (s, element, channels, oname, flags)
                print("%s %s %s: skipped %d, chunks %d, fragments %d, most %d" % (kind, name, note, skipped, by_chunks,
                                                                                  by_fragments, texture_bytes - region_bytes))
                assert r == 0 and res == [0, 0], (note, res)
                for i in (0, 1):
                    P.check(targets[i], want[i], note + (i,))
                if oname == "whole":
                    assert skipped == 0 and by_chunks == 0 and by_fragments == 0, note
                assert skipped >= by_chunks, (note, skipped, by_chunks)
                if kind == "table" and not flags & hap.DECODE_IGNORE_FRAGMENT_INDEX:
                    assert skipped >= by_fragments, (note, skipped, by_fragments)
                assert skipped <= texture_bytes - region_bytes, (note, skipped)
            if kind == "table":
                assert ctx.table_fallbacks() == fallbacks, oname


# ----------------------------------------------------------------------------------------- 3. the pieces the scan finds --
SW, SH = R.SW, R.SH                               # 1024 x 256: 256 KiB of YCoCg, a block row 4 KiB
SCAN_ORIGINS = (((0, 192), (512, 0)), (256, 64))  # each frame's tile leaves 192 KiB of its texture in front of or behind it


@pytest.mark.parametrize("kind", ("plain", "reference", "fine_chunks"))
def test_blocks_the_scan_finds_are_skipped_frame_by_frame(ctx, hap, kind):
    pictures = [R.gradient(SW, SH, 5), D.rgba(SW, SH, 6)]
    fmts = [L.FMT_YCOCG]
    decode_flags = 0
    if kind == "fine_chunks":
        made = R.frames_of(ctx, hap, fmts, pictures, SW, SH, flags=hap.ENCODE_FINE_CHUNKS, chunks=1)
        decode_flags = hap.DECODE_GUESS_FIELDS
    else:
        made = R.make_frames(ctx, hap, kind, fmts, pictures, SW, SH, 1)
    frames = [made[0], R.dev(made[1])]
    total = (SW // 4) * (SH // 4) * 16
    origins, size = SCAN_ORIGINS
    s, element, channels = 1, "f16", 3
    whole = whole_frames(ctx, frames, 1, SW, SH, s, element, channels, decode_flags)
    for flags in (decode_flags, decode_flags | hap.DECODE_NO_BLOCK_SCAN):
        whole_frames(ctx, frames[::-1], 1, SW, SH, s, element, channels, flags)     # (the scratch holds the other frame's)
        before = ctx.skipped_texture_bytes()
        r, res, targets = region_frames(ctx, frames, 1, SW, SH, origins, size, s, element, channels, flags)
        skipped = ctx.skipped_texture_bytes() - before
        print("%s flags %#x: skipped %d" % (kind, flags, skipped))
        assert r == 0 and res == [0, 0], (flags, res)
        for i in (0, 1):
            P.check(targets[i], crop(whole[i], origins[i], size, s), (flags, i))
        assert skipped <= 2 * (total - (size[0] // 4) * (size[1] // 4) * 16), (flags, skipped)
        if kind == "fine_chunks" or not flags & hap.DECODE_NO_BLOCK_SCAN:
            # whatever the pieces are -- 8 KiB or 64 KiB blocks of the scan, 8 KiB chunks --: frame 0's first 128 KiB and
            # frame 1's last 128 KiB hold nothing of their tiles and begin and end on a piece's edge
            assert skipped >= 2 * 131072, (flags, skipped)


# ---------------------------------------------------------------------------------------------------------- 4. slicing --
def test_more_frames_than_one_slice_holds(ctx, hap):
    """A call decodes its frames 32768 textures at a time; the rectangle arrays are the call's.  32768 + 40 frames of
    16 x 8 texels, cycling through 5 frames of random blocks and 7 origins: 32768 is 1 modulo 7, so an origin looked up by a frame's
    place in its slice is another frame's, and a wrong crop."""
    w, h, size = 16, 8, (4, 4)
    n = 32768 + 40
    rng = np.random.default_rng(4)                                  # (random blocks: no two crops alike)
    made = [P.hap_encode(hap, [rng.integers(0, 256, 8 * 8, dtype=np.uint8).tobytes()], [L.FMT_DXT1]) for _ in range(5)]
    places = [(x, y) for y in (0, 4) for x in (0, 4, 8, 12)][:7]
    whole = whole_frames(ctx, made, 1, w, h, 0, "f16", 3)
    crops = np.stack([np.stack([crop(whole[i], p, size, 0) for p in places]) for i in range(5)])   # [5, 7, 3, 4, 4]
    assert len({crops[i, p].tobytes() for i in range(5) for p in range(7)}) == 35
    # the frames in device memory, behind each other at 256-byte steps
    step = 256
    assert max(len(f) for f in made) <= step
    store = np.zeros(5 * step, dtype=np.uint8)
    for i, f in enumerate(made):
        store[i * step: i * step + len(f)] = np.frombuffer(f, np.uint8)
    store = torch.from_numpy(store).cuda()
    frames = [store[(f % 5) * step: (f % 5 + 1) * step] for f in range(n)]
    lens = [len(made[f % 5]) for f in range(n)]
    origins = [places[f % 7] for f in range(n)]
    out = torch.zeros((n, 3, 4, 4), dtype=torch.float16, device="cuda")
    r, res = ctx.decode_frames_planes_region(frames, lens, 1, out, w, h, origins, size, scale=CONSTANTS[0][:3],
                                             bias=CONSTANTS[1][:3])
    assert r == 0 and res == [0] * n
    f = np.arange(n)
    got = bits_of(out, "f16")
    want = crops[f % 5, f % 7]
    wrong = np.argwhere((got != want).reshape(n, -1).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()


# ---------------------------------------------------------------------------------------------------- 5. failing alone --
W, H = R.W, R.H                                   # 64 x 32, two chunks


def test_a_bad_frame_fails_alone(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    lib = hap._lib.lib
    size, s, kind, channels = (32, 16), 0, "f16", 3
    good = (R.frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1), D.rgba(W, H, 2)], W, H)
            + R.frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3)], W, H))
    small = R.frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(32, 32, 9)], 32, 32)[0]
    whole = whole_frames(ctx, good, 1, W, H, s, kind, channels)
    #          good     off the grid  past the right  past the bottom  broken         another size  host      misaligned  good      good
    frames = [good[0], good[1], good[2], good[0], good[1][:-3], small, good[2], good[0], good[1], good[2]]
    origins = [(0, 0), (2, 0), (48, 0), (0, 24), (16, 16), (0, 0), (0, 0), (0, 0), (32, 16), (16, 4)]
    source = [0, None, None, None, None, None, None, None, 1, 2]
    n = len(frames)
    # what the whole-frame call says of the broken frame: its rectangle reaches the last rows, so this call says it too
    out = torch.zeros((n, channels, H, W), dtype=torch.float16, device="cuda")
    _r, full_res = ctx.decode_frames_planes(frames, [len(f) for f in frames], 1, out, W, H)
    assert full_res[4] not in (0, bad) and full_res[5] == bad
    expect = [0, bad, bad, bad, full_res[4], bad, bad, bad, 0, 0]
    targets = [P.Target(kind, channels, size[1], size[0]) for _ in frames]
    host = np.full(channels * size[0] * size[1] * 2, SENTINEL, dtype=np.uint8)
    outs = [t.tensor.data_ptr() for t in targets]
    outs[6] = host.ctypes.data
    outs[7] += 2                                                    # (a lane stores 8 bytes a row)
    keep = [np.frombuffer(f, dtype=np.uint8) for f in frames]
    scale, bias = (C.c_float * 3)(*CONSTANTS[0][:3]), (C.c_float * 3)(*CONSTANTS[1][:3])
    res = (C.c_uint * n)(*([77] * n))
    before = ctx.skipped_texture_bytes()
    r = lib.HapGpuDecodeFramesPlanesRegion(ctx.handle, n, (C.c_void_p * n)(*[k.ctypes.data for k in keep]),
                                           (C.c_ulong * n)(*[len(f) for f in frames]), 1, (C.c_void_p * n)(*outs), W, H,
                                           (C.c_uint * n)(*[o[0] for o in origins]), (C.c_uint * n)(*[o[1] for o in origins]),
                                           size[0], size[1], s, channels, 0, size[0] * size[1] * 2, size[0] * 2, scale, bias,
                                           res, 0)
    assert list(res) == expect and r == bad, list(res)
    assert (host == SENTINEL).all()
    for i, t in enumerate(targets):
        if source[i] is None:
            assert t.untouched(), i
        else:
            P.check(t, crop(whole[source[i]], origins[i], size, s), i)
    # frames refused for their origins are not handed to the skip: only what the others leave out is counted, never more
    # than their textures less their rectangles
    skipped = ctx.skipped_texture_bytes() - before
    counted = [i for i in range(n) if i not in (1, 2, 3)]
    assert skipped <= sum(R.NB * 16 - (size[0] // 4) * (size[1] // 4) * 16 for _ in counted), skipped


def test_a_frame_decoded_again_without_its_table_counts_what_it_skips_once(ctx, hap):
    """The region test's frame whose fragment table lies about a fragment, beside a sound copy of it, each with a band of
    its own: the liar is decoded a second time without its table (table_fallbacks() rises by one) with ITS rectangle,
    and counts once.  For both frames the chunks the band does not need and the texture less the band are the same
    figure, so the counter rises by exactly twice that."""
    import test_gpu_parity as G
    w, h = 1024, 256                                                 # 256 KiB YCoCg: 4 chunks of 16 block rows
    tex = D.oracle_bc_encode(D.rgba(w, h, frame=6), L.FMT_YCOCG)
    out = np.zeros(hap.HapMaxEncodedLength([len(tex)], [L.FMT_YCOCG], [4]) + 65536, dtype=np.uint8)
    r, used, res = ctx.encode_frames([[tex]], [L.FMT_YCOCG], [1], [4], [out], flags=hap.ENCODE_FRAGMENT_INDEX)
    assert r == 0 and res == [0]
    frame = out[: used[0]].tobytes()
    r, offsets = hap.HapGpuGetFrameTextureChunkLayout(frame, 0)
    assert r == 0 and offsets == [0, 65536, 131072, 196608, 262144]
    _fs_at, n, gt_at = G._group_table(frame)
    assert n == 4 * 8
    liar = bytearray(frame)
    liar[gt_at: gt_at + G.GT] = bytes(G.GT)                          # the first fragment's group table: all zero
    liar = bytes(liar)
    size = (w, 64)
    s, kind, channels = 1, "f16", 3
    whole = whole_frames(ctx, [frame], 1, w, h, s, kind, channels)[0]
    # (the liar's band is the one its lie is in; the sound frame's the last)
    for frames, origins, noticed in (([liar, frame], [(0, 0), (0, 192)], 1), ([frame, liar], [(0, 64), (0, 192)], 0)):
        by_chunks = sum(R.pieces_without(hap, w, 16, o + size, offsets) for o in origins)
        assert by_chunks == 2 * 196608 == 2 * (len(tex) - (size[0] // 4) * (size[1] // 4) * 16)
        fallbacks, before = ctx.table_fallbacks(), ctx.skipped_texture_bytes()
        r, res, targets = region_frames(ctx, frames, 1, w, h, origins, size, s, kind, channels)
        skipped = ctx.skipped_texture_bytes() - before
        print("origins %s: skipped %d, fallbacks +%d" % (origins, skipped, ctx.table_fallbacks() - fallbacks))
        assert r == 0 and res == [0, 0], res
        for i in (0, 1):
            P.check(targets[i], crop(whole, origins[i], size, s), (origins, i))
        assert skipped == by_chunks, (origins, skipped)
        assert ctx.table_fallbacks() == fallbacks + noticed, origins


# ----------------------------------------------------------------------------------------------- 6. whole-call refusals --
def test_whole_call_refusals(ctx, hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    frames = (R.frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 0)], W, H)
              + R.frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3), D.rgba(W, H, 4)], W, H))
    n = len(frames)
    rw, rh = 32, 16
    e, row, plane = 2, rw * 2, rw * rh * 2                  # half elements at full size: a lane stores 8 bytes a row
    targets = [P.Target("f16", 4, rh, rw) for _ in frames]
    keep = [np.frombuffer(f, dtype=np.uint8) for f in frames]
    ptrs = (C.c_void_p * n)(*[k.ctypes.data for k in keep])
    lens = (C.c_ulong * n)(*[len(f) for f in frames])
    outs = (C.c_void_p * n)(*[t.tensor.data_ptr() for t in targets])
    xs, ys = (C.c_uint * n)(0, 16, 32), (C.c_uint * n)(0, 8, 16)
    scale, bias = (C.c_float * 4)(*P.DEFAULT[0]), (C.c_float * 4)(*P.DEFAULT[1])

    def call(width=W, height=H, w=rw, h=rh, s=0, channels=4, element=0, plane_bytes=plane, row_bytes=row, arrays=None):
        a = dict(ptrs=ptrs, lens=lens, outs=outs, scale=scale, bias=bias, xs=xs, ys=ys)
        a.update(arrays or {})
        res = (C.c_uint * n)(*([77] * n))
        r = lib.HapGpuDecodeFramesPlanesRegion(ctx.handle, n, a["ptrs"], a["lens"], 1, a["outs"], width, height, a["xs"],
                                               a["ys"], w, h, s, channels, element, plane_bytes, row_bytes, a["scale"],
                                               a["bias"], res, 0)
        return r, list(res)

    refusals = {
        # what the planes call refuses
        "channels 2": dict(channels=2), "channels 5": dict(channels=5), "element 3": dict(element=3),
        "scaleLog2 3": dict(s=3), "width 6": dict(width=6),
        "rowBytes too short": dict(row_bytes=row - 8), "planeBytes too short": dict(plane_bytes=plane - 8),
        "rowBytes off the unit": dict(row_bytes=row + e), "planeBytes off the unit": dict(plane_bytes=plane + e),
        "no frames": dict(arrays=dict(ptrs=None)), "no sizes": dict(arrays=dict(lens=None)),
        "no tensors": dict(arrays=dict(outs=None)), "no scale": dict(arrays=dict(scale=None)),
        "no bias": dict(arrays=dict(bias=None)),
        # the rectangle arrays and the rectangles' size
        "no regionXs": dict(arrays=dict(xs=None)), "no regionYs": dict(arrays=dict(ys=None)),
        "regionWidth 0": dict(w=0), "regionHeight 0": dict(h=0), "regionWidth off the grid": dict(w=rw + 2),
        "regionHeight off the grid": dict(h=rh - 2), "regionWidth above the frame's": dict(w=W + 4),
        "regionHeight above the frame's": dict(h=H + 4), "regionWidth wraps": dict(w=0xFFFFFFFC),
        "regionHeight wraps": dict(h=0xFFFFFFFC),
    }
    for name, arguments in refusals.items():
        assert call(**arguments) == (bad, [bad] * n), name
        assert all(t.untouched() for t in targets), name
    # ... and the same call with nothing wrong
    assert call() == (0, [0] * n)
    assert not any(t.untouched() for t in targets)
    # a context between ...Begin and ...Finish
    busy = hap.Context(0)
    try:
        picture = np.ascontiguousarray(D.rgba(W, H, 1))
        buf = np.zeros(hap.HapMaxEncodedLength([R.NB * 16], [L.FMT_DXT5], [1]) + 4096, dtype=np.uint8)
        assert busy.encode_frames_rgba_begin([picture], W, H, W * 4, [L.FMT_DXT5], [1], [1], [buf]) == 0
        keep_alive = (picture, buf)
        mine = [P.Target("f16", 4, rh, rw) for _ in frames]
        res = (C.c_uint * n)(*([77] * n))
        r = lib.HapGpuDecodeFramesPlanesRegion(busy.handle, n, ptrs, lens, 1, (C.c_void_p * n)(*[t.tensor.data_ptr() for t in mine]),
                                               W, H, xs, ys, rw, rh, 0, 4, 0, plane, row, scale, bias, res, 0)
        internal = hap.HapResult.Internal_Error
        assert r == internal and list(res) == [internal] * n and all(t.untouched() for t in mine)
        busy.encode_finish()
        del keep_alive
    finally:
        busy.close()


# ----------------------------------------------------------------------------------- 7. one launch per format present --
@pytest.mark.parametrize("s", P.SCALES)
def test_one_launch_per_format_present_in_the_existing_class(ctx, hap, s):
    frames = (R.frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 0)], W, H)
              + R.frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1), D.rgba(W, H, 2)], W, H)
              + R.frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3), D.rgba(W, H, 4)], W, H))
    frames = [frames[i] for i in (0, 1, 3, 2, 4)]
    n, size = len(frames), (32, 16)
    origins = [(4 * i, 4 * (i % 3)) for i in range(n)]
    out = torch.empty((n, 3, size[1] >> s, size[0] >> s), dtype=torch.float16, device="cuda")
    ctx.set_profiling(True)
    ctx.collect_profile()
    r, res = ctx.decode_frames_planes_region(frames, [len(f) for f in frames], 1, out, W, H, origins, size, scale_log2=s)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert r == 0 and res == [0] * n
    assert prof["block_decode"][0] == 3, prof["block_decode"]
    full = torch.empty((n, 3, H >> s, W >> s), dtype=torch.float16, device="cuda")
    assert ctx.decode_frames_planes(frames, [len(f) for f in frames], 1, full, W, H, scale_log2=s)[0] == 0
    for i in range(n):
        assert np.array_equal(bits_of(out[i], "f16"), crop(bits_of(full[i], "f16"), origins[i], size, s)), i

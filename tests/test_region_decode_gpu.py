"""A block-aligned rectangle of block textures and Hap frames straight to RGBA pictures of the rectangle's size
(HapGpuDecompressRGBARegion, HapGpuDecodeFramesRGBARegion), and what the second stage leaves undecoded for it
(HapGpuSkippedTextureBytes, HapGpuRegionNeedsBytes).  Every expected picture is full[ry:ry+rh, rx:rx+rw] of the full-size
decode -- the CPU checkers' (tests/_data.oracle_bc_decode, tests/_bptc_value_space.decode_bc7_blocks) -- and every
comparison is byte for byte, into sentinel-filled buffers whose remaining bytes must stay sentinel."""
import functools

import numpy as np
import pytest

import _bptc_value_space as V
import _data as D
import _libs as L
from _value_space import picture_of_blocks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha", "bc7")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG, "bc7": L.FMT_BC7}
BLOCK_BYTES = dict(D.BLOCK_BYTES)
BLOCK_BYTES.setdefault(L.FMT_BC7, 16)


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


def full_size(case, tex, plane, w, h):
    """What the CPU checkers make of a texture (and its RGTC1 plane) at full size."""
    if case == "bc7":
        return picture_of_blocks(V.decode_bc7_blocks(np.frombuffer(tex, np.uint8).reshape(-1, 16)), row=w // 4)
    pic = D.oracle_bc_decode(tex, FORMATS[case], w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(plane, L.FMT_RGTC1, w, h)
    return pic


def crop(full, region):
    x, y, w, h = region
    return full[y: y + h, x: x + w]


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def filled(nbytes, where):
    t = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=where)
    torch.cuda.synchronize()
    return t


def rows_of(buf, w, h, stride):
    """(the picture [h, w, 4], everything else of the buffer) of a buffer of rows `stride` apart"""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    body = a[: h * stride].reshape(h, stride)
    rest = np.concatenate([body[:, w * 4:].ravel(), a[h * stride:]])
    return body[:, : w * 4].reshape(h, w, 4), rest


def region_of_texture(ctx, case, tex, plane, w, h, region, where, stride=None, offset=0):
    """decompress_rgba_region into a sentinel-filled picture: (result, picture, the bytes that are not the picture's)"""
    rw, rh = region[2], region[3]
    stride = rw * 4 if stride is None else stride
    buf = filled(offset + rh * max(stride, rw * 4) + 64, where)
    r, _ = ctx.decompress_rgba_region(tex, FORMATS[case], w, h, region, rgba=buf[offset:], alpha=plane, row_bytes=stride)
    if stride < rw * 4:                                     # (a pitch no picture fits in: the whole buffer is "the picture")
        whole = buf.cpu().numpy()
        return r, whole, whole[:0]
    pic, rest = rows_of(buf[offset:], rw, rh, stride)
    return r, pic, np.concatenate([rest, buf[:offset].cpu().numpy()])


# ------------------------------------------------------------------------------- 1. kernel edges, texture -> region --
@functools.lru_cache(maxsize=None)
def random_texture(case, w, h):
    """Seeded random bytes: any 8 / 16 bytes are a block (the recipe of test_scaled_decode_gpu.random_texture: every
    BC7 mode and the reserved one).  (texture, plane | None, full-size picture)"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([CASES.index(case), w, h])
    tex = rng.integers(0, 256, nb * BLOCK_BYTES[FORMATS[case]], dtype=np.uint8)
    if case == "bc7":
        first = tex.reshape(-1, 16)[:, 0]
        mode = np.arange(nb) % 9
        first[:] = np.where(mode == 8, 0, (first & ~((2 << mode) - 1) & 0xFF) | (1 << mode)).astype(np.uint8)
    tex = tex.tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    return tex, plane, full_size(case, tex, plane, w, h)


def edge_regions(w, h):
    regions = [(0, 0, w, h), (0, 0, 4, 4), (w - 4, h - 4, 4, 4), (0, 4, w, 4), (256, 0, 4, 12), (8, 4, w - 12, 8)]
    if w == 516:
        regions.append((4, 0, 260, 12))          # 65 blocks wide: a wave crosses region rows
    return regions


@pytest.mark.parametrize("size", ((260, 12), (516, 12)), ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_random_blocks_at_every_edge_of_the_region(ctx, hap, case, size):
    w, h = size
    tex, plane, full = random_texture(case, w, h)
    dtex, dplane = dev(tex), dev(plane) if plane else None
    bad = hap.HapResult.Bad_Arguments
    for region in edge_regions(w, h):
        want = crop(full, region)
        natural = region[2] * 4
        for where in ("cuda", "cpu"):
            for t, p in ((tex, plane), (dtex, dplane)):
                r, got, rest = region_of_texture(ctx, case, t, p, w, h, region, where)
                assert r == 0, (region, where)
                assert np.array_equal(got, want), (region, where, np.argwhere(got != want)[:4].tolist())
                assert (rest == SENTINEL).all(), (region, where)
            # a pitch 16 bytes longer, and a picture offset by 16 bytes
            for stride, offset in ((natural + 16, 0), (natural + 16, 16), (natural, 16)):
                r, got, rest = region_of_texture(ctx, case, dtex, dplane, w, h, region, where, stride=stride, offset=offset)
                assert r == 0, (region, where, stride, offset)
                assert np.array_equal(got, want), (region, where, stride, offset)
                assert (rest == SENTINEL).all(), (region, where, stride, offset)
            # a pitch that is no multiple of 16, and one shorter than the region
            for stride in (natural + 8, natural - 16):
                r, got, rest = region_of_texture(ctx, case, dtex, dplane, w, h, region, where, stride=stride)
                assert r == bad, (region, where, stride)
                assert (got == SENTINEL).all() and (rest == SENTINEL).all(), (region, where, stride)
        # a device picture offset by 8 bytes
        r, got, rest = region_of_texture(ctx, case, dtex, dplane, w, h, region, "cuda", offset=8)
        assert r == bad and (got == SENTINEL).all() and (rest == SENTINEL).all(), region
    # the picture the method allocates itself
    r, got = ctx.decompress_rgba_region(tex, FORMATS[case], w, h, (8, 4, w - 12, 8), alpha=plane)
    assert r == 0 and np.array_equal(np.frombuffer(got, np.uint8).reshape(8, w - 12, 4), crop(full, (8, 4, w - 12, 8)))


# ------------------------------------------------------------------------------------------- 2. every refused region --
W, H = 64, 32
NB = (W // 4) * (H // 4)
REFUSED = ((W - 4, 0, 8, 4), (0, H - 4, 4, 8), (W, 0, 4, 4), (0, H, 4, 4),            # off by 4 past each edge
           (0, 0, W + 4, 4), (0, 0, 4, H + 4),
           (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 0, 0),                                    # zero width or height
           (2, 0, 4, 4), (0, 0, 6, 4), (0, 2, 4, 4), (0, 0, 4, 6), (1, 1, 3, 3),       # off the block grid
           (0xFFFFFFFC, 0, 8, 4), (8, 0, 0xFFFFFFFC, 4), (0, 0xFFFFFFFC, 4, 8), (0, 8, 4, 0xFFFFFFFC))   # wrapping 2^32


def frames_of(ctx, hap, fmts, pictures, w, h, flags=0, chunks=2):
    """One Hap frame per RGBA picture (textures of `fmts`), made by encode_frames_rgba: list of bytes"""
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    counts = [chunks] * len(fmts)
    bufs = [np.zeros(hap.HapMaxEncodedLength(sizes, fmts, counts) + 65536, dtype=np.uint8) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba([np.ascontiguousarray(p) for p in pictures], w, h, w * 4, fmts, [1] * len(fmts),
                                          counts, bufs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return [b[:u].tobytes() for b, u in zip(bufs, used)]


def test_every_refused_region(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    tex, _plane, _full = random_texture("dxt5", 260, 12)
    tex = tex[: NB * 16]
    frame = frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 3)], W, H)[0]
    for region in REFUSED:
        for where in ("cuda", "cpu"):
            buf = filled(W * H * 4, where)
            assert ctx.decompress_rgba_region(tex, L.FMT_DXT5, W, H, region, rgba=buf, row_bytes=W * 4)[0] == bad, region
            assert (buf.cpu().numpy() == SENTINEL).all(), region
            r, res = ctx.decode_frames_rgba_region([frame, frame, frame], [len(frame)] * 3, 1, [buf, buf, buf], W, H, region,
                                                   row_bytes=W * 4)
            assert r == bad and res == [bad, bad, bad], (region, res)
            assert (buf.cpu().numpy() == SENTINEL).all(), region
    # ... and the same calls with a region that fits
    buf = filled(W * H * 4, "cuda")
    r, res = ctx.decode_frames_rgba_region([frame], [len(frame)], 1, [buf], W, H, (W - 4, H - 4, 4, 4), row_bytes=W * 4)
    assert r == 0 and res == [0]


# -------------------------------------------------------------------------------------------------------- 3. frames --
FW, FH = 512, 32                                  # 128 x 8 blocks: 16 KiB YCoCg, 8 KiB plane or DXT1
FRAME_REGIONS = {"top": (0, 0, 512, 8), "bottom": (0, 24, 512, 8), "left": (0, 0, 256, 32), "tile": (128, 8, 256, 16),
                 "whole": (0, 0, 512, 32)}
FRAME_FORMATS = {"hap": [L.FMT_DXT1], "hap_q": [L.FMT_YCOCG], "hap_q_alpha": [L.FMT_YCOCG, L.FMT_RGTC1], "hap_r": [L.FMT_BC7]}
CASE_OF = {L.FMT_DXT1: "dxt1", L.FMT_DXT5: "dxt5", L.FMT_YCOCG: "ycocg", L.FMT_BC7: "bc7"}


def gradient(w, h, seed):
    """A smooth picture: ramps across the width in steps of 16 texels, one slow step down the height"""
    x = np.arange(w)[None, :] // 16
    y = np.arange(h)[:, None] // 16
    pic = np.empty((h, w, 4), dtype=np.uint8)
    pic[..., 0] = (x * 8 + seed * 3) % 256
    pic[..., 1] = (255 - x * 6 - y * 4) % 256
    pic[..., 2] = (y * 8 + x * 2 + seed) % 256
    pic[..., 3] = (64 + x * 5) % 256
    return pic


def section(frame, at):
    """(header bytes, length, type) of the section at `at` (hap.c: 3-byte length, or 0 and a 4-byte one)"""
    n = frame[at] | (frame[at + 1] << 8) | (frame[at + 2] << 16)
    if n == 0:
        return 8, int.from_bytes(frame[at + 4: at + 8], "little"), frame[at + 3]
    return 4, n, frame[at + 3]


def chunk_compressors(frame, index):
    """The compressor table of texture `index` of a frame: one byte per chunk (0x0B: Snappy)"""
    head, _length, kind = section(frame, 0)
    at = 0
    if kind == 0x0D:
        at = head
        for _ in range(index):
            h, n, _k = section(frame, at)
            at += h + n
    head, _length, kind = section(frame, at)
    assert kind >> 4 == 0xC, hex(kind)                      # a chunked texture
    ihead, ilen, ikind = section(frame, at + head)
    assert ikind == 0x01
    q = at + head + ihead
    end = q + ilen
    while q < end:
        shead, slen, skind = section(frame, q)
        if skind == 0x02:
            return list(frame[q + shead: q + shead + slen])
        q += shead + slen
    raise AssertionError("no compressor table")


def textures_of(ctx, frames, index, cap):
    """What decode_frames yields for every frame: list of (result, texture bytes, format)"""
    outs = [np.zeros(cap, dtype=np.uint8) for _ in frames]
    _r, used, fmts, res = ctx.decode_frames(frames, [len(f) for f in frames], index, outs)
    return [(res[i], outs[i][: used[i]].tobytes(), fmts[i]) for i in range(len(frames))]


def checker_pictures(ctx, frames, texture_count, good, w, h):
    """frame index -> full-size picture: the CPU checkers' decode of the textures decode_frames yields"""
    nb = (w // 4) * (h // 4)
    first = textures_of(ctx, frames, 0, nb * 16)
    second = textures_of(ctx, frames, 1, nb * 8) if texture_count == 2 else None
    out = {}
    for i in good:
        code, tex, fmt = first[i]
        assert code == 0 and len(tex) == nb * BLOCK_BYTES[fmt], i
        plane = None
        if second:
            code, plane, pfmt = second[i]
            assert code == 0 and pfmt == L.FMT_RGTC1 and len(plane) == nb * 8, i
        out[i] = full_size(CASE_OF[fmt], tex, plane, w, h)
    return out


def make_frames(ctx, hap, kind, fmts, pictures, w, h, chunks):
    """Frames of one of the three kinds: (a) "table": this library's, with its fragment table of 1 KiB fragments;
    (b) "plain": this library's, hap.h sections only; (c) "reference": written by the reference encoder (its restatement
    where the reference is not built), as tests/test_gpu_parity.py makes them"""
    bptc = hap.ENCODE_BPTC_BLOCKS if L.FMT_BC7 in fmts else 0
    if kind == "table":
        own = hap.Context(0)
        try:
            assert own.set_fragment_log2(10) == 0
            return frames_of(own, hap, fmts, pictures, w, h, flags=hap.ENCODE_FRAGMENT_INDEX | bptc, chunks=chunks)
        finally:
            own.close()
    if kind == "plain":
        return frames_of(ctx, hap, fmts, pictures, w, h, flags=bptc, chunks=chunks)
    api = L.ref_api() or L.oracle_api()
    out = []
    for p in pictures:
        textures = []
        for f in fmts:
            r, tex = ctx.compress_rgba(np.ascontiguousarray(p), w, h, w * 4, f, flags=bptc if f == L.FMT_BC7 else 0)
            assert r == 0
            textures.append(tex)
        r, frame = api.encode(textures, fmts, [L.COMP_SNAPPY] * len(fmts), [chunks] * len(fmts))
        assert r == 0
        out.append(frame)
    return out


def pieces_without(hap, w, block_bytes, region, offsets):
    """bytes of the pieces [offsets[i], offsets[i + 1]) that hold no byte of the region's blocks"""
    return sum(b - a for a, b in zip(offsets[:-1], offsets[1:])
               if not hap.region_needs_bytes(w, block_bytes, region, a, b - a))


def region_call(ctx, frames, count, w, h, region, where, stride, flags):
    """(result, results, pictures [rh, rw, 4], all the other bytes sentinel?)"""
    rw, rh = region[2], region[3]
    pics = [filled(rh * stride + 32, where) for _ in frames]
    r, res = ctx.decode_frames_rgba_region(frames, [len(f) for f in frames], count, pics, w, h, region, row_bytes=stride,
                                           flags=flags)
    got = [rows_of(p, rw, rh, stride) for p in pics]
    return r, res, [g[0] for g in got], all((g[1] == SENTINEL).all() for g in got)


@pytest.mark.parametrize("name", tuple(FRAME_FORMATS))
@pytest.mark.parametrize("kind", ("table", "plain", "reference"))
def test_frames_to_region_pictures_and_what_is_skipped(ctx, hap, kind, name):
    fmts = FRAME_FORMATS[name]
    count = len(fmts)
    flag = hap.DECODE_BPTC_PICTURES if name == "hap_r" else 0
    made = make_frames(ctx, hap, kind, fmts, [gradient(FW, FH, 1), gradient(FW, FH, 2)], FW, FH, 4)
    sizes = [(FW // 4) * (FH // 4) * BLOCK_BYTES[f] for f in fmts]
    layouts = []
    for frame in made:
        for t in range(count):
            comps = chunk_compressors(frame, t)
            assert comps == [0x0B] * 4, (kind, name, t, comps)            # every chunk Snappy-compressed
            r, offsets = hap.HapGpuGetFrameTextureChunkLayout(frame, t)
            assert r == 0 and len(offsets) == 5 and offsets[-1] == sizes[t], offsets
            layouts.append((BLOCK_BYTES[fmts[t]], offsets))
    frames = [made[0], dev(made[1])]                                      # one frame on the host, one in device memory
    # the full call, and the CPU checkers on its textures
    full = [np.zeros(FW * FH * 4, dtype=np.uint8) for _ in frames]
    r, res = ctx.decode_frames_rgba(frames, [len(f) for f in frames], count, full, FW, FH, flags=flag)
    assert r == 0 and res == [0, 0]
    full = [f.reshape(FH, FW, 4) for f in full]
    checked = checker_pictures(ctx, made, count, (0, 1), FW, FH)
    assert all(np.array_equal(full[i], checked[i]) for i in (0, 1))
    for rname, region in FRAME_REGIONS.items():
        rw, rh = region[2], region[3]
        want = [crop(f, region) for f in full]
        region_bytes = sum((rw // 4) * (rh // 4) * bb for bb, _o in layouts)
        fallbacks = ctx.table_fallbacks()
        for where, stride in (("cuda", rw * 4), ("cpu", rw * 4), ("cpu", rw * 4 + 16)):
            before = ctx.skipped_texture_bytes()
            r, res, got, clean = region_call(ctx, frames, count, FW, FH, region, where, stride, flag)
            skipped = ctx.skipped_texture_bytes() - before
            assert r == 0 and res == [0, 0], (rname, where, res)
            assert clean, (rname, where)
            for i in (0, 1):
                assert np.array_equal(got[i], want[i]), (rname, where, i, np.argwhere(got[i] != want[i])[:4].tolist())
            # what was left undecoded: nothing for the whole frame; at least the chunks that hold none of the region's
            # blocks; with the table at least its 1 KiB fragments; never a byte of the region's blocks
            by_chunks = sum(pieces_without(hap, FW, bb, region, offsets) for bb, offsets in layouts)
            by_fragments = sum(pieces_without(hap, FW, bb, region, list(range(0, offsets[-1] + 1, 1024)))
                               for bb, offsets in layouts)
            if rname == "whole":
                assert skipped == 0 and by_chunks == 0 and by_fragments == 0
            if rname in ("top", "bottom"):
                assert by_chunks > 0
            if rname == "left" and name in ("hap_q", "hap_q_alpha", "hap_r"):
                assert by_fragments > 0 and by_chunks == 0         # a block row of the 16-byte blocks is two fragments
            assert skipped >= by_chunks, (rname, where, skipped, by_chunks)
            if kind == "table":
                assert skipped >= by_fragments, (rname, where, skipped, by_fragments)
            assert skipped <= sum(offsets[-1] for _bb, offsets in layouts) - region_bytes, (rname, where, skipped)
        # the same pictures without the table and without the block scan
        for flags in (hap.DECODE_IGNORE_FRAGMENT_INDEX, hap.DECODE_NO_BLOCK_SCAN,
                      hap.DECODE_IGNORE_FRAGMENT_INDEX | hap.DECODE_NO_BLOCK_SCAN):
            r, res, got, clean = region_call(ctx, frames, count, FW, FH, region, "cuda", rw * 4, flag | flags)
            assert r == 0 and res == [0, 0] and clean, (rname, flags, res)
            assert all(np.array_equal(got[i], want[i]) for i in (0, 1)), (rname, flags)
        if kind == "table":
            assert ctx.table_fallbacks() == fallbacks, rname


# ------------------------------------------------------------------------------- 4. mixed batches and broken frames --
MIXED_REGION = (16, 16, 32, 16)


@pytest.fixture(scope="module")
def batches(ctx, hap):
    """name -> (frames, texture_count, decode flags, indices of the good frames, of the truncated one, of the one of
    another geometry, formats present); the batches of test_scaled_decode_gpu.py, made once"""
    small = [D.rgba(32, 32, 9)]
    out = {}
    one = (frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 0)], W, H)
           + frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1), D.rgba(W, H, 2)], W, H)
           + frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3), D.rgba(W, H, 4)], W, H))
    out["mixed"] = ([one[0], one[1], one[2][:-3], one[3], frames_of(ctx, hap, [L.FMT_DXT5], small, 32, 32)[0], one[4]],
                    1, 0, (0, 1, 3, 5), 2, 4, 3)
    qa = frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 5 + i) for i in range(3)], W, H)
    out["hap_q_alpha"] = ([qa[0], qa[1][:-3], frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], small, 32, 32)[0], qa[2]],
                          2, 0, (0, 3), 1, 2, 1)
    flag = hap.ENCODE_BPTC_BLOCKS
    hr = frames_of(ctx, hap, [L.FMT_BC7], [D.rgba(W, H, 8 + i) for i in range(3)], W, H, flags=flag)
    out["hap_r"] = ([hr[0], frames_of(ctx, hap, [L.FMT_BC7], small, 32, 32, flags=flag)[0], hr[1], hr[2][:-3]],
                    1, hap.DECODE_BPTC_PICTURES, (0, 2), 3, 1, 1)
    return out


@pytest.mark.parametrize("name", ("mixed", "hap_q_alpha", "hap_r"))
def test_mixed_batches_and_broken_frames(ctx, hap, batches, name):
    frames, count, flag, good, cut, other, formats_present = batches[name]
    lens = [len(f) for f in frames]
    n = len(frames)
    bad = hap.HapResult.Bad_Arguments
    region = MIXED_REGION
    rw, rh = region[2], region[3]
    want = {i: crop(p, region) for i, p in checker_pictures(ctx, frames, count, good, W, H).items()}
    # what the full-size call says of the truncated frame: the region reaches the last rows, so the region call says it too
    full = [np.zeros(W * H * 4, dtype=np.uint8) for _ in range(n)]
    _r, full_res = ctx.decode_frames_rgba(frames, lens, count, full, W, H, flags=flag)
    assert full_res[cut] != 0 and [full_res[i] for i in good] == [0] * len(good)
    expect = [0] * n
    expect[cut], expect[other] = full_res[cut], bad
    for where, stride in (("cuda", rw * 4), ("cpu", rw * 4), ("cuda", rw * 4 + 16), ("cpu", rw * 4 + 16)):
        pics = [filled(rh * stride + 32, where) for _ in range(n)]
        r, res = ctx.decode_frames_rgba_region(frames, lens, count, pics, W, H, region, row_bytes=stride, flags=flag)
        assert res == expect and r == next(c for c in res if c), (where, res)
        for i in range(n):
            got, rest = rows_of(pics[i], rw, rh, stride)
            assert (rest == SENTINEL).all(), (where, i)
            if i in want:
                assert np.array_equal(got, want[i]), (where, i, np.argwhere(got != want[i])[:4].tolist())
                assert np.array_equal(got, crop(full[i].reshape(H, W, 4), region)), (where, i)
            else:
                assert (got == SENTINEL).all(), (where, i)
    # one block-decode launch per format present, in the existing class
    pics = [filled(rh * rw * 4, "cuda") for _ in range(n)]
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.decode_frames_rgba_region(frames, lens, count, pics, W, H, region, flags=flag)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == formats_present, prof["block_decode"]
    if flag:
        # Hap R frames without the flag: Bad_Arguments frame by frame, pictures untouched
        pics = [filled(rh * rw * 4, "cuda") for _ in range(n)]
        r, res = ctx.decode_frames_rgba_region(frames, lens, count, pics, W, H, region)
        assert r != 0 and [res[i] for i in good] == [bad] * len(good) and res[other] == bad and res[cut] == full_res[cut]
        assert all((p.cpu().numpy() == SENTINEL).all() for p in pics)


# -------------------------------------------- 5. streams without a table that are long enough for the block scan --
SW, SH = 1024, 256                                # 256 x 64 blocks of YCoCg: 256 KiB, a block row 4 KiB
SCAN_REGIONS = {"bottom": (0, 192, 1024, 64), "top_left": (0, 0, 512, 16), "tile": (256, 64, 256, 128)}


@pytest.mark.parametrize("kind", ("plain", "reference", "fine_chunks"))
def test_blocks_the_scan_finds_are_skipped_too(ctx, hap, kind):
    """One chunk of 256 KiB per frame: this library's plain stream (the scan cuts it into 8 KiB pieces), the reference
    encoder's (four 64 KiB blocks), and fine chunks whose group tables the decoder guesses (a unit per 8 KiB chunk)."""
    pictures = [gradient(SW, SH, 5), D.rgba(SW, SH, 6)]
    fmts = [L.FMT_YCOCG]
    decode_flags = 0
    if kind == "fine_chunks":
        made = frames_of(ctx, hap, fmts, pictures, SW, SH, flags=hap.ENCODE_FINE_CHUNKS, chunks=1)
        decode_flags = hap.DECODE_GUESS_FIELDS
    else:
        made = make_frames(ctx, hap, kind, fmts, pictures, SW, SH, 1)
    frames = [made[0], dev(made[1])]
    total = (SW // 4) * (SH // 4) * 16
    full = [np.zeros(SW * SH * 4, dtype=np.uint8) for _ in frames]
    r, res = ctx.decode_frames_rgba(frames, [len(f) for f in frames], 1, full, SW, SH, flags=decode_flags)
    assert r == 0 and res == [0, 0]
    full = [f.reshape(SH, SW, 4) for f in full]
    checked = checker_pictures(ctx, made, 1, (0, 1), SW, SH)
    assert all(np.array_equal(full[i], checked[i]) for i in (0, 1))
    for rname, region in SCAN_REGIONS.items():
        rw, rh = region[2], region[3]
        want = [crop(f, region) for f in full]
        for flags in (decode_flags, decode_flags | hap.DECODE_NO_BLOCK_SCAN):
            before = ctx.skipped_texture_bytes()
            r, res, got, clean = region_call(ctx, frames, 1, SW, SH, region, "cuda", rw * 4, flags)
            skipped = ctx.skipped_texture_bytes() - before
            assert r == 0 and res == [0, 0] and clean, (rname, flags, res)
            for i in (0, 1):
                assert np.array_equal(got[i], want[i]), (rname, flags, i, np.argwhere(got[i] != want[i])[:4].tolist())
            assert skipped <= 2 * (total - (rw // 4) * (rh // 4) * 16), (rname, flags, skipped)
            if rname == "bottom" and (kind == "fine_chunks" or not flags & hap.DECODE_NO_BLOCK_SCAN):
                # whatever the pieces are -- 8 KiB or 64 KiB blocks of the scan, 8 KiB chunks, 64 KiB pieces of a chunk
                # stored raw --: the first 128 KiB of each texture hold nothing of the band and end on a piece's edge
                assert skipped >= 2 * 131072, (rname, flags, skipped)


# ------------------------------------------------------------------- a frame that is decoded a second time counts once --
def test_a_frame_decoded_again_without_its_table_counts_what_it_skips_once(ctx, hap):
    """A frame whose fragment table lies about a needed fragment is decoded a second time without the table
    (table_fallbacks() rises), and the second pass skips whole chunks again.  HapGpuSkippedTextureBytes counts that frame
    once: here the lower bound (the chunks the rectangle does not need) and the upper bound (the texture minus the
    rectangle's blocks) are the same figure, so the rise is exactly that.  The same lie inside a skipped fragment is
    not seen by the picture: it is the crop either way."""
    import test_gpu_parity as P
    w, h = 1024, 256                                                 # 256 KiB YCoCg: 4 chunks of 16 block rows
    tex = D.oracle_bc_encode(D.rgba(w, h, frame=6), L.FMT_YCOCG)
    out = np.zeros(hap.HapMaxEncodedLength([len(tex)], [L.FMT_YCOCG], [4]) + 65536, dtype=np.uint8)
    r, used, res = ctx.encode_frames([[tex]], [L.FMT_YCOCG], [1], [4], [out], flags=hap.ENCODE_FRAGMENT_INDEX)
    assert r == 0 and res == [0]
    frame = out[: used[0]].tobytes()
    r, offsets = hap.HapGpuGetFrameTextureChunkLayout(frame, 0)
    assert r == 0 and offsets == [0, 65536, 131072, 196608, 262144]
    _fs_at, n, gt_at = P._group_table(frame)
    assert n == 4 * 8
    bad = bytearray(frame)
    bad[gt_at: gt_at + P.GT] = bytes(P.GT)                           # the first fragment's group table: all zero
    bad = bytes(bad)
    full = full_size("ycocg", tex, None, w, h)
    for region, noticed in (((0, 0, w, 64), True), ((0, 192, w, 64), None)):
        by_chunks = pieces_without(hap, w, 16, region, offsets)
        assert by_chunks == 196608 == len(tex) - (region[2] // 4) * (region[3] // 4) * 16
        for where in ("cpu", "cuda"):
            fallbacks, before = ctx.table_fallbacks(), ctx.skipped_texture_bytes()
            r, res, got, clean = region_call(ctx, [bad], 1, w, h, region, where, region[2] * 4, 0)
            assert r == 0 and res == [0] and clean, (region, where, res)
            assert np.array_equal(got[0], crop(full, region)), (region, where)
            skipped = ctx.skipped_texture_bytes() - before
            print(f"region {region} {where}: skipped {skipped}, fallbacks +{ctx.table_fallbacks() - fallbacks}")
            assert skipped == by_chunks, (region, where, skipped)
            if noticed:
                assert ctx.table_fallbacks() == fallbacks + 1, (region, where)

"""Half- and quarter-size RGBA pictures straight from block textures and Hap frames (HapGpuDecompressRGBAScaled,
HapGpuDecodeFramesRGBAScaled): every output texel is, per channel, (sum of the 2^s x 2^s full-size texels +
(1 << (2s - 1))) >> 2s.  Every expected picture is the CPU checkers' full-size decode (tests/_data.oracle_bc_decode for
DXT1 / DXT5 / YCoCg / RGTC1, tests/_bptc_value_space.decode_bc7_blocks for BC7) box-filtered with numpy; every
comparison is byte for byte."""
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
SCALES = (1, 2)
CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha", "bc7")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG, "bc7": L.FMT_BC7}
# one lane; the smallest two-lane grids; exactly 64 blocks a row; 65 a row (a wave crosses a block row, 195 blocks: less
# than a workgroup); 387 blocks (a partly filled second workgroup)
GEOMETRIES = ((4, 4), (8, 4), (4, 8), (256, 8), (260, 12), (516, 12))


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
    """The definition: [h, w, c] uint8 -> [h >> s, w >> s, c], halves rounded up."""
    k = 1 << s
    h, w, c = img.shape
    sums = img.astype(np.uint32).reshape(h // k, k, w // k, k, c).sum(axis=(1, 3))
    return ((sums + (1 << (2 * s - 1))) >> (2 * s)).astype(np.uint8)


def full_size(case, tex, plane, w, h):
    """What the CPU checkers make of a texture (and its RGTC1 plane) at full size."""
    if case == "bc7":
        return picture_of_blocks(V.decode_bc7_blocks(np.frombuffer(tex, np.uint8).reshape(-1, 16)), row=w // 4)
    pic = D.oracle_bc_decode(tex, FORMATS[case], w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(plane, L.FMT_RGTC1, w, h)
    return pic


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


def scaled(ctx, case, tex, plane, w, h, s, where, stride=None, offset=0):
    """decompress_rgba_scaled into a sentinel-filled picture: (result, picture, the bytes that are not the picture's)"""
    ow, oh = w >> s, h >> s
    stride = stride or ow * 4
    buf = filled(offset + oh * stride + 64, where)
    r, _ = ctx.decompress_rgba_scaled(tex, FORMATS[case], w, h, s, rgba=buf[offset:], alpha=plane, row_bytes=stride)
    if stride < ow * 4:                                     # (a pitch no picture fits in: the whole buffer is "the picture")
        whole = buf.cpu().numpy()
        return r, whole, whole[:0]
    pic, rest = rows_of(buf[offset:], ow, oh, stride)
    return r, pic, np.concatenate([rest, buf[:offset].cpu().numpy()])


# ------------------------------------------------------------------ 1. every block pattern, every edge of the grid --
@functools.lru_cache(maxsize=None)
def random_texture(case, w, h):
    """Seeded random bytes: any 8 / 16 bytes are a block.  (texture, plane | None, full-size picture)"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([CASES.index(case), w, h])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8)
    if case == "bc7":
        # (a random first byte hardly ever names mode 7 or no mode at all: block i takes mode i mod 9, 8 = reserved)
        first = tex.reshape(-1, 16)[:, 0]
        mode = np.arange(nb) % 9
        first[:] = np.where(mode == 8, 0, (first & ~((2 << mode) - 1) & 0xFF) | (1 << mode)).astype(np.uint8)
    tex = tex.tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    return tex, plane, full_size(case, tex, plane, w, h)


def test_the_random_blocks_reach_what_they_are_meant_to():
    tex = np.frombuffer(random_texture("dxt1", 516, 12)[0], np.uint8).view("<u2").reshape(-1, 4)
    assert (tex[:, 0] <= tex[:, 1]).any() and (tex[:, 0] > tex[:, 1]).any()          # three- and four-colour DXT1
    tex = np.frombuffer(random_texture("dxt5", 516, 12)[0], np.uint8).reshape(-1, 16)
    assert (tex[:, 0] <= tex[:, 1]).any() and (tex[:, 0] > tex[:, 1]).any()          # both alpha ramp orders
    tex = np.frombuffer(random_texture("bc7", 516, 12)[0], np.uint8).reshape(-1, 16)
    modes = {int(b & -b).bit_length() - 1 if b else 8 for b in tex[:, 0].tolist()}
    assert modes == set(range(9))                                                    # all modes and the reserved one
    tex, _plane, pic = random_texture("ycocg", 516, 12)
    scales = {int(b) & 31 for b in np.frombuffer(tex, np.uint8).reshape(-1, 16)[:, 8].tolist()}   # blue of colour 0
    assert len(scales) == 32 and (pic[..., :3] == 0).any() and (pic[..., :3] == 255).any()         # ... and clamping


@pytest.mark.parametrize("size", GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_random_blocks_at_every_edge_of_the_grid(ctx, case, size):
    w, h = size
    tex, plane, full = random_texture(case, w, h)
    dtex, dplane = dev(tex), dev(plane) if plane else None
    for s in SCALES:
        want = box(full, s)
        for where in ("cuda", "cpu"):
            for t, p in ((tex, plane), (dtex, dplane)):
                r, got, rest = scaled(ctx, case, t, p, w, h, s, where)
                assert r == 0, (s, where)
                assert np.array_equal(got, want), (s, where, np.argwhere(got != want)[:4].tolist())
                assert (rest == SENTINEL).all(), (s, where)
    # the picture the method allocates itself
    r, got = ctx.decompress_rgba_scaled(tex, FORMATS[case], w, h, 1, alpha=plane)
    assert r == 0 and np.array_equal(np.frombuffer(got, np.uint8).reshape(h // 2, w // 2, 4), box(full, 1))


# ------------------------------------------------------------------------------------------ 2. rounding and range --
def alpha_block(base, texels_up):
    """An alpha-style block (DXT5 alpha, Hap Q luma, an RGTC1 plane) with endpoints base + 1 and base: code 0 gives
    base + 1, code 1 and every interpolated code base -- texels_up[i] picks code 0 for texel i."""
    codes = 0
    for i, up in enumerate(texels_up):
        codes |= (0 if up else 1) << (3 * i)
    return bytes([base + 1, base]) + codes.to_bytes(6, "little")


def dxt_colour_block(indices):
    """A DXT1 colour block with red endpoints expand5(1) = 8 and 0: entries 8, 0, 5, 2 of red, green and blue 0."""
    word = 0
    for i, k in enumerate(indices):
        word |= k << (2 * i)
    return (1 << 11).to_bytes(2, "little") + bytes(2) + word.to_bytes(4, "little")


def region_of(i, s):
    r, c = divmod(i, 4)
    return 0 if s == 2 else 2 * (r // 2) + c // 2


def residues(s):
    half = 1 << (2 * s - 1)
    return half - 1, half, half + 1


def single_texel_blocks(s):
    """Per region, `half - 1`, `half` and `half + 1` texels one above the rest (the three taken in turn by the regions
    of a block, every block starting one further), at bases 0, 200 and 254."""
    out = []
    for base in (0, 200, 254):
        for turn in range(3):
            filled_so_far = {}
            ups = []
            for i in range(16):
                q = region_of(i, s)
                n = residues(s)[(q + turn) % 3]
                ups.append(filled_so_far.get(q, 0) < n)
                filled_so_far[q] = filled_so_far.get(q, 0) + 1
            # (not the first texels of a region only: the last ones in the next block)
            out.append(alpha_block(base, ups))
            out.append(alpha_block(base, ups[::-1]))
    return out


def colour_blocks(s):
    """DXT1 blocks whose regions' red sums are half - 1, half and half + 1 modulo 4^s, from the entries 8, 0, 5, 2."""
    texels = 1 << (2 * s)
    values = (8, 0, 5, 2)
    found = {}
    for n in np.ndindex(*(texels + 1,) * 3):
        if sum(n) <= texels:
            counts = n + (texels - sum(n),)
            total = sum(c * v for c, v in zip(counts, values))
            found.setdefault(total % texels, []).append(counts)
    out = []
    for turn in range(3):
        for pick in range(4):
            fill = {}
            idx = []
            for i in range(16):
                q = region_of(i, s)
                options = found[residues(s)[(q + turn) % 3]]
                counts = options[(pick * 7 + q) % len(options)]
                order = [k for k in range(4) for _ in range(counts[k])]
                idx.append(order[fill.get(q, 0)])
                fill[q] = fill.get(q, 0) + 1
            out.append(dxt_colour_block(idx))
    return out


HAPQ_GREY = ((16 << 11) | (32 << 5) | 31).to_bytes(2, "little") * 2 + bytes(4)      # Co, Cg -> 0 at scale 32: R = G = B = Y
BC7_WHITE = ((1 << 6) | (((1 << 58) - 1) << 7)).to_bytes(16, "little")              # mode 6, every endpoint and p-bit set
BC7_BLACK = (1 << 6).to_bytes(16, "little")
FF8 = b"\xff\xff" + bytes(6)


@functools.lru_cache(maxsize=None)
def rounding_textures(s):
    """case -> (texture, plane | None, width, full-size picture) of one row of hand-made blocks"""
    ramps, colours = single_texel_blocks(s), colour_blocks(s)
    white = {"dxt1": b"\xff" * 4 + bytes(4), "dxt5": FF8 + b"\xff" * 4 + bytes(4), "ycocg": FF8 + HAPQ_GREY, "bc7": BC7_WHITE}
    sets = {
        "dxt1": colours + [white["dxt1"], bytes(8)],
        "dxt5": [ramps[i % len(ramps)] + colours[i % len(colours)] for i in range(max(len(ramps), len(colours)))]
                + [white["dxt5"], bytes(16)],
        "ycocg": [r + HAPQ_GREY for r in ramps] + [white["ycocg"], bytes(8) + HAPQ_GREY],
        "bc7": [BC7_BLACK, BC7_WHITE, bytes(16)],
    }
    sets["ycocg_alpha"] = sets["ycocg"]
    out = {}
    for case, blocks in sets.items():
        plane = None
        if case == "ycocg_alpha":
            plane = b"".join(ramps[::-1]) + FF8 + bytes(8)
        tex = b"".join(blocks)
        w = 4 * len(blocks)
        out[case] = (tex, plane, w, full_size(case, tex, plane, w, 4))
    return out


@pytest.mark.parametrize("s", SCALES)
def test_the_hand_made_blocks_are_what_they_claim(s):
    texels, (below, half, above) = 1 << (2 * s), residues(s)
    sets = rounding_textures(s)

    def sums(pic, channel):
        k = 1 << s
        return pic[..., channel].astype(int).reshape(4 // k, k, -1, k).sum(axis=(1, 3)).ravel()

    for case, channel in (("dxt1", 0), ("dxt5", 0), ("dxt5", 3), ("ycocg", 0), ("ycocg", 1), ("ycocg", 2), ("ycocg_alpha", 3)):
        seen = set((sums(sets[case][3], channel) % texels).tolist())
        assert {below, half, above} <= seen, (case, channel, seen)
    # single texels: sums of 4^s * base + n at bases 0, 200 and 254
    alpha = sums(sets["dxt5"][3], 3)
    for base in (0, 200, 254):
        assert {texels * base + n for n in (below, half, above)} <= set(alpha.tolist()), base
    for case, (_tex, _plane, w, pic) in sets.items():
        last = pic[:, w - 8: w - 4]                         # the all-255 block: no accumulator may wrap at 4^s * 255
        assert (last == 255).all(), case
        zero = pic[:, w - 4:]
        assert (zero[..., :3] == 0).all() and (zero[..., 3] == (255 if case in ("dxt1", "ycocg") else 0)).all(), case
    assert (sets["bc7"][3][:, :4] == 0).all()                # mode 6 with every endpoint 0, beside the reserved block


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("case", CASES)
def test_ties_round_up_and_nothing_wraps(ctx, case, s):
    tex, plane, w, full = rounding_textures(s)[case]
    want = box(full, s)
    assert (want[:, (w - 8) >> s: (w - 4) >> s] == 255).all()
    for where in ("cuda", "cpu"):
        r, got, rest = scaled(ctx, case, tex, plane, w, 4, s, where)
        assert r == 0
        assert np.array_equal(got, want), (where, np.argwhere(got != want)[:4].tolist())
        assert (rest == SENTINEL).all()


# ------------------------------------------------------------------------------------------ 3. pitch and neighbours --
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("case", ("dxt1", "ycocg_alpha", "bc7"))
def test_longer_rows_and_the_alignment_rule(ctx, hap, case, s):
    w, h = 260, 12
    tex, plane, full = random_texture(case, w, h)
    want = box(full, s)
    unit = 16 >> s                                          # what a lane stores per output row
    natural = (w >> s) * 4
    bad = hap.HapResult.Bad_Arguments
    for where in ("cuda", "cpu"):
        # longer rows, and (device) a picture that is aligned to the unit and to nothing larger
        for stride, offset in ((natural + unit, 0), (natural + 3 * unit, unit)):
            r, got, rest = scaled(ctx, case, tex, plane, w, h, s, where, stride=stride, offset=offset)
            assert r == 0, (where, stride, offset)
            assert np.array_equal(got, want), (where, stride, offset)
            assert (rest == SENTINEL).all(), (where, stride, offset)
        # a pitch off the unit, and one shorter than the picture's row
        for stride in (natural + unit // 2, natural - unit):
            r, got, rest = scaled(ctx, case, tex, plane, w, h, s, where, stride=stride)
            assert r == bad, (where, stride)
            assert (got == SENTINEL).all() and (rest == SENTINEL).all(), (where, stride)
    # a device picture off the unit
    r, got, rest = scaled(ctx, case, tex, plane, w, h, s, "cuda", offset=unit // 2)
    assert r == bad and (got == SENTINEL).all() and (rest == SENTINEL).all()


@pytest.mark.parametrize("s", (0, 3))
def test_other_scales_are_refused(ctx, hap, s):
    w, h = 64, 32
    bad = hap.HapResult.Bad_Arguments
    tex, _plane, _full = random_texture("dxt5", 8, 4)
    tex = tex * ((w // 8) * (h // 4))
    frame = frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(w, h, 3)], w, h)[0]
    for where in ("cuda", "cpu"):
        buf = filled(w * h * 4, where)
        assert ctx.decompress_rgba_scaled(tex, L.FMT_DXT5, w, h, s, rgba=buf)[0] == bad
        assert (buf.cpu().numpy() == SENTINEL).all()
        r, res = ctx.decode_frames_rgba_scaled([frame, frame], [len(frame)] * 2, 1, [buf, buf], w, h, s)
        assert r == bad and res == [bad, bad]
        assert (buf.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- 4. frames, mixed --
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


def textures_of(ctx, frames, index, cap):
    """What decode_frames yields for every frame: list of (result, texture bytes, format)"""
    outs = [np.zeros(cap, dtype=np.uint8) for _ in frames]
    _r, used, fmts, res = ctx.decode_frames(frames, [len(f) for f in frames], index, outs)
    return [(res[i], outs[i][: used[i]].tobytes(), fmts[i]) for i in range(len(frames))]


@pytest.fixture(scope="module")
def batches(ctx, hap):
    """name -> (frames, texture_count, decode flags, indices of the good frames, of the truncated one, of the one of
    another geometry); made once"""
    small = [D.rgba(32, 32, 9)]
    out = {}
    one = (frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 0)], W, H)
           + frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1), D.rgba(W, H, 2)], W, H)
           + frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3), D.rgba(W, H, 4)], W, H))
    out["mixed"] = ([one[0], one[1], one[2][:-3], one[3], frames_of(ctx, hap, [L.FMT_DXT5], small, 32, 32)[0], one[4]],
                    1, 0, (0, 1, 3, 5), 2, 4)
    qa = frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 5 + i) for i in range(3)], W, H)
    out["hap_q_alpha"] = ([qa[0], qa[1][:-3], frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], small, 32, 32)[0], qa[2]],
                          2, 0, (0, 3), 1, 2)
    flag = hap.ENCODE_BPTC_BLOCKS
    hr = frames_of(ctx, hap, [L.FMT_BC7], [D.rgba(W, H, 8 + i) for i in range(3)], W, H, flags=flag)
    out["hap_r"] = ([hr[0], frames_of(ctx, hap, [L.FMT_BC7], small, 32, 32, flags=flag)[0], hr[1], hr[2][:-3]],
                    1, hap.DECODE_BPTC_PICTURES, (0, 2), 3, 1)
    return out


def oracle_pictures(ctx, frames, texture_count, good):
    """frame index -> full-size picture, from the textures decode_frames yields"""
    first = textures_of(ctx, frames, 0, NB * 16)
    second = textures_of(ctx, frames, 1, NB * 8) if texture_count == 2 else None
    out = {}
    for i in good:
        code, tex, fmt = first[i]
        assert code == 0 and len(tex) == NB * D.BLOCK_BYTES[fmt], i
        case = {v: k for k, v in FORMATS.items() if k != "ycocg_alpha"}[fmt]
        plane = None
        if second:
            code, plane, pfmt = second[i]
            assert code == 0 and pfmt == L.FMT_RGTC1 and len(plane) == NB * 8, i
        out[i] = full_size(case, tex, plane, W, H)
    return out


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ("mixed", "hap_q_alpha", "hap_r"))
def test_frames_to_scaled_pictures(ctx, hap, batches, name, s):
    frames, count, flag, good, cut, other = batches[name]
    lens = [len(f) for f in frames]
    n = len(frames)
    bad = hap.HapResult.Bad_Arguments
    want = {i: box(p, s) for i, p in oracle_pictures(ctx, frames, count, good).items()}
    if name == "mixed":
        assert len({textures_of(ctx, frames, 0, NB * 16)[i][2] for i in good}) == 3         # DXT1, DXT5 and YCoCg
    # what the full-size call says of the truncated frame
    full = [np.zeros(W * H * 4, dtype=np.uint8) for _ in range(n)]
    _r, full_res = ctx.decode_frames_rgba(frames, lens, count, full, W, H, flags=flag)
    assert full_res[cut] != 0 and [full_res[i] for i in good] == [0] * len(good)
    expect = [0] * n
    expect[cut], expect[other] = full_res[cut], bad
    ow, oh = W >> s, H >> s
    for where, stride in (("cuda", ow * 4), ("cpu", ow * 4), ("cuda", ow * 4 + 16), ("cpu", ow * 4 + 16)):
        pics = [filled(oh * stride + 32, where) for _ in range(n)]
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, count, pics, W, H, s, row_bytes=stride, flags=flag)
        assert res == expect and r == next(c for c in res if c), (where, res)
        for i in range(n):
            got, rest = rows_of(pics[i], ow, oh, stride)
            assert (rest == SENTINEL).all(), (where, i)
            if i in want:
                assert np.array_equal(got, want[i]), (where, i, np.argwhere(got != want[i])[:4].tolist())
            else:
                assert (got == SENTINEL).all(), (where, i)
        # 5. the same as the long way round: the box mean of what decode_frames_rgba writes at full size
        for i in good:
            assert np.array_equal(rows_of(pics[i], ow, oh, stride)[0], box(full[i].reshape(H, W, 4), s)), (where, i)
    if flag:
        # Hap R frames without the flag: Bad_Arguments frame by frame, pictures untouched
        pics = [filled(oh * ow * 4, "cuda") for _ in range(n)]
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, count, pics, W, H, s)
        assert r != 0 and [res[i] for i in good] == [bad] * len(good) and res[other] == bad and res[cut] == full_res[cut]
        assert all((p.cpu().numpy() == SENTINEL).all() for p in pics)


@pytest.mark.parametrize("s", SCALES)
def test_one_launch_per_format_present_in_the_existing_class(ctx, batches, s):
    frames, count, flag, _good, _cut, _other = batches["mixed"]
    pics = [filled((W >> s) * (H >> s) * 4, "cuda") for _ in frames]
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.decode_frames_rgba_scaled(frames, [len(f) for f in frames], count, pics, W, H, s, flags=flag)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 3, prof["block_decode"]

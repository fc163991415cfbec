"""Deterministic sweeps over the whole input space of the DXT1 / DXT5 / RGTC1 / scaled YCoCg-DXT5 block kernels.

The block kernels replace the oracle's exact divisions by reciprocal multiplies that are right only inside a value
range (bc_decode.hip: /7, /5, /3 and the Hap Q chroma divide; bc_encode_core.hpp: floor(2^19 / d), floor(3 * 2^24 /
len2), the scale thresholds).  Random blocks reach a few per cent of those ranges; these generators reach all of them:

  ramp_blocks()          8-byte alpha blocks: every (a0, a1) pair, all eight codes in every block, every code at
                         every texel position across the sweep
  colour_blocks()        5:6:5 colour blocks: every ordered endpoint pair of each channel, green and blue pairs in
                         both the c0 > c1 and the c0 <= c1 order, c0 == c1 for every 16-bit colour, all four indices
  hapq_colour_blocks()   scaled YCoCg colour halves: every (Co byte, scale) and (Cg byte, scale) that a 5:6:5 palette
                         can hold, in each of the four palette slots (scale 1..32 through the interpolated blue entries)
  *_scaled_sweep()       the endpoints of the above with seeded random codes and every fourth block flat, for the
                         half- and quarter-size decoders: every residue of the region sums, not the even ones only
  ramp_picture()         every lo < hi ramp, the blocks of a pair holding every value lo..hi (every d and u of the
                         alpha encoder), in A and in R = G = B
  all_colours_picture()  every 24-bit RGB colour once
  two_colour_picture()   a block per len2 the encoder's endpoint rule allows: two box corners fix the endpoints, the
                         other texels project where floor(3 * 2^24 / len2) off by one would change an index
  scale_edge_picture()   Hap Q blocks with max |C - 128| of 30..33 and 62..65 (either sign, Co or Cg) and with C = 1 / 256

Everything is computed here (numpy, fixed seeds); nothing is read from disk.  Pictures are uint8 [h, w, 4] arrays made
of whole 4x4 blocks; block i of a sweep is block i of the picture in row-major block order.
"""
import numpy as np

BLOCK_ROW = 256                       # blocks per picture row of the block sweeps (1024 pixels)

E5 = np.array([(q << 3) | (q >> 2) for q in range(32)], dtype=np.int64)
E6 = np.array([(q << 2) | (q >> 4) for q in range(64)], dtype=np.int64)


def quant5(v):
    t = v * 31 + 128
    return (t + (t >> 8)) >> 8


def quant6(v):
    t = v * 63 + 128
    return (t + (t >> 8)) >> 8


def pad_blocks(blocks, row=BLOCK_ROW):
    """Repeats the first blocks until the count is a multiple of `row` (a whole picture row)."""
    n = len(blocks)
    extra = (-n) % row
    return np.concatenate([blocks, blocks[:extra]]) if extra else blocks


def picture_of_blocks(px, row=BLOCK_ROW):
    """px: uint8 [n, 16, 4] (texels of each block, row-major) -> picture [4 * rows, 4 * row, 4]; n is padded to whole
    rows first."""
    px = pad_blocks(px, row)
    rows = len(px) // row
    return np.ascontiguousarray(px.reshape(rows, row, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(rows * 4, row * 4, 4))


def blocks_of_picture(img):
    """Inverse of picture_of_blocks: [h, w, 4] -> [n, 16, 4]."""
    h, w = img.shape[:2]
    return img.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4)


def _pack_codes(codes, bits):
    """codes: int [n, 16] -> little-endian bytes of the 16 * bits index field, [n, 2 * bits]."""
    v = np.zeros(len(codes), dtype=np.uint64)
    for i in range(16):
        v |= codes[:, i].astype(np.uint64) << np.uint64(bits * i)
    return v.view(np.uint8).reshape(-1, 8)[:, : 2 * bits]


# ------------------------------------------------------------------------------------------- block sweeps (decode) --
def ramp_blocks():
    """uint8 [65536, 8]: block k = a0 (k >> 8), a1 (k & 255), texel p carries code (p + k) % 8."""
    k = np.arange(65536)
    codes = (np.arange(16)[None, :] + k[:, None]) % 8
    out = np.empty((65536, 8), dtype=np.uint8)
    out[:, 0] = k >> 8
    out[:, 1] = k & 255
    out[:, 2:] = _pack_codes(codes, 3)
    return out


def _colour_half(c0, c1, k):
    """8-byte colour blocks c0, c1 (16-bit), texel p of block k carrying index (p + k) % 4."""
    codes = (np.arange(16)[None, :] + np.asarray(k)[:, None]) % 4
    out = np.empty((len(c0), 8), dtype=np.uint8)
    out[:, 0:2] = np.asarray(c0, dtype=np.uint16).view(np.uint8).reshape(-1, 2)
    out[:, 2:4] = np.asarray(c1, dtype=np.uint16).view(np.uint8).reshape(-1, 2)
    out[:, 4:8] = _pack_codes(codes, 2)[:, :4]
    return out


def colour_endpoints():
    """(c0, c1) of the colour sweep, int64 arrays.  Part 1: green takes every ordered pair (4096), red every ordered
    pair 4 times over, blue every ordered pair through an odd stride; part 2 / 3: the same green and blue pairs with red
    (31, 0) and (0, 31), which put every green and blue pair into the c0 > c1 and the c0 < c1 order; part 4: c0 == c1
    for every 16-bit colour."""
    i = np.arange(4096)
    g0, g1 = i >> 6, i & 63
    r0, r1 = (i >> 5) & 31, i & 31
    j = (i * 37 + 5) & 1023
    b0, b1 = j >> 5, j & 31
    parts0, parts1 = [], []
    for rr0, rr1 in ((r0, r1), (np.full(4096, 31), np.zeros(4096, np.int64)), (np.zeros(4096, np.int64), np.full(4096, 31))):
        parts0.append(rr0 << 11 | g0 << 5 | b0)
        parts1.append(rr1 << 11 | g1 << 5 | b1)
    c = np.arange(65536)
    parts0.append(c)
    parts1.append(c)
    return np.concatenate(parts0).astype(np.int64), np.concatenate(parts1).astype(np.int64)


def colour_blocks():
    """uint8 [77824, 8] DXT1 blocks (also the colour half of the DXT5 sweep)."""
    c0, c1 = colour_endpoints()
    return _colour_half(c0, c1, np.arange(len(c0)))


def _palette_entries(e0, e1):
    """The four palette entries of the 4-colour mode, int64 [n, 4]."""
    return np.stack([e0, e1, (2 * e0 + e1) // 3, (e0 + 2 * e1) // 3], axis=-1)


def hapq_colour_endpoints():
    """(c0, c1) of the Hap Q colour sweep.  Red (Co) and blue (scale) are independent fields, and so are green (Cg)
    and blue: for each palette slot every reachable (Co byte, scale) pair gets a block with a representative red pair
    and blue pair, and the same block carries the next of the slot's (Cg byte, scale) pairs through a green pair."""
    p5 = np.array([(a, b) for a in range(32) for b in range(32)])
    p6 = np.array([(a, b) for a in range(64) for b in range(64)])
    pal5 = _palette_entries(E5[p5[:, 0]], E5[p5[:, 1]])                    # [1024, 4]
    pal6 = _palette_entries(E6[p6[:, 0]], E6[p6[:, 1]])                    # [4096, 4]
    scale = (pal5 >> 3) + 1                                                  # blue pairs -> scale per slot
    c0s, c1s = [], []
    for slot in range(4):
        s_vals, s_rep = np.unique(scale[:, slot], return_index=True)
        o_vals, o_rep = np.unique(pal5[:, slot], return_index=True)
        g_vals, g_rep = np.unique(pal6[:, slot], return_index=True)
        need_o = np.array([(o, s) for o in o_rep for s in s_rep])           # (red pair, blue pair)
        need_g = np.array([(g, s) for g in g_rep for s in s_rep])           # (green pair, blue pair)
        n = max(len(need_o), len(need_g))
        for t in range(n):
            ro, bo = need_o[t % len(need_o)]
            gg, bg = need_g[t % len(need_g)]
            for (r, g, b) in ((ro, gg, bo), (ro, gg, bg)) if bo != bg else ((ro, gg, bo),):
                c0s.append(p5[r, 0] << 11 | p6[g, 0] << 5 | p5[b, 0])
                c1s.append(p5[r, 1] << 11 | p6[g, 1] << 5 | p5[b, 1])
    return np.array(c0s, dtype=np.int64), np.array(c1s, dtype=np.int64)


def hapq_colour_blocks():
    """uint8 [n, 8] colour halves of scaled YCoCg-DXT5 blocks (always the 4-entry palette: no c0 > c1 rule)."""
    c0, c1 = hapq_colour_endpoints()
    return _colour_half(c0, c1, np.arange(len(c0)))


def cycle_to(a, n):
    """The rows of a repeated to n rows."""
    return a[np.arange(n) % len(a)]


def dxt5_sweep():
    """uint8 [n, 16]: ramp alpha halves (cycled) in front of the colour sweep, n covering both."""
    ramps, cols = ramp_blocks(), colour_blocks()
    n = max(len(ramps), len(cols))
    return pad_blocks(np.concatenate([cycle_to(ramps, n), cycle_to(cols, n)], axis=1))


def hapq_sweep():
    """(uint8 [n, 16] Hap Q blocks, uint8 [n, 8] RGTC1 alpha plane): the ramp sweep as luma and as alpha (the alpha
    plane shifted by half the ramp sweep so that Y and A differ), the Hap Q colour sweep cycled beside them."""
    ramps, cols = ramp_blocks(), hapq_colour_blocks()
    n = max(len(ramps), len(cols))
    blocks = pad_blocks(np.concatenate([cycle_to(ramps, n), cycle_to(cols, n)], axis=1))
    alpha = cycle_to(np.roll(ramps, 32768, axis=0), len(blocks))
    return blocks, np.ascontiguousarray(alpha)


# --------------------------------------------------------------- block sweeps (decode at half and quarter size) --
# The code fields above rotate ((p + k) % n): every 2 x 2 or 4 x 4 region of a block then holds every index equally
# often, its sums are multiples of 2 (half size) or 4 (quarter size), and the neighbours of the rounding term never
# occur.  The sweeps below keep the endpoints and take their codes from a seeded generator.
def recoded(blocks, field_offset, bits, seed):
    """A copy of `blocks` (uint8 [n, b]) whose 16-code field of 2 * bits bytes at byte field_offset holds seeded random
    codes; block k with k % 4 == 0 is flat, all 16 texels carrying code (k // 4) % (1 << bits).  Endpoints are kept."""
    n = len(blocks)
    codes = np.random.default_rng(seed).integers(0, 1 << bits, (n, 16))
    k = np.arange(0, n, 4)
    codes[k] = ((k // 4) % (1 << bits))[:, None]
    out = np.array(blocks, dtype=np.uint8, copy=True)
    out[:, field_offset: field_offset + 2 * bits] = _pack_codes(codes, bits)
    return out


def dxt1_scaled_sweep():
    """uint8 [77824, 8]: the colour sweep's endpoints with random indices."""
    return recoded(pad_blocks(colour_blocks()), 4, 2, 0xD171)


def dxt5_scaled_sweep():
    """uint8 [n, 16]: dxt5_sweep()'s endpoints, the alpha codes and the colour indices random (seeds of their own)."""
    return recoded(recoded(dxt5_sweep(), 2, 3, 0xD175A), 12, 2, 0xD175C)


def hapq_scaled_sweep():
    """(uint8 [n, 16] Hap Q blocks, uint8 [n, 8] RGTC1 alpha plane): hapq_sweep()'s endpoints -- the plane rolled as
    there -- with random luma codes, colour indices and plane codes."""
    blocks, alpha = hapq_sweep()
    return recoded(recoded(blocks, 2, 3, 0x4A91), 12, 2, 0x4A9C), recoded(alpha, 2, 3, 0x4A9A)


# ------------------------------------------------------------------------------------ pictures (encode) --
def ramp_picture():
    """Every pair lo < hi: ceil((d - 1) / 14) blocks (at least one) whose minimum is lo and maximum hi, together
    holding every value lo..hi; texel positions rotate from block to block.  R = G = B = A = the ramp value (Hap Q's
    luma of a grey is the grey itself)."""
    rows = []
    serial = 0
    for d in range(1, 256):
        lo = np.arange(256 - d)
        nb = max(1, -(-(d - 1) // 14))
        j = np.arange(nb)
        vals = np.empty((len(lo), nb, 16), dtype=np.int64)
        vals[..., 0] = lo[:, None]
        vals[..., 1] = lo[:, None] + d
        t = j[:, None] * 14 + np.arange(14)[None, :]                      # [nb, 14]
        inner = 1 + t % (d - 1) if d > 1 else np.where(np.arange(14) % 2 == 0, 0, 1)[None, :].repeat(nb, 0)
        vals[..., 2:] = lo[:, None, None] + inner[None, :, :]
        vals = vals.reshape(-1, 16)
        rot = (serial + np.arange(len(vals))) % 16
        serial += len(vals)
        idx = (np.arange(16)[None, :] - rot[:, None]) % 16                 # texel q takes slot (q - rot) % 16
        rows.append(np.take_along_axis(vals, idx, axis=1))
    v = np.concatenate(rows).astype(np.uint8)
    return picture_of_blocks(np.repeat(v[..., None], 4, axis=2))


# colour bit b: channel b >> 3, bit b & 7 (R = bits 0..7, G = 8..15, B = 16..23).  The picture has four regions, told
# apart by colour bits 4 and 20; in region q the 16 texels of a block differ in the four bits TEXEL_BITS[q] (from
# neighbouring values to opposite corners of the cube) and the other 18 bits count the region's blocks.
_REGION_BITS = (4, 20)
TEXEL_BITS = ((0, 8, 16, 1), (3, 11, 19, 10), (7, 15, 23, 14), (0, 13, 23, 6))


def all_colours_picture():
    """4096 x 4096: every 24-bit RGB colour exactly once.  A = G ^ B of the texel (an alpha plane with every value)."""
    k = np.arange(1 << 18, dtype=np.int64)
    regions = []
    for q in range(4):
        tb = TEXEL_BITS[q]
        free = [b for b in range(24) if b not in tb and b not in _REGION_BITS]
        base = (q & 1) << _REGION_BITS[0] | (q >> 1) << _REGION_BITS[1]
        for i, b in enumerate(free):
            base = base | ((k >> i) & 1) << b
        base = np.broadcast_to(base, k.shape) if np.ndim(base) == 0 else base
        p = np.arange(16, dtype=np.int64)
        off = np.zeros(16, dtype=np.int64)
        for i, b in enumerate(tb):
            off |= ((p >> i) & 1) << b
        regions.append(base[:, None] | off[None, :])
    c = np.concatenate(regions)                                              # [2^20, 16] colours
    # interleave the regions so that every block row mixes them
    c = c.reshape(4, -1, 16).transpose(1, 0, 2).reshape(-1, 16)
    px = np.empty(c.shape + (4,), dtype=np.uint8)
    px[..., 0] = c & 255
    px[..., 1] = (c >> 8) & 255
    px[..., 2] = (c >> 16) & 255
    px[..., 3] = px[..., 1] ^ px[..., 2]
    return picture_of_blocks(px, row=1024)


def channel_diffs(quant, expand):
    """{|expand(code a) - expand(code b)|: a, b the codes the encoder gives the inset box of a channel with values
    lo <= hi} -> (lo, hi) of the widest box that gives each (diff sorted ascending; widest: the most room for texels
    inside the box)."""
    lo, hi = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    m = lo <= hi
    lo, hi = lo[m], hi[m]
    ins = (hi - lo) >> 4
    diff = np.abs(expand[quant(hi - ins)] - expand[quant(lo + ins)])
    order = np.lexsort((lo, -(hi - lo), diff))
    vals, first = np.unique(diff[order], return_index=True)
    return vals, lo[order][first], hi[order][first]


def colour_block_model(px, m24_offset=0):
    """The colour half of the oracle's encoder (oracle/bc_oracle.c colour_block) in numpy: px int [n, 16, 3] ->
    dict of c0, c1, indices [n, 16], len2, m24 and the projections t [n, 16] (clamped).  m24_offset adds to
    floor(3 * 2^24 / len2) before the indices are taken: what a reciprocal off by one would write."""
    px = np.asarray(px, dtype=np.int64)
    lo, hi = px.min(axis=1), px.max(axis=1)
    d = 2 * px - (lo + hi)[:, None, :]
    cov_rg = (d[..., 0] * d[..., 1]).sum(axis=1)
    cov_bg = (d[..., 2] * d[..., 1]).sum(axis=1)
    ins = (hi - lo) >> 4
    lo, hi = lo + ins, hi - ins
    ar, br = np.where(cov_rg < 0, lo[:, 0], hi[:, 0]), np.where(cov_rg < 0, hi[:, 0], lo[:, 0])
    ab, bb = np.where(cov_bg < 0, lo[:, 2], hi[:, 2]), np.where(cov_bg < 0, hi[:, 2], lo[:, 2])
    qa = quant5(ar) << 11 | quant6(hi[:, 1]) << 5 | quant5(ab)
    qb = quant5(br) << 11 | quant6(lo[:, 1]) << 5 | quant5(bb)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    p0 = np.stack([E5[c0 >> 11], E6[(c0 >> 5) & 63], E5[c0 & 31]], axis=-1)
    p1 = np.stack([E5[c1 >> 11], E6[(c1 >> 5) & 63], E5[c1 & 31]], axis=-1)
    dirv = p0 - p1
    len2 = (dirv * dirv).sum(axis=1)
    base = (p1 * dirv).sum(axis=1)
    m24 = 50331648 // np.maximum(len2, 1) + m24_offset
    sixth = len2 // 6
    t = (px * dirv[:, None, :]).sum(axis=-1) + (sixth - base)[:, None]
    t = np.clip(t, 0, (len2 + sixth)[:, None])
    pos = np.minimum((t * m24[:, None]) >> 24, 3)
    idx = np.array([1, 3, 2, 0])[pos]
    idx[c0 == c1] = 0
    return {"c0": c0, "c1": c1, "indices": idx, "len2": len2, "m24": m24, "t": t, "dir": dirv, "base": base}


def ycocg_block_model(co, cg, m24_offset=0):
    """The colour half of the oracle's scaled YCoCg encoder (oracle/bc_oracle.c ycocg_colour_block) in numpy: co, cg
    int [n, 16] (1..256) -> dict of scale, c0, c1, indices, len2 and m24 (m24_offset as in colour_block_model)."""
    co, cg = np.asarray(co, dtype=np.int64), np.asarray(cg, dtype=np.int64)
    lo_o, hi_o, lo_g, hi_g = co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1)
    m = np.maximum(np.maximum(128 - lo_o, hi_o - 128), np.maximum(128 - lo_g, hi_g - 128))
    s = np.where(m <= 31, 4, np.where(m <= 63, 2, 1))
    cov = ((2 * co - (lo_o + hi_o)[:, None]) * (2 * cg - (lo_g + hi_g)[:, None])).sum(axis=1)
    lo_o, hi_o = (lo_o - 128) * s + 128, (hi_o - 128) * s + 128
    lo_g, hi_g = (lo_g - 128) * s + 128, (hi_g - 128) * s + 128
    ins = (hi_o - lo_o) >> 4
    lo_o, hi_o = lo_o + ins, hi_o - ins
    ins = (hi_g - lo_g) >> 4
    lo_g, hi_g = lo_g + ins, hi_g - ins
    ag, bg = np.where(cov < 0, lo_g, hi_g), np.where(cov < 0, hi_g, lo_g)
    qa = quant5(hi_o) << 11 | quant6(ag) << 5 | (s - 1)
    qb = quant5(lo_o) << 11 | quant6(bg) << 5 | (s - 1)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    p0 = np.stack([E5[c0 >> 11], E6[(c0 >> 5) & 63]], axis=-1)
    p1 = np.stack([E5[c1 >> 11], E6[(c1 >> 5) & 63]], axis=-1)
    dirv = p0 - p1
    len2 = (dirv * dirv).sum(axis=1)
    base = (p1 * dirv).sum(axis=1)
    m24 = 50331648 // np.maximum(len2, 1) + m24_offset
    sixth = len2 // 6
    v = np.stack([(co - 128) * s[:, None] + 128, (cg - 128) * s[:, None] + 128], axis=-1)
    t = np.clip((v * dirv[:, None, :]).sum(axis=-1) + (sixth - base)[:, None], 0, (len2 + sixth)[:, None])
    idx = np.array([1, 3, 2, 0])[np.minimum((t * m24[:, None]) >> 24, 3)]
    idx[c0 == c1] = 0
    return {"scale": s, "c0": c0, "c1": c1, "indices": idx, "len2": len2, "m24": m24}


def _boundary_intervals(len2, m24):
    """[6, n, 2] closed t intervals, for k = 1, 2, 3 and m24 + 1, m24 - 1: the projections t <= len2 + len2 / 6 at which
    (t * m24) >> 24 and (t * (m24 +- 1)) >> 24 fall on different sides of k (empty: lo > hi)."""
    top = len2 + len2 // 6
    out = []
    for k in (1, 2, 3):
        edge = -(-(k << 24) // m24)                                  # first t at k with m24
        plus = -(-(k << 24) // (m24 + 1))                            # ... with m24 + 1
        minus = -(-(k << 24) // (m24 - 1))                           # ... with m24 - 1
        out.append(np.stack([plus, np.minimum(edge - 1, top)], axis=-1))
        out.append(np.stack([edge, np.minimum(minus - 1, top)], axis=-1))
    return np.stack(out)


def _texel_in_box(lo, hi, dirv, s_lo, s_hi):
    """A texel x, lo <= x <= hi (int [3]), with s_lo <= x . dir <= s_hi, or None: every (red, blue) of the box is
    tried, green solved for."""
    xr = np.arange(lo[0], hi[0] + 1)[:, None]
    xb = np.arange(lo[2], hi[2] + 1)[None, :]
    rest = xr * dirv[0] + xb * dirv[2]
    if dirv[1] == 0:
        ok = (rest >= s_lo) & (rest <= s_hi)
        g = np.full(ok.shape, lo[1])
    else:
        g = np.maximum(-((rest - s_lo) // dirv[1]), lo[1])            # ceil((s_lo - rest) / dg), at least lo
        ok = (g <= hi[1]) & (rest + g * dirv[1] <= s_hi)
    hit = np.argwhere(ok)
    if not len(hit):
        return None
    i, j = hit[len(hit) // 2]
    return np.array([xr[i, 0], g[i, j], xb[0, j]])


def two_colour_boundary_blocks():
    """int [n, 16, 3] (one block per encodable len2) and bool [n, 6] (which of the six m24 +- 1 boundaries of
    _boundary_intervals some texel of the box can reach, and the block holds).  Ten texels sit on the box's top and
    bottom corners (they fix the box, and keep both covariances >= 0 whatever the rest holds: the endpoints are those
    of the two colours); the other six project onto the places where floor(3 * 2^24 / len2) off by one in either
    direction changes an index."""
    rv, rlo, rhi = channel_diffs(quant5, E5)
    gv, glo, ghi = channel_diffs(quant6, E6)
    l2 = (rv[:, None, None] ** 2 + gv[None, :, None] ** 2 + rv[None, None, :] ** 2).ravel()
    vals, first = np.unique(l2, return_index=True)
    first = first[vals > 0]
    ir, ig, ib = np.unravel_index(first, (len(rv), len(gv), len(rv)))
    n = len(first)
    top = np.stack([rhi[ir], ghi[ig], rhi[ib]], axis=-1)
    bottom = np.stack([rlo[ir], glo[ig], rlo[ib]], axis=-1)
    corners = np.concatenate([np.repeat(top[:, None], 8, axis=1), np.repeat(bottom[:, None], 8, axis=1)], axis=1)
    model = colour_block_model(corners)
    dirv, base, len2, m24 = model["dir"], model["base"], model["len2"], model["m24"]
    iv = _boundary_intervals(len2, m24)                                        # [6, n, 2] in t
    s_iv = iv - (len2 // 6 - base)[None, :, None]                              # ... in x . dir
    px = corners.copy()
    reached = np.zeros((n, 6), dtype=bool)
    # first the texels near the box diagonal (all blocks at once), then every texel of the box for what is left
    span = np.maximum((top * dirv).sum(axis=1) - (bottom * dirv).sum(axis=1), 1)
    d = np.arange(-4, 5)
    dr, db = np.meshgrid(d, d, indexing="ij")
    dr, db = dr.ravel()[None, :], db.ravel()[None, :]
    for j in range(6):
        s_lo, s_hi = s_iv[j, :, 0:1], s_iv[j, :, 1:2]
        lam = ((s_lo + s_hi) / 2 - (bottom * dirv).sum(axis=1)[:, None]) / span[:, None]
        diag = np.rint(bottom[:, None, :] + np.clip(lam, 0, 1)[..., None] * (top - bottom)[:, None, :]).astype(np.int64)
        xr = np.clip(diag[..., 0] + dr, bottom[:, 0:1], top[:, 0:1])
        xb = np.clip(diag[..., 2] + db, bottom[:, 2:3], top[:, 2:3])
        rest = xr * dirv[:, 0:1] + xb * dirv[:, 2:3]
        dg = np.maximum(dirv[:, 1:2], 1)
        g = np.where(dirv[:, 1:2] == 0, bottom[:, 1:2], np.maximum(-((rest - s_lo) // dg), bottom[:, 1:2]))
        sv = rest + g * dirv[:, 1:2]
        ok = (g <= top[:, 1:2]) & (sv >= s_lo) & (sv <= s_hi)
        found = ok.any(axis=1)
        c = ok.argmax(axis=1)
        b = np.flatnonzero(found)
        px[b, 10 + j] = np.stack([xr[b, c[b]], g[b, c[b]], xb[b, c[b]]], axis=-1)
        reached[b, j] = True
    for b, j in zip(*np.nonzero(~reached & (s_iv[:, :, 0] <= s_iv[:, :, 1]).T)):
        x = _texel_in_box(bottom[b], top[b], dirv[b], s_iv[j, b, 0], s_iv[j, b, 1])
        if x is not None:
            px[b, 10 + j] = x
            reached[b, j] = True
    # positions rotate from block to block
    rot = np.arange(n) % 16
    idx = (np.arange(16)[None, :] - rot[:, None]) % 16
    return np.take_along_axis(px, idx[..., None].repeat(3, axis=2), axis=1), reached


def encodable_len2():
    """Sorted len2 values (> 0) of the endpoint pairs the colour encoder can produce: the inset box rule shortens every
    channel, so only the per-channel differences channel_diffs() finds occur."""
    r, _, _ = channel_diffs(quant5, E5)
    g, _, _ = channel_diffs(quant6, E6)
    l2 = (r[:, None, None] ** 2 + g[None, :, None] ** 2 + r[None, None, :] ** 2).ravel()
    return np.unique(l2[l2 > 0])


def formable_len2():
    """Sorted len2 values (> 0) of any two distinct 5:6:5 codes (expanded differences, no encoder involved)."""
    d5 = np.unique(np.abs(E5[:, None] - E5[None, :]))
    d6 = np.unique(np.abs(E6[:, None] - E6[None, :]))
    l2 = (d5[:, None, None] ** 2 + d6[None, :, None] ** 2 + d5[None, None, :] ** 2).ravel()
    return np.unique(l2[l2 > 0])


def two_colour_picture():
    """two_colour_boundary_blocks() as a picture (alpha: 255 on the top corner texels, 0 elsewhere)."""
    px, _reached = two_colour_boundary_blocks()
    alpha = np.where((px == px.max(axis=1, keepdims=True)).all(axis=-1), 255, 0)
    return picture_of_blocks(np.concatenate([px, alpha[..., None]], axis=-1).astype(np.uint8))


def ycocg(rgb):
    """Co, Cg (1..256) of int RGB [..., 3] as the encoder forms them."""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return ((r - b + 1) >> 1) + 128, ((-r + 2 * g - b + 2) >> 2) + 128


SCALE_EDGES = (30, 31, 32, 33, 62, 63, 64, 65)
EXTREME_TEXELS = ((255, 128, 0), (0, 128, 255), (0, 255, 0), (255, 0, 255))      # Co 256, Co 1, Cg 256, Cg 1


def scale_edge_picture(per_case=256, seed=0x5CA1E):
    """Hap Q blocks whose largest |C - 128| is exactly m for m in SCALE_EDGES, reached by Co or Cg, above or below 128
    (one texel at the edge, 15 from inside the box |Co - 128|, |Cg - 128| <= m), and blocks holding one of the
    extreme texels of EXTREME_TEXELS among random ones."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (1 << 20, 3)).astype(np.int64)
    co, cg = ycocg(pool)
    co, cg = co - 128, cg - 128
    blocks = []
    for m in SCALE_EDGES:
        inside = pool[(np.abs(co) <= m) & (np.abs(cg) <= m)]
        for ch, other in ((co, cg), (cg, co)):
            for sign in (1, -1):
                edge = pool[(ch == sign * m) & (np.abs(other) <= m)]
                px = inside[rng.integers(0, len(inside), (per_case, 16))]
                px[np.arange(per_case), rng.integers(0, 16, per_case)] = edge[rng.integers(0, len(edge), per_case)]
                blocks.append(px)
    for t in EXTREME_TEXELS:
        px = pool[rng.integers(0, len(pool), (per_case, 16))]
        px[np.arange(per_case), rng.integers(0, 16, per_case)] = t
        blocks.append(px)
    rgb = np.concatenate(blocks)
    a = rng.integers(0, 256, rgb.shape[:2] + (1,))
    return picture_of_blocks(np.concatenate([rgb, a], axis=-1).astype(np.uint8))


ENCODE_PICTURES = {"ramps": ramp_picture, "all_colours": all_colours_picture, "two_colour": two_colour_picture,
                   "scale_edges": scale_edge_picture}

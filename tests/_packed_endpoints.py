"""Inputs and the numpy restatement for the pair form of the Hap Q colour half (hap_amd/csrc/bc_encode_core.hpp,
ycocg_colour_block): Co and Cg side by side as two 16-bit halves from the box to the index constants.

  pair_*()            the kernel's packed steps on int16 / uint16 arrays, so that a value that does not fit its half
                      wraps around here as it would there
  pair_form_block()   the whole colour half in that form: centred Co, Cg [n, 16] -> c0, c1, the index word
  box_grid_blocks()   two-colour blocks whose Co / Cg box corners run over a grid with -127, 128 and the thresholds of
                      the scale rule, in both covariance signs
  luma_range_blocks() grey blocks: every range d = 1..255 at several minima, every value of the range present

Everything is computed here (numpy, fixed order); nothing is read from disk."""
import numpy as np

import _value_space as V

I16, U16, I32 = np.int16, np.uint16, np.int32


# ------------------------------------------------------------------------------------- the pair form, step by step --
def pair_shift(m):
    """max(-lo, hi) over both channels (0..128) -> the scale as a shift count: 2, 1, 0 for m <= 31, <= 63, above."""
    return np.maximum(2 - (np.asarray(m, dtype=I16) >> 5), 0).astype(I16)


def pair_scale_inset(lo, hi, sh):
    """One half of lo | hi (int16, centred) -> the scaled and inset ends, uint16 (centred still: wrap-around)."""
    ls = (lo.astype(I16).view(U16) << sh.astype(U16)).astype(U16)
    hs = (hi.astype(I16).view(U16) << sh.astype(U16)).astype(U16)
    ins = ((hs - ls).astype(U16) >> U16(4)).astype(U16)
    return (ls + ins).astype(U16), (hs - ins).astype(U16)


def pair_quant(v, bits):
    """quant5 / quant6 of the biased value from the centred one: the constant carries 128 * mul + 128."""
    mul = U16(31 if bits == 5 else 63)
    add = U16(int(mul) * 128 + 128)
    t = (v.astype(U16) * mul + add).astype(U16)
    return (((t + (t >> U16(8))).astype(U16)) >> U16(8)).astype(U16)


def pair_expand(q, bits):
    up, down = (U16(3), U16(2)) if bits == 5 else (U16(2), U16(4))
    return ((q.astype(U16) << up).astype(U16) | (q.astype(U16) >> down)).astype(U16)


def dot2_i16(ax, ay, bx, by, acc):
    """v_dot2_i32_i16: signed halves, 32-bit products and sum (wrap-around)."""
    r = ax.astype(np.int64) * bx.astype(np.int64) + ay.astype(np.int64) * by.astype(np.int64) + np.asarray(acc, dtype=np.int64)
    return ((r + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int64)


def pair_setup(qo_a, qo_b, qg_a, qg_b, sh):
    """The quantised ends (uint16 halves) and the shift count -> c0, c1, swap, dir2 (Co, Cg int16), len2, K, top."""
    s1 = (np.int64(1) << sh.astype(np.int64)) - 1
    qa = qo_a.astype(np.int64) * 2048 + qg_a.astype(np.int64) * 32 + s1                 # v_dot2_u32_u16
    qb = qo_b.astype(np.int64) * 2048 + qg_b.astype(np.int64) * 32 + s1
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    sw = qa < qb
    q0o, q0g = np.where(sw, qo_b, qo_a).astype(U16), np.where(sw, qg_b, qg_a).astype(U16)
    q1o, q1g = np.where(sw, qo_a, qo_b).astype(U16), np.where(sw, qg_a, qg_b).astype(U16)
    p0o, p0g, p1o, p1g = pair_expand(q0o, 5), pair_expand(q0g, 6), pair_expand(q1o, 5), pair_expand(q1g, 6)
    d_o, d_g = (p0o - p1o).astype(U16).view(I16), (p0g - p1g).astype(U16).view(I16)
    b_o, b_g = (U16(128) - p1o).astype(U16).view(I16), (U16(128) - p1g).astype(U16).view(I16)
    len2 = dot2_i16(d_o, d_g, d_o, d_g, 0)
    dot_back = dot2_i16(d_o, d_g, b_o, b_g, 0)
    sixth = len2 // 6
    dir2_o = (d_o.view(U16) << sh.astype(U16)).astype(U16).view(I16)
    dir2_g = (d_g.view(U16) << sh.astype(U16)).astype(U16).view(I16)
    return c0, c1, sw, dir2_o, dir2_g, len2, dot_back + sixth, len2 + sixth


def pair_half_covariance(co, cg, lo_o, hi_o, lo_g, hi_g):
    """Half the covariance of the block as the kernel forms it: int16 sums, the reduced sums 4 mid - sums in int16,
    one dot product with 2 prod as its accumulator."""
    co16, cg16 = co.astype(I16), cg.astype(I16)
    prod = (co16.astype(np.int64) * cg16.astype(np.int64)).sum(axis=1)
    sum_o, sum_g = np.zeros(len(co), dtype=I16), np.zeros(len(co), dtype=I16)
    for i in range(16):
        sum_o, sum_g = (sum_o + co16[:, i]).astype(I16), (sum_g + cg16[:, i]).astype(I16)
    mid_o, mid_g = (lo_o.astype(I16) + hi_o.astype(I16)).astype(I16), (lo_g.astype(I16) + hi_g.astype(I16)).astype(I16)
    rest_o = ((mid_o.view(U16) << U16(2)).astype(U16) - sum_o.view(U16)).astype(U16).view(I16)
    rest_g = ((mid_g.view(U16) << U16(2)).astype(U16) - sum_g.view(U16)).astype(U16).view(I16)
    return dot2_i16(rest_o, rest_g, mid_g, mid_o, 2 * prod)


def pair_form_block(co, cg):
    """The colour half in the pair form: co, cg int [n, 16], centred (-127..128) -> (c0, c1, index word)."""
    co, cg = np.asarray(co, dtype=np.int64), np.asarray(cg, dtype=np.int64)
    lo_o, hi_o, lo_g, hi_g = (a.astype(I16) for a in (co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1)))
    m = np.maximum(np.maximum(-lo_o, hi_o), np.maximum(-lo_g, hi_g))
    sh = pair_shift(m)
    neg = pair_half_covariance(co, cg, lo_o, hi_o, lo_g, hi_g) < 0
    lo_os, hi_os = pair_scale_inset(lo_o, hi_o, sh)
    lo_gs, hi_gs = pair_scale_inset(lo_g, hi_g, sh)
    a_g, b_g = np.where(neg, lo_gs, hi_gs), np.where(neg, hi_gs, lo_gs)
    c0, c1, _sw, d_o, d_g, len2, K, top = pair_setup(pair_quant(hi_os, 5), pair_quant(lo_os, 5), pair_quant(a_g, 6),
                                                     pair_quant(b_g, 6), sh)
    m24 = 50331648 // np.maximum(len2, 1)
    t = dot2_i16(co.astype(I16), cg.astype(I16), d_o[:, None], d_g[:, None], K[:, None])
    t = np.clip(t, 0, top[:, None])
    pos = (t * m24[:, None]) >> 24
    assert pos.max(initial=0) <= 3
    idx = np.array([1, 3, 2, 0])[pos]
    idx[c0 == c1] = 0
    return c0, c1, sum(idx[:, k] << (2 * k) for k in range(16))


# ------------------------------------------------------------------------------------------------------ inputs --
GRID = (-127, -64, -63, -32, -31, -1, 0, 1, 31, 32, 63, 64, 128)      # box corners: the extremes, the scale rule's edges

_rgb_of = None


def rgb_of_chroma():
    """int16 [256, 256, 3]: an RGB colour with Co - 128 = i - 127 and Cg - 128 = j - 127, or -1 where no colour has."""
    global _rgb_of
    if _rgb_of is None:
        r, g = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
        table = np.full((256, 256, 3), -1, dtype=np.int16)
        for b in range(256):                        # a slice of the cube at a time
            rgb = np.stack([r, g, np.full_like(r, b)], axis=-1)
            co, cg = V.ycocg(rgb)                   # 1..256 each
            table[co - 1, cg - 1] = rgb
        _rgb_of = table
    return _rgb_of


def box_grid_blocks():
    """(uint8 [n, 16, 4], int [n, 4]): two-colour blocks and their boxes (lo_o, hi_o, lo_g, hi_g, centred).  For every
    Co pair and Cg pair of GRID with lo <= hi: the colours (lo_o, lo_g) and (hi_o, hi_g) -- covariance >= 0 -- and
    (lo_o, hi_g) and (hi_o, lo_g) -- covariance <= 0 --, wherever RGB colours with those chroma values exist.  The
    number of texels of the first colour runs 1..15 and their places rotate from block to block; alpha counts."""
    table = rgb_of_chroma()
    pairs = [(a, b) for a in GRID for b in GRID if a <= b]
    px, boxes = [], []
    serial = 0
    for lo_o, hi_o in pairs:
        for lo_g, hi_g in pairs:
            for first, second in (((lo_o, lo_g), (hi_o, hi_g)), ((lo_o, hi_g), (hi_o, lo_g))):
                ca, cb = table[first[0] + 127, first[1] + 127], table[second[0] + 127, second[1] + 127]
                if ca[0] < 0 or cb[0] < 0:
                    continue
                k = 1 + serial % 15
                texel = np.where((((np.arange(16) + serial) % 16) < k)[:, None], ca[None, :], cb[None, :])
                px.append(np.concatenate([texel, ((np.arange(16) * 17 + serial) % 256)[:, None]], axis=1))
                boxes.append((lo_o, hi_o, lo_g, hi_g))
                serial += 1
    return np.array(px, dtype=np.uint8), np.array(boxes, dtype=np.int64)


def luma_range_blocks():
    """uint8 [n, 16, 4] grey blocks (R = G = B = A: Hap Q's luma of a grey is the grey, its chroma the centre): for every
    range d = 1..255 and the minima 0, 1, (255 - d) / 2 and 255 - d, ceil((d - 1) / 14) blocks (at least one) holding
    the minimum, the maximum and between them every value of the range; places rotate from block to block."""
    rows = []
    serial = 0
    for d in range(1, 256):
        nb = max(1, -(-(d - 1) // 14))
        inner = (1 + (np.arange(nb * 14) % (d - 1))) if d > 1 else np.arange(nb * 14) % 2
        for a1 in sorted({0, min(1, 255 - d), (255 - d) // 2, 255 - d}):
            vals = np.empty((nb, 16), dtype=np.int64)
            vals[:, 0], vals[:, 1] = a1, a1 + d
            vals[:, 2:] = a1 + inner.reshape(nb, 14)
            rot = (serial + np.arange(nb)) % 16
            serial += nb
            rows.append(np.take_along_axis(vals, (np.arange(16)[None, :] - rot[:, None]) % 16, axis=1))
    v = np.concatenate(rows).astype(np.uint8)
    return np.repeat(v[..., None], 4, axis=2)

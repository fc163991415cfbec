"""The pixel loops of the Hap Q colour half on NON-NEGATIVE Co | Cg pairs (hap_amd/csrc/bc_encode_core.hpp,
ycocg_colour_block: Co and Cg 1..256, the definition's own values, side by side in one 32-bit word) restated in numpy,
and the pictures that reach the edges of that representation.

  biased_*()          the kernel's steps on uint32 words and their int16 / float16 halves, so that a carry between the
                      halves, a value that does not fit its half or a half that orders wrongly as an IEEE half shows
                      here as it would there; the per-block steps behind them are tests/_packed_endpoints.py's
  biased_form_block() the whole colour half in that form: Co, Cg [n, 16] in 1..256 -> c0, c1, the index word
  extreme_*()         blocks at the ends of the chroma range (1, 2, 128, 255, 256 a channel)
  pictures()          the picture set of tests/test_biased_pairs_gpu.py, none larger than 256 x 64

Everything is computed here (numpy, fixed order; the noise of hap_amd.synth); nothing is read from disk."""
import numpy as np

import _packed_endpoints as PE
import _value_space as V

I16, U16, U32, F16 = np.int16, np.uint16, np.uint32, np.float16

EXTREMES = (-127, -126, 0, 127, 128)           # Co - 128, Cg - 128: both ends of the range, next to one end, the centre


# ------------------------------------------------------------------------------------- the pixel loops, step by step --
def words(co, cg):
    """Co | Cg << 16 as the transform leaves them: uint32 [n, 16]."""
    co, cg = np.asarray(co, dtype=np.int64), np.asarray(cg, dtype=np.int64)
    assert co.min() >= 1 and co.max() <= 256 and cg.min() >= 1 and cg.max() <= 256
    return (co | cg << 16).astype(U32)


def halves(w):
    """(low, high) halves of uint32 words as uint16."""
    w = np.asarray(w, dtype=U32)
    return (w & U32(0xFFFF)).astype(U16), (w >> U32(16)).astype(U16)


def _f16_pick3(pick, a, b, c):
    """One half of v_pk_minimum3_f16 / v_pk_maximum3_f16: the operands read as IEEE halves, the result's bits."""
    return pick(pick(a.view(F16), b.view(F16)), c.view(F16)).view(U16)


def biased_box(w):
    """The box in eight three-input steps a side, as the kernel walks it: (lo, hi) uint32 words."""
    lo_h, hi_h = [], []
    for h in halves(w):
        lo, hi = _f16_pick3(np.minimum, h[:, 0], h[:, 1], h[:, 2]), _f16_pick3(np.maximum, h[:, 0], h[:, 1], h[:, 2])
        for i in range(3, 15, 2):
            lo, hi = _f16_pick3(np.minimum, lo, h[:, i], h[:, i + 1]), _f16_pick3(np.maximum, hi, h[:, i], h[:, i + 1])
        lo_h.append(_f16_pick3(np.minimum, lo, h[:, 15], h[:, 15]))
        hi_h.append(_f16_pick3(np.maximum, hi, h[:, 15], h[:, 15]))
    return (lo_h[0].astype(U32) | lo_h[1].astype(U32) << U32(16)), (hi_h[0].astype(U32) | hi_h[1].astype(U32) << U32(16))


def biased_sums(w):
    """Sum Co | sum Cg << 16 by sixteen 32-bit adds on the words (wrap-around at 32 bits)."""
    total = np.zeros(len(w), dtype=U32)
    for i in range(16):
        total = (total + w[:, i]).astype(U32)
    return total


def centred_words_sum(co, cg):
    """The same adds on the words of the CENTRED form, (Co - 128) | (Cg - 128) << 16 as signed halves: what Part R12
    tried, and where every negative Co carries into Cg's half."""
    co16, cg16 = (np.asarray(co) - 128).astype(I16).view(U16), (np.asarray(cg) - 128).astype(I16).view(U16)
    return biased_sums(co16.astype(U32) | cg16.astype(U32) << U32(16))


def biased_half_covariance(w, lo, hi):
    """Half the covariance from the biased words: prod by v_mad_i32_i16 (32-bit), the sums' halves read as int16,
    mid = lo + hi and 4 mid - sums in int16, one dot product with 2 prod as its accumulator."""
    co, cg = (h.view(I16).astype(np.int64) for h in halves(w))
    prod = np.zeros(len(w), dtype=np.int64)
    for i in range(16):
        prod = PE.dot2_i16(co[:, i], np.zeros_like(co[:, i]), cg[:, i], np.zeros_like(co[:, i]), prod)
    sum_o, sum_g = (h.view(I16) for h in halves(biased_sums(w)))
    (lo_o, lo_g), (hi_o, hi_g) = (tuple(h.view(I16) for h in halves(x)) for x in (lo, hi))
    mid_o, mid_g = (lo_o + hi_o).astype(I16), (lo_g + hi_g).astype(I16)
    rest_o = ((mid_o.view(U16) << U16(2)).astype(U16) - sum_o.view(U16)).astype(U16).view(I16)
    rest_g = ((mid_g.view(U16) << U16(2)).astype(U16) - sum_g.view(U16)).astype(U16).view(I16)
    return PE.dot2_i16(rest_o, rest_g, mid_g, mid_o, 2 * prod)


def biased_constant(dir2_o, dir2_g, k_centred):
    """The projection's accumulator for biased pixels: one more v_dot2_i32_i16, s dir . (-128 | -128) on top of K'."""
    minus = np.full(np.shape(dir2_o), -128, dtype=I16)
    return PE.dot2_i16(np.asarray(dir2_o, dtype=I16), np.asarray(dir2_g, dtype=I16), minus, minus, k_centred)


def biased_form_block(co, cg):
    """The colour half as the kernel has it: co, cg int [n, 16] in 1..256 -> (c0, c1, index word)."""
    w = words(co, cg)
    lo, hi = biased_box(w)
    neg = biased_half_covariance(w, lo, hi) < 0
    # once a block: the box recentred (v_pk_sub_i16), and from there tests/_packed_endpoints.py's per-block steps
    (lo_o, lo_g), (hi_o, hi_g) = (tuple((h - U16(128)).astype(U16).view(I16) for h in halves(x)) for x in (lo, hi))
    m = np.maximum(np.maximum(-lo_o, hi_o), np.maximum(-lo_g, hi_g))
    sh = PE.pair_shift(m)
    lo_os, hi_os = PE.pair_scale_inset(lo_o, hi_o, sh)
    lo_gs, hi_gs = PE.pair_scale_inset(lo_g, hi_g, sh)
    a_g, b_g = np.where(neg, lo_gs, hi_gs), np.where(neg, hi_gs, lo_gs)
    c0, c1, _sw, d_o, d_g, len2, k_centred, top = PE.pair_setup(PE.pair_quant(hi_os, 5), PE.pair_quant(lo_os, 5),
                                                                PE.pair_quant(a_g, 6), PE.pair_quant(b_g, 6), sh)
    k = biased_constant(d_o, d_g, k_centred)
    m24 = 50331648 // np.maximum(len2, 1)
    co_h, cg_h = (h.view(I16) for h in halves(w))
    t = np.clip(PE.dot2_i16(co_h, cg_h, d_o[:, None], d_g[:, None], k[:, None]), 0, top[:, None])
    pos = (t * m24[:, None]) >> 24
    assert pos.max(initial=0) <= 3
    idx = np.array([1, 3, 2, 0])[pos]
    idx[c0 == c1] = 0
    return c0, c1, sum(idx[:, k] << (2 * k) for k in range(16))


# ------------------------------------------------------------------------------------------------------ inputs --
def _two_colour(ca, cb, serial):
    """One block of colours ca and cb: 1 + serial % 15 texels of the first, places rotating with serial; alpha counts."""
    k = 1 + serial % 15
    texel = np.where((((np.arange(16) + serial) % 16) < k)[:, None], np.asarray(ca)[None, :], np.asarray(cb)[None, :])
    return np.concatenate([texel, ((np.arange(16) * 17 + serial) % 256)[:, None]], axis=1)


_colours = None


def extreme_colours():
    """int [n, 3]: for EVERY (R, B) whose Co - 128 is one of EXTREMES, every G that makes Cg - 128 one of them too --
    and, for the (R, B) that no such G exists for, G = 0 and 255 (the ends of the Cg that pair can reach)."""
    global _colours
    if _colours is None:
        r, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
        keep = np.isin(((r - b + 1) >> 1), EXTREMES)
        r, b = r[keep], b[keep]
        out = []
        for ri, bi in zip(r, b):
            g = np.arange(256, dtype=np.int64)
            cg = (-ri + 2 * g - bi + 2) >> 2
            gs = g[np.isin(cg, EXTREMES)]
            if not len(gs):
                gs = np.array([0, 255])
            out.extend((ri, gi, bi) for gi in gs)
        _colours = np.array(out, dtype=np.int64)
    return _colours


def extreme_blocks():
    """(a) uint8 [n, 16, 4]: every colour of extreme_colours() in a two-colour block with another of them (the partner
    runs through the list at a stride coprime to its length), then every ordered pair of the distinct (Co, Cg) corners
    those colours reach."""
    c = extreme_colours()
    n = len(c)
    px = [_two_colour(c[i], c[(i * 37 + 11) % n], i) for i in range(n)]
    co, cg = V.ycocg(c)
    _, first = np.unique(np.stack([co, cg], axis=1), axis=0, return_index=True)
    corner = c[np.sort(first)]
    serial = n
    for i in range(len(corner)):
        for j in range(len(corner)):
            if i != j:
                px.append(_two_colour(corner[i], corner[j], serial))
                serial += 1
    return np.array(px, dtype=np.uint8)


def flat_blocks():
    """(b) uint8 [n, 16, 4]: blocks of ONE colour (c0 == c1) for every distinct (Co, Cg) that extreme_colours() reaches,
    and for the four corners of the RGB cube that make Co or Cg 1 or 256."""
    c = extreme_colours()
    co, cg = V.ycocg(c)
    _, first = np.unique(np.stack([co, cg], axis=1), axis=0, return_index=True)
    cols = np.concatenate([c[np.sort(first)], np.array(V.EXTREME_TEXELS, dtype=np.int64)])
    return np.array([_two_colour(x, x, i) for i, x in enumerate(cols)], dtype=np.uint8)


def full_range_blocks():
    """(c) uint8 [n, 16, 4]: the box touches 1 and 256 in one channel and is flat in the other.  Co: (0 or 1, G, 255)
    against (255, G, 0), both with R + B = 255, so one Cg for every G.  Cg: (0, 255, 0) against (255, 0, 255) or
    (254, 0, 255), Co = 128 all three.  Every split 1..15."""
    px = []
    serial = 0
    for g in (0, 1, 127, 128, 254, 255):
        for k in range(15):
            px.append(_two_colour((0, g, 255), (255, g, 0), serial))
            serial += 1
    for low in ((255, 0, 255), (254, 0, 255)):
        for k in range(15):
            px.append(_two_colour((0, 255, 0), low, serial))
            serial += 1
    return np.array(px, dtype=np.uint8)


def noise_picture(amplitude, frame):
    """(d) uint8 [16, 16, 4], 4 x 4 blocks: mid grey plus the low bits of a hap_amd.synth frame folded to
    -amplitude..amplitude a channel, so |Co - 128| and |Cg - 128| stay at or below the amplitude (+ 1 for Cg)."""
    from hap_amd import synth
    n = synth.rgba_frame(16, 16, frame_index=frame).numpy().astype(np.int64)
    n = (n * 0x9E5 + np.arange(16)[None, :, None] * 77 + np.arange(16)[:, None, None] * 131) % (2 * amplitude + 1) - amplitude
    out = np.clip(128 + n, 0, 255)
    out[..., 3] = 255
    return np.ascontiguousarray(out.astype(np.uint8))


NOISE_AMPLITUDES = {4: 12, 2: 40, 1: 120}       # scale -> amplitude: m <= 31, 32..63, above


def _cycled(blocks, n):
    """The blocks repeated in their order until there are n of them."""
    return blocks[np.arange(n) % len(blocks)]


def pictures():
    """{name: uint8 [h, w, 4]}: (a) in pictures of 256 x 64 (1024 blocks, two fragments), (b) and (c) in one, (d) three
    of 16 x 16, (e) 256 x 60, whose second fragment is ragged (448 of 512 blocks)."""
    import _data as D
    out = {}
    a = extreme_blocks()
    for i in range(0, len(a), 1024):
        out["a%d" % (i // 1024)] = V.picture_of_blocks(_cycled(a[i: i + 1024], 1024), 64)
    out["bc"] = V.picture_of_blocks(_cycled(np.concatenate([flat_blocks(), full_range_blocks()]), 1024), 64)
    for scale, amp in NOISE_AMPLITUDES.items():
        out["d-scale%d" % scale] = noise_picture(amp, 3 + scale)
    out["e"] = D.rgba(256, 60, frame=31)                       # (a frame whose field stream is half its texture)
    return out

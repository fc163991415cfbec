"""The arithmetic substitutions of the block encoder (hap_amd/csrc/bc_encode_core.hpp), each restated in numpy next to
the expression it replaced and compared over its WHOLE input domain, then pinned against oracle/bc_oracle.c (built by
oracle/Makefile) -- the definition -- not against the kernel.  CPU only.

  1. ramp codes.  Was: position r = x >> 20, code = table[r] (0->0, 7->1, r->r+1), a byte-table lookup per pixel.
     Now: x + 2^20, the 3-bit field holds (r + 1) mod 8, and eight fields at a time get
     w ^= ~((w >> 1) | (w >> 2)) & 0x249249.   Domains: every 24-bit word of fields (2^24); every (a0, a1, a) with
     a1 <= a <= a0 (the encoder's a0 / a1 are the block's maximum and minimum: 2 829 056 triples, and all 256^3 for
     the field itself); the oracle on tests/_value_space.ramp_picture(), which holds every one of those triples.
  2. Hap Q colour index set-up.  Was: pack both 5:6:5 words, order them, unpack and expand again, make_projection over
     three channels with |dir|, complement masks and their 255 |dir| constants, then K and the signed direction from
     those.  Now: the ordered pair's entries from the quantised channels at hand, signed direction directly,
     K = len2 / 6 + sum dir (128 - 128 s - p1).  Domain: every (Co pair, Cg pair, scale) = 32^2 x 64^2 x 3 =
     12 582 912 cases; per case K, the direction pair, len2 are integers that do not depend on the pixel, and the
     per-pixel expression (dot * sm + Km) >> 24 is unchanged -- so equality of these IS equality for every pixel.
     Against the oracle: the scale-edge sweep, the Hap Q colour sweep and 2^17 seeded random blocks (sample size
     stated; the per-pixel expression did not change, the set-up is what the exhaustive part covers).
"""
import numpy as np

import _data as D
import _libs as L
import _value_space as V

M8 = 0x249249


def ramp_codes(w):
    return w ^ (~((w >> 1) | (w >> 2)) & M8)


CODE_OF = np.array([0, 2, 3, 4, 5, 6, 7, 1], dtype=np.int64)      # ramp position -> S3TC code


def test_ramp_code_fixup_on_every_24_bit_word():
    w = np.arange(1 << 24, dtype=np.int64)
    want = np.zeros_like(w)
    for k in range(8):
        f = (w >> (3 * k)) & 7                    # the field holds (r + 1) mod 8
        want |= CODE_OF[(f - 1) & 7] << (3 * k)
    assert np.array_equal(ramp_codes(w), want)


def test_ramp_position_plus_one_over_every_a0_a1_a():
    """old: table[((14 u + bias) m) >> 20]; new: fix-up of ((x + 2^20) >> 20) & 7 -- all 256^3 (a0, a1, a), the
    products in the 32-bit wrap-around arithmetic of v_mad_i32_i24 (a0 <= a1 and a outside a1..a0 included: not
    reachable, but the identity does not need the range)."""
    a1, a = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for a0 in range(256):
        d = a0 - a1
        dd = np.where(d > 0, d, 1)
        m = (1 << 19) // dd + 1
        x = ((14 * (a0 - a) + np.maximum(d - 6, 0)) * m) & 0xFFFFFFFF
        reach = (d > 0) & (a >= a1) & (a <= a0)
        assert int(x[reach].max(initial=0)) < (1 << 23)
        old = CODE_OF[(x >> 20) & 7]
        new = ramp_codes((((x + (1 << 20)) & 0xFFFFFFFF) >> 20) & 7) & 7
        assert np.array_equal(old, new), a0
        assert np.all(((x[reach] >> 20) & ~7) == 0)


def test_ramp_codes_against_the_oracle_on_every_reachable_triple():
    img = V.ramp_picture()
    blocks = np.frombuffer(D.oracle_bc_encode(img, L.FMT_RGTC1), dtype=np.uint8).reshape(-1, 8).astype(np.int64)
    a = V.blocks_of_picture(img)[..., 3].astype(np.int64)                     # [n, 16]
    a0, a1 = a.max(axis=1), a.min(axis=1)
    assert np.array_equal(blocks[:, 0], a0) and np.array_equal(blocks[:, 1], a1)
    d = a0 - a1
    assert d.min() >= 1
    seen = np.zeros((256, 256, 256), dtype=bool)
    seen[a0[:, None].repeat(16, 1), a1[:, None].repeat(16, 1), a] = True
    want_seen = np.zeros_like(seen)
    for hi in range(256):
        for lo in range(hi):
            want_seen[hi, lo, lo:hi + 1] = True
    assert np.array_equal(seen, want_seen)                                    # 2 829 056 triples, every one present
    m = (1 << 19) // d + 1
    start = a0 * 14 * m + np.maximum(d - 6, 0) * m + (1 << 20)
    f = ((start[:, None] - a * (14 * m)[:, None]) >> 20) & 7
    lo24 = sum(f[:, k] << (3 * k) for k in range(8))
    hi24 = sum(f[:, 8 + k] << (3 * k) for k in range(8))
    bits = ramp_codes(lo24) | (ramp_codes(hi24) << 24)
    got = sum(blocks[:, 2 + k] << (8 * k) for k in range(6))
    assert np.array_equal(bits, got)


def _old_setup(qo_a, qo_b, qg_a, qg_b, s):
    """bc_encode_core.hpp before: 5:6:5 words, ordered, expanded again, three-channel make_projection, K, dir2."""
    qa = qo_a << 11 | qg_a << 5 | (s - 1)
    qb = qo_b << 11 | qg_b << 5 | (s - 1)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    p0 = [V.E5[c0 >> 11], V.E6[(c0 >> 5) & 63], np.zeros_like(c0)]
    p1 = [V.E5[c1 >> 11], V.E6[(c1 >> 5) & 63], np.zeros_like(c0)]
    neg = base = len2 = 0
    adir, down = [], []
    for c in range(3):
        dirc = p0[c] - p1[c]
        ad = np.abs(dirc)
        adir.append(ad)
        down.append(dirc < 0)
        neg = neg + np.where(dirc < 0, ad, 0)
        base = base + p1[c] * dirc
        len2 = len2 + ad * ad
    sixth = len2 // 6
    start = sixth - base - 255 * neg
    K = start + adir[0] * np.where(down[0], 127 + 128 * s, 128 - 128 * s) + adir[1] * np.where(down[1], 127 + 128 * s, 128 - 128 * s)
    return c0, c1, np.where(down[0], -adir[0], adir[0]), np.where(down[1], -adir[1], adir[1]), len2, K


def _new_setup(qo_a, qo_b, qg_a, qg_b, s):
    qa = qo_a << 11 | qg_a << 5 | (s - 1)
    qb = qo_b << 11 | qg_b << 5 | (s - 1)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    sw = qa < qb
    eo_a, eo_b, eg_a, eg_b = V.E5[qo_a], V.E5[qo_b], V.E6[qg_a], V.E6[qg_b]
    d_o, d_g = np.where(sw, eo_b - eo_a, eo_a - eo_b), np.where(sw, eg_b - eg_a, eg_a - eg_b)
    p1_o, p1_g = np.where(sw, eo_a, eo_b), np.where(sw, eg_a, eg_b)
    len2 = d_o * d_o + d_g * d_g
    centre = 128 - 128 * s
    K = d_o * (centre - p1_o) + d_g * (centre - p1_g) + len2 // 6
    return c0, c1, d_o, d_g, len2, K


def test_hapq_index_setup_over_every_endpoint_pair_and_scale():
    qo_a, qo_b, qg_a, qg_b = np.meshgrid(np.arange(32, dtype=np.int64), np.arange(32, dtype=np.int64),
                                         np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    cases = 0
    for s in (1, 2, 4):
        old = _old_setup(qo_a, qo_b, qg_a, qg_b, s)
        new = _new_setup(qo_a, qo_b, qg_a, qg_b, s)
        for name, o, n in zip(("c0", "c1", "dir Co", "dir Cg", "len2", "K"), old, new):
            assert np.array_equal(o, n), (s, name)
        # the operands stay inside the 24-bit signed multiplier and the 16-bit direction pair
        assert np.abs(new[2]).max() <= 255 and np.abs(new[3]).max() <= 255 and int(np.abs(new[5]).max()) < (1 << 23)
        cases += qo_a.size
    assert cases == 12582912


def _hapq_model_new(co, cg):
    """ycocg_colour_block with the new set-up, the per-pixel expression in the kernel's wrap-around form."""
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
    c0, c1, d_o, d_g, len2, K = _new_setup(V.quant5(hi_o), V.quant5(lo_o), V.quant6(ag), V.quant6(bg), s)
    m24 = 50331648 // np.maximum(len2, 1)
    off = 1 << 17
    dot = co * d_o[:, None] + cg * d_g[:, None] + off
    assert dot.min() >= 1 and dot.max() < (1 << 24)
    v = (dot * (s * m24)[:, None] + (((K - s * off) * m24) & 0xFFFFFFFF)[:, None]) & 0xFFFFFFFF
    v = np.where(v >= (1 << 31), v - (1 << 32), v)                           # as a signed 32-bit value
    pos = np.clip(v >> 24, 0, 3)
    idx = np.array([1, 3, 2, 0])[pos]
    idx[c0 == c1] = 0
    return c0, c1, idx


def test_hapq_colour_half_against_the_oracle():
    rng = np.random.default_rng(0x1DE7)
    sample = 1 << 17                                                         # seeded random blocks (sample size: 131 072)
    rnd = rng.integers(0, 256, (sample, 16, 4)).astype(np.uint8)
    near = (rng.integers(0, 256, (sample, 1, 4)) + rng.integers(-24, 25, (sample, 16, 4))).clip(0, 255).astype(np.uint8)
    extremes = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255],
                         [255, 0, 255]], dtype=np.uint8)
    corners = np.zeros((64 * 16, 16, 4), dtype=np.uint8)                     # every pair of extreme colours, the second at each texel
    for i in range(8):
        for j in range(8):
            for k in range(16):
                corners[(i * 8 + j) * 16 + k, :, :3] = extremes[i]
                corners[(i * 8 + j) * 16 + k, k, :3] = extremes[j]
    pictures = [V.picture_of_blocks(rnd), V.picture_of_blocks(near), V.picture_of_blocks(corners), V.scale_edge_picture()]
    for img in pictures:
        blocks = np.frombuffer(D.oracle_bc_encode(img, L.FMT_YCOCG), dtype=np.uint8).reshape(-1, 16)
        px = V.blocks_of_picture(img).astype(np.int64)
        co, cg = V.ycocg(px[..., :3])
        c0, c1, idx = _hapq_model_new(co, cg)
        w = blocks[:, 8:].astype(np.int64)
        assert np.array_equal(w[:, 0] | w[:, 1] << 8, c0) and np.array_equal(w[:, 2] | w[:, 3] << 8, c1)
        got = (w[:, 4] | w[:, 5] << 8 | w[:, 6] << 16 | w[:, 7] << 24)
        want = sum(idx[:, k] << (2 * k) for k in range(16))
        assert np.array_equal(got, want)

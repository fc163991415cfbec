"""The pair form of the Hap Q colour half (hap_amd/csrc/bc_encode_core.hpp, ycocg_colour_block: Co and Cg as two 16-bit
halves of one register from the box to the index constants) restated in numpy on int16 / uint16 arrays
(tests/_packed_endpoints.py: a value that does not fit its half wraps around there as it would in the kernel) and
compared with the definition, oracle/bc_oracle.c's ycocg_colour_block -- its expressions in 64-bit integers stage by
stage, and the C function itself (built by oracle/Makefile) on whole blocks.  CPU only; nothing is sampled in (a), (b).

  (a) per channel: every lo <= hi in -127..128 and every scale the rule for m allows (m is at least the channel's own
      max(-lo, hi); the other channel can only lower the scale), as the 5-bit and as the 6-bit channel: the scaled, inset,
      quantised and expanded values of both ends.
  (b) across channels: every (qo_a, qo_b, qg_a, qg_b, s), 32 * 32 * 64 * 64 * 3 = 12 582 912 cases: c0, c1, the swap,
      the scaled direction, len2, K and top.
  (c) the covariance: its value over random blocks in random boxes and over blocks of extreme corners.
  Whole blocks: the box grid, the scale edges and random blocks through the C oracle."""
import numpy as np

import _data as D
import _libs as L
import _packed_endpoints as PE
import _value_space as V


def _shift_of(m):
    return np.where(m <= 31, 2, np.where(m <= 63, 1, 0))


def test_shift_count_is_the_scale_rule_for_every_m():
    m = np.arange(0, 129)
    assert np.array_equal(PE.pair_shift(m), _shift_of(m))
    assert np.array_equal((1 << PE.pair_shift(m).astype(np.int64)), np.where(m <= 31, 4, np.where(m <= 63, 2, 1)))


def test_per_channel_scale_inset_quantise_expand():
    lo, hi = np.meshgrid(np.arange(-127, 129, dtype=np.int64), np.arange(-127, 129, dtype=np.int64), indexing="ij")
    keep = lo <= hi
    lo, hi = lo[keep], hi[keep]
    own = _shift_of(np.maximum(-lo, hi))
    cases = 0
    for sh in (0, 1, 2):
        ok = own >= sh                                                  # the rule allows this scale or a larger one
        l, h = lo[ok], hi[ok]
        s = 1 << sh
        # the definition: biased, 64-bit
        lo_b, hi_b = l * s + 128, h * s + 128
        ins = (hi_b - lo_b) >> 4
        lo_b, hi_b = lo_b + ins, hi_b - ins
        assert lo_b.min() >= 0 and hi_b.max() <= 256
        # the pair form: centred, 16-bit
        shv = np.full(len(l), sh, dtype=np.int16)
        ls, hs = PE.pair_scale_inset(l.astype(np.int16), h.astype(np.int16), shv)
        assert np.array_equal(ls.view(np.int16).astype(np.int64) + 128, lo_b), sh
        assert np.array_equal(hs.view(np.int16).astype(np.int64) + 128, hi_b), sh
        for bits, quant, expand in ((5, V.quant5, V.E5), (6, V.quant6, V.E6)):
            for got_in, want_in in ((ls, lo_b), (hs, hi_b)):
                q = PE.pair_quant(got_in, bits)
                assert np.array_equal(q.astype(np.int64), quant(want_in)), (sh, bits)
                assert np.array_equal(PE.pair_expand(q, bits).astype(np.int64), expand[quant(want_in)]), (sh, bits)
        cases += len(l)
    assert cases == 256 * 257 // 2 + 127 * 128 // 2 + 63 * 64 // 2      # every lo <= hi in -127..128, in +-63, in +-31


def _definition_setup(qo_a, qo_b, qg_a, qg_b, s):
    """oracle/bc_oracle.c: the words ordered, the ends unpacked from them and expanded, the projection of
    pick_indices on v = c' s + 128 (c' the centred pixel): t = s (c' . dir) + K, K = len2 / 6 - p1 . dir + 128 sum dir."""
    qa = qo_a << 11 | qg_a << 5 | (s - 1)
    qb = qo_b << 11 | qg_b << 5 | (s - 1)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    p0o, p0g, p1o, p1g = V.E5[c0 >> 11], V.E6[(c0 >> 5) & 63], V.E5[c1 >> 11], V.E6[(c1 >> 5) & 63]
    d_o, d_g = p0o - p1o, p0g - p1g
    len2 = d_o * d_o + d_g * d_g
    sixth = len2 // 6
    K = sixth - (p1o * d_o + p1g * d_g) + 128 * (d_o + d_g)
    return c0, c1, qa < qb, d_o * s, d_g * s, len2, K, len2 + sixth


def test_across_channels_every_quantised_pair_and_scale():
    qo_a, qo_b, qg_a, qg_b = np.meshgrid(np.arange(32, dtype=np.int64), np.arange(32, dtype=np.int64),
                                         np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    cases = 0
    for sh in (0, 1, 2):
        want = _definition_setup(qo_a, qo_b, qg_a, qg_b, 1 << sh)
        got = PE.pair_setup(qo_a.astype(np.uint16), qo_b.astype(np.uint16), qg_a.astype(np.uint16), qg_b.astype(np.uint16),
                            np.full(qo_a.shape, sh, dtype=np.int16))
        for name, w, g in zip(("c0", "c1", "swap", "dir2 Co", "dir2 Cg", "len2", "K", "top"), want, got):
            assert np.array_equal(w, np.asarray(g).astype(w.dtype)), (sh, name)
        assert np.abs(want[3]).max() <= 1020 and np.abs(want[4]).max() <= 1020
        cases += qo_a.size
    assert cases == 12582912


def _covariance(co, cg):
    mo, mg = co.min(axis=1) + co.max(axis=1), cg.min(axis=1) + cg.max(axis=1)
    return ((2 * co - mo[:, None]) * (2 * cg - mg[:, None])).sum(axis=1)


def _pair_half_cov(co, cg):
    return PE.pair_half_covariance(co, cg, co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1))


def test_covariance_value_over_random_boxes_and_extreme_corners():
    rng = np.random.default_rng(0xC0FA)
    n = 1 << 16                                                              # seeded random boxes (sample size: 65 536)
    edge = rng.integers(-127, 129, (n, 2, 2))
    lo, hi = edge.min(axis=1), edge.max(axis=1)
    co = rng.integers(lo[:, None, 0], hi[:, None, 0] + 1, (n, 16))
    cg = rng.integers(lo[:, None, 1], hi[:, None, 1] + 1, (n, 16))
    assert np.array_equal(2 * _pair_half_cov(co, cg), _covariance(co, cg))
    # extreme corners: every texel at -127 or 128 in each channel -- every split k : 16 - k between every ordered
    # pair of the four corners, and 4096 blocks of corners drawn at random
    corner = np.array([(a, b) for a in (-127, 128) for b in (-127, 128)])
    blocks = [np.where((np.arange(16) < k)[:, None], corner[i][None, :], corner[j][None, :])
              for i in range(4) for j in range(4) for k in range(17)]
    blocks = np.concatenate([np.array(blocks), corner[rng.integers(0, 4, (4096, 16))]])
    co, cg = blocks[..., 0], blocks[..., 1]
    want = _covariance(co, cg)
    assert np.array_equal(2 * _pair_half_cov(co, cg), want)
    assert want.min() == -16 * 255 * 255 and want.max() == 16 * 255 * 255    # both ends of the value's range are there


def _blocks_against_oracle(px, what):
    img = V.picture_of_blocks(px)
    blocks = np.frombuffer(D.oracle_bc_encode(img, L.FMT_YCOCG), dtype=np.uint8).reshape(-1, 16)
    rgb = V.blocks_of_picture(img).astype(np.int64)[..., :3]
    co, cg = V.ycocg(rgb)
    c0, c1, idx = PE.pair_form_block(co - 128, cg - 128)
    w = blocks[:, 8:].astype(np.int64)
    assert np.array_equal(w[:, 0] | w[:, 1] << 8, c0) and np.array_equal(w[:, 2] | w[:, 3] << 8, c1), what
    assert np.array_equal(w[:, 4] | w[:, 5] << 8 | w[:, 6] << 16 | w[:, 7] << 24, idx), what


def test_box_grid_holds_what_it_says():
    px, boxes = PE.box_grid_blocks()
    assert 2000 <= len(px) <= 20000
    co, cg = V.ycocg(px.astype(np.int64)[..., :3])
    co, cg = co - 128, cg - 128
    got = np.stack([co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1)], axis=1)
    assert np.array_equal(got, boxes)
    for ch in (0, 2):
        assert {-127, 128, 31, 32, 63, 64, -31, -32, -63, -64} <= set(boxes[:, ch]) | set(boxes[:, ch + 1])
    cov = _covariance(co, cg)
    assert (cov < 0).sum() > 500 and (cov > 0).sum() > 500 and (cov == 0).sum() > 100
    m = np.abs(boxes).max(axis=1)
    for edge in (31, 32, 63, 64, 128):
        assert (m == edge).any()
    # both orders of the two words, and blocks of one colour
    sh = PE.pair_shift(m)
    neg = cov < 0
    ends = [PE.pair_scale_inset(boxes[:, c].astype(np.int16), boxes[:, c + 1].astype(np.int16), sh) for c in (0, 2)]
    a_g, b_g = np.where(neg, ends[1][0], ends[1][1]), np.where(neg, ends[1][1], ends[1][0])
    c0, c1, sw = PE.pair_setup(PE.pair_quant(ends[0][1], 5), PE.pair_quant(ends[0][0], 5), PE.pair_quant(a_g, 6),
                               PE.pair_quant(b_g, 6), sh)[:3]
    assert sw.sum() > 20 and (~sw & (c0 != c1)).sum() > 1000 and (c0 == c1).sum() > 10


def test_pair_form_blocks_against_the_oracle():
    rng = np.random.default_rng(0x9A1F)
    sample = 1 << 15                                                         # seeded random blocks (sample size: 32 768 each)
    rnd = rng.integers(0, 256, (sample, 16, 4)).astype(np.uint8)
    near = (rng.integers(0, 256, (sample, 1, 4)) + rng.integers(-12, 13, (sample, 16, 4))).clip(0, 255).astype(np.uint8)
    _blocks_against_oracle(PE.box_grid_blocks()[0], "box grid")
    _blocks_against_oracle(V.blocks_of_picture(V.scale_edge_picture()), "scale edges")
    _blocks_against_oracle(rnd, "random")
    _blocks_against_oracle(near, "near")
    _blocks_against_oracle(PE.luma_range_blocks(), "luma ranges")

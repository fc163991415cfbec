"""The pixel loops of the Hap Q colour half on non-negative Co | Cg pairs (hap_amd/csrc/bc_encode_core.hpp,
ycocg_colour_block; restated in tests/_biased_pairs.py on uint32 words and their int16 / float16 halves) against the
definition, oracle/bc_oracle.c -- its expressions in 64-bit integers, and the C function itself on whole blocks.
CPU only; nothing is sampled except where a sample size is stated.

  order        for every a, b in 0..256 the minimum / maximum of the two read as IEEE halves is the integers'; so is
               the three-input form's over {0, 1, 2, 127, 128, 129, 255, 256}^3, and the eight-step box over blocks
  sums         sum Co | sum Cg by plain 32-bit adds on the words: every count 0..16 of extreme pixels, in either
               channel and both; the centred form's counter-example of LABNOTES Part R12 (sixteen pixels of
               Co - 128 = -127: sixteen off there) passes here
  covariance   the sign and the value, also where it is the smallest it can be on either side of zero.  The
               covariance, sum (2 Co - mo)(2 Cg - mg), is EVEN for every block (an odd term needs mo and mg odd, and
               then all sixteen terms are odd), so -1 and +1 are values of the HALF covariance, which is what the
               kernel forms and takes the sign of: blocks with half covariance -1, 0, +1 at both ends of the range
  constant     the projection's accumulator K = K' - 128 (s d_o + s d_g) for every scale at the largest and the
               smallest directions, and t for EVERY biased pixel there against the definition's t on the centred one
  whole blocks the picture set of tests/test_biased_pairs_gpu.py and random blocks through the C oracle"""
import numpy as np

import _biased_pairs as BP
import _data as D
import _libs as L
import _packed_endpoints as PE
import _value_space as V

U16, F16 = np.uint16, np.float16


def test_halves_0_to_256_order_as_ieee_halves():
    a, b = np.meshgrid(np.arange(257, dtype=U16), np.arange(257, dtype=U16), indexing="ij")
    assert np.array_equal(np.minimum(a.view(F16), b.view(F16)).view(U16), np.minimum(a, b))
    assert np.array_equal(np.maximum(a.view(F16), b.view(F16)).view(U16), np.maximum(a, b))
    assert 256 < 0x7C00 and np.isfinite(np.array([256], dtype=U16).view(F16)).all()      # far below infinity's pattern
    s = np.array([0, 1, 2, 127, 128, 129, 255, 256], dtype=U16)
    x, y, z = (g.ravel() for g in np.meshgrid(s, s, s, indexing="ij"))
    assert np.array_equal(BP._f16_pick3(np.minimum, x, y, z), np.minimum(np.minimum(x, y), z))
    assert np.array_equal(BP._f16_pick3(np.maximum, x, y, z), np.maximum(np.maximum(x, y), z))


def _extreme_count_blocks():
    """Blocks with k pixels at one corner of the range and 16 - k at another, every k = 0..16, every ordered pair of the
    corners (Co, Cg) in {1, 256}^2, the k pixels in rotating places: int [n, 16] each."""
    corner = [(a, b) for a in (1, 256) for b in (1, 256)]
    co, cg = [], []
    serial = 0
    for ca in corner:
        for cb in corner:
            for k in range(17):
                first = ((np.arange(16) + serial) % 16) < k
                co.append(np.where(first, ca[0], cb[0]))
                cg.append(np.where(first, ca[1], cb[1]))
                serial += 1
    return np.array(co, dtype=np.int64), np.array(cg, dtype=np.int64)


def test_pair_sums_are_plain_32_bit_adds():
    co, cg = _extreme_count_blocks()
    rng = np.random.default_rng(0xB1A5)
    co = np.concatenate([co, rng.integers(1, 257, (1 << 14, 16))])              # seeded random blocks (sample size: 16 384)
    cg = np.concatenate([cg, rng.integers(1, 257, (1 << 14, 16))])
    lo, hi = BP.halves(BP.biased_sums(BP.words(co, cg)))
    assert np.array_equal(lo.astype(np.int64), co.sum(axis=1)) and np.array_equal(hi.astype(np.int64), cg.sum(axis=1))
    assert co.sum(axis=1).min() == 16 and co.sum(axis=1).max() == 4096 and cg.sum(axis=1).max() == 4096
    # Part R12's counter-example: sixteen pixels of Co - 128 = -127.  On the centred words the adds are sixteen off in
    # Cg's half; on the biased words of the same pixels they are right.
    co, cg = np.full((1, 16), 1, dtype=np.int64), np.full((1, 16), 140, dtype=np.int64)
    centred = BP.halves(BP.centred_words_sum(co, cg))[1].view(np.int16).astype(np.int64)
    assert centred[0] - (cg - 128).sum() == 15                   # sixteen carries in, one borrow out for the negative total
    lo, hi = BP.halves(BP.biased_sums(BP.words(co, cg)))
    assert (int(lo[0]), int(hi[0])) == (16, 16 * 140)


def _covariance(co, cg):
    mo, mg = co.min(axis=1) + co.max(axis=1), cg.min(axis=1) + cg.max(axis=1)
    return ((2 * co - mo[:, None]) * (2 * cg - mg[:, None])).sum(axis=1)


def _half_cov(co, cg):
    w = BP.words(co, cg)
    lo, hi = BP.biased_box(w)
    return BP.biased_half_covariance(w, lo, hi)


def _smallest_covariance_blocks():
    """Co in {a, a + 1}, Cg in {b, b + 1}: every term of the covariance is +-1, so `agree` pixels where both channels
    are at the same end and 16 - agree where they are not give 2 agree - 16: half covariance -1, 0, +1 for 7, 8, 9.
    a, b at both ends of the range and in the middle."""
    co, cg, want = [], [], []
    serial = 0
    for a in (1, 128, 255):
        for b in (1, 128, 255):
            for agree in (7, 8, 9):
                up_o = (np.arange(16) % 2) == 0                                  # eight pixels at each end of Co
                same = np.concatenate([np.arange(16)[up_o][: (agree + 1) // 2], np.arange(16)[~up_o][: agree // 2]])
                up_g = np.where(np.isin(np.arange(16), same), up_o, ~up_o)
                roll = serial % 16
                co.append(np.roll(a + up_o, roll))
                cg.append(np.roll(b + up_g, roll))
                want.append(agree - 8)
                serial += 1
    return np.array(co, dtype=np.int64), np.array(cg, dtype=np.int64), np.array(want, dtype=np.int64)


def test_covariance_sign_and_value_on_biased_pairs():
    co, cg, want = _smallest_covariance_blocks()
    assert sorted(set(want)) == [-1, 0, 1]
    assert np.array_equal(_covariance(co, cg), 2 * want) and np.array_equal(_covariance(co - 128, cg - 128), 2 * want)
    assert np.array_equal(_half_cov(co, cg), want)
    # the value over random boxes and over blocks of extreme corners (both ends of its range)
    rng = np.random.default_rng(0xC0FB)
    n = 1 << 15                                                                  # seeded random boxes (sample size: 32 768)
    edge = rng.integers(1, 257, (n, 2, 2))
    lo, hi = edge.min(axis=1), edge.max(axis=1)
    rco = rng.integers(lo[:, None, 0], hi[:, None, 0] + 1, (n, 16))
    rcg = rng.integers(lo[:, None, 1], hi[:, None, 1] + 1, (n, 16))
    xco, xcg = _extreme_count_blocks()
    for c_o, c_g in ((rco, rcg), (xco, xcg)):
        cov = _covariance(c_o, c_g)
        assert (cov % 2 == 0).all() and np.array_equal(2 * _half_cov(c_o, c_g), cov)
    cov = _covariance(xco, xcg)
    assert cov.min() == -16 * 255 * 255 and cov.max() == 16 * 255 * 255
    # every intermediate in its half: mid 2..512, 4 mid - sums inside int16 by a wide margin
    mid, sums = xco.min(axis=1) + xco.max(axis=1), xco.sum(axis=1)
    assert mid.min() >= 2 and mid.max() <= 512 and (4 * mid - sums).min() >= -3068 and (4 * mid - sums).max() <= 2032


def test_projection_constant_for_biased_pixels():
    # ends (quantised) that give the largest and the smallest directions, with both signs and both orders of the words
    qo = np.array([0, 31, 0, 31, 5, 5, 6, 17], dtype=np.int64)
    qo_b = np.array([31, 0, 31, 0, 5, 5, 5, 17], dtype=np.int64)
    qg = np.array([0, 63, 63, 0, 9, 10, 9, 40], dtype=np.int64)
    qg_b = np.array([63, 0, 0, 63, 10, 9, 9, 41], dtype=np.int64)
    co, cg = (g.ravel() for g in np.meshgrid(np.arange(1, 257, dtype=np.int64), np.arange(1, 257, dtype=np.int64), indexing="ij"))
    seen = set()
    for sh in (0, 1, 2):
        shv = np.full(len(qo), sh, dtype=np.int16)
        _c0, _c1, _sw, d_o, d_g, len2, k_centred, _top = PE.pair_setup(qo.astype(U16), qo_b.astype(U16), qg.astype(U16),
                                                                      qg_b.astype(U16), shv)
        k = BP.biased_constant(d_o, d_g, k_centred)
        do64, dg64 = d_o.astype(np.int64), d_g.astype(np.int64)
        assert np.array_equal(k, k_centred - 128 * (do64 + dg64))
        assert np.abs(k).max() < 1 << 19
        assert np.abs(do64).max() == 255 << sh and np.abs(dg64).max() == 255 << sh and len2.min() == 16 and len2.max() == 130050
        for i in range(len(qo)):
            # the definition on the centred pixel, 64-bit, against the kernel's dot product on the biased pair
            want = (co - 128) * do64[i] + (cg - 128) * dg64[i] + k_centred[i]
            got = PE.dot2_i16(co.astype(np.int16), cg.astype(np.int16), d_o[i], d_g[i], k[i])
            assert np.array_equal(got, want), (sh, i)
            seen.add((int(np.sign(do64[i])), int(np.sign(dg64[i]))))
    assert {(1, 1), (-1, -1), (1, -1), (-1, 1), (0, 1), (0, -1), (1, 0)} <= seen | {(-s[0], -s[1]) for s in seen}


def _blocks_against_oracle(px, what):
    img = V.picture_of_blocks(BP._cycled(px, -(-len(px) // V.BLOCK_ROW) * V.BLOCK_ROW))      # whole picture rows
    blocks = np.frombuffer(D.oracle_bc_encode(img, L.FMT_YCOCG), dtype=np.uint8).reshape(-1, 16)
    rgb = V.blocks_of_picture(img).astype(np.int64)[..., :3]
    co, cg = V.ycocg(rgb)
    # the box by three-input half minima / maxima is the integers'
    lo, hi = BP.biased_box(BP.words(co, cg))
    assert np.array_equal(BP.halves(lo)[0], co.min(axis=1)) and np.array_equal(BP.halves(lo)[1], cg.min(axis=1)), what
    assert np.array_equal(BP.halves(hi)[0], co.max(axis=1)) and np.array_equal(BP.halves(hi)[1], cg.max(axis=1)), what
    c0, c1, idx = BP.biased_form_block(co, cg)
    w = blocks[:, 8:].astype(np.int64)
    assert np.array_equal(w[:, 0] | w[:, 1] << 8, c0) and np.array_equal(w[:, 2] | w[:, 3] << 8, c1), what
    assert np.array_equal(w[:, 4] | w[:, 5] << 8 | w[:, 6] << 16 | w[:, 7] << 24, idx), what
    return c0, c1


def test_extreme_blocks_hold_what_they_say():
    c = BP.extreme_colours()
    co, cg = V.ycocg(c)
    assert set(co - 128) == set(BP.EXTREMES) and set(cg - 128) == set(BP.EXTREMES)
    # every (R, B) that makes Co - 128 one of the five is there
    r, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    keep = np.isin((r - b + 1) >> 1, BP.EXTREMES)
    assert {(int(x), int(y)) for x, y in zip(r[keep], b[keep])} == {(int(x[0]), int(x[2])) for x in c}
    for px, ch in ((BP.full_range_blocks()[:90], 0), (BP.full_range_blocks()[90:], 1)):
        v = V.ycocg(px.astype(np.int64)[..., :3])
        assert (v[ch].min(axis=1) == 1).all() and (v[ch].max(axis=1) == 256).all()
        assert (v[1 - ch].min(axis=1) == v[1 - ch].max(axis=1)).all()


def test_biased_form_blocks_against_the_oracle():
    _blocks_against_oracle(BP.extreme_blocks(), "extremes")
    c0, c1 = _blocks_against_oracle(BP.flat_blocks(), "flat")
    assert (c0 == c1).all()
    c0, c1 = _blocks_against_oracle(BP.full_range_blocks(), "full range")
    assert (c0 != c1).all() and ((c0 & 31) == 0).all()                          # scale 1: the blue field is s - 1
    scales = set()
    for scale, amp in BP.NOISE_AMPLITUDES.items():
        c0, _ = _blocks_against_oracle(V.blocks_of_picture(BP.noise_picture(amp, 3 + scale)), "noise %d" % scale)
        assert ((c0 & 31) == scale - 1).mean() >= 0.5, scale                    # the picture's blocks are mostly at its scale
        scales.add(scale)
    assert scales == {1, 2, 4}
    rng = np.random.default_rng(0x9A20)
    sample = 1 << 14                                                            # seeded random blocks (sample size: 16 384 each)
    _blocks_against_oracle(rng.integers(0, 256, (sample, 16, 4)).astype(np.uint8), "random")
    near = (rng.integers(0, 256, (sample, 1, 4)) + rng.integers(-12, 13, (sample, 16, 4))).clip(0, 255).astype(np.uint8)
    _blocks_against_oracle(near, "near")
    _blocks_against_oracle(PE.box_grid_blocks()[0], "box grid")
    _blocks_against_oracle(V.blocks_of_picture(V.scale_edge_picture()), "scale edges")

"""Sum Co and sum Cg of a Hap Q block by plain 32-bit adds of its sixteen Co | Cg words (hap_amd/csrc/bc_encode_core.hpp,
ycocg_colour_block) -- what holds, stated in numpy on 32-bit words, and why the kernel keeps its packed adds.

The proposal: add the sixteen words cc[i] = (Co - 128) & 0xFFFF | (Cg - 128) << 16 as 32-bit integers (three operands
an instruction), then put the borrow of the low half back once, acc += (acc & 0x8000) << 1, and read sum Co mod 2^16 and
sum Cg from the halves.

  * The fix-up is right for the word (sum Cg << 16) + sum Co, for every pair of totals a block can have
    (test_fixup_restores_every_pair_of_totals).
  * The sum of the words is not that word.  A negative Co stands in its half as Co + 2^16, so every pixel with a
    negative Co carries one into the upper half, not the total once: after the fix-up the upper half is
    sum Cg + (number of pixels with Co < 0).  That number cannot be had from the sum
    (test_word_sum_carries_once_per_negative_co), so the packed adds, whose halves do not carry, stay.
  * With the pixels in integer form, (Cg << 16) + Co, the proposal holds through to the covariance's sign
    (test_integer_form_reaches_the_covariance_sign): the identity is one of the words' form, which the transform does
    not produce."""
import numpy as np

import _packed_endpoints as PE

M32 = np.int64(0xFFFFFFFF)


def fix_up(acc):
    """acc += (acc & 0x8000) << 1 on 32-bit words (held in int64)."""
    return (acc + ((acc & 0x8000) << 1)) & M32


def halves(acc):
    """A 32-bit word's halves as signed 16-bit numbers."""
    lo = (acc & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    hi = (acc >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    return lo, hi


def blocks():
    """Centred Co, Cg [n, 16] in -127..128: the extremes, alternating ones, and random blocks (fixed seed)."""
    rng = np.random.default_rng(12)
    ext = []
    for a in (-127, 128, -1, 0, 1):
        for b in (-127, 128, -1, 0, 1):
            ext.append((np.full(16, a), np.full(16, b)))
            ext.append((np.where(np.arange(16) & 1, a, b), np.where(np.arange(16) & 1, b, a)))
            ext.append((np.where(np.arange(16) & 1, a, -a + 1), np.full(16, b)))
    co = np.array([e[0] for e in ext], dtype=np.int64)
    cg = np.array([e[1] for e in ext], dtype=np.int64)
    n = 4096
    wide = rng.integers(-127, 129, size=(2, n, 16))
    centre = rng.integers(-127, 129, size=(2, n, 1))
    narrow = np.clip(centre + rng.integers(-9, 10, size=(2, n, 16)), -127, 128)
    co = np.concatenate([co, wide[0], narrow[0]])
    cg = np.concatenate([cg, wide[1], narrow[1]])
    assert co.min() == -127 and co.max() == 128 and cg.min() == -127 and cg.max() == 128
    return co, cg


def test_fixup_restores_every_pair_of_totals():
    """Every (sum Co, sum Cg) of sixteen values in -127..128, as the wrapped 32-bit word (sum Cg << 16) + sum Co."""
    so = np.arange(-2032, 2049, dtype=np.int64)
    cases = 0
    for sg0 in range(-2032, 2049, 256):
        sg = np.arange(sg0, min(sg0 + 256, 2049), dtype=np.int64)[:, None]
        acc = ((sg << 16) + so[None, :]) & M32
        # |sum Co| <= 2048: bit 15 of the low half is its sign, and the borrow it took from the upper half
        assert np.array_equal((acc >> 15) & 1, np.broadcast_to((so < 0).astype(np.int64)[None, :], acc.shape))
        lo, hi = halves(fix_up(acc))
        assert np.array_equal(lo, np.broadcast_to(so[None, :], acc.shape))
        assert np.array_equal(hi, np.broadcast_to(sg, acc.shape))
        cases += acc.size
    assert cases == 4081 * 4081


def test_word_sum_carries_once_per_negative_co():
    """The kernel's words, halves side by side: their 32-bit sum's upper half is off by the count of negative Co."""
    co, cg = blocks()
    words = ((cg & 0xFFFF) << 16) | (co & 0xFFFF)
    acc = words.sum(axis=1) & M32
    lo, hi = halves(fix_up(acc))
    neg = (co < 0).sum(axis=1)
    assert np.array_equal(lo, co.sum(axis=1))
    assert np.array_equal(hi, cg.sum(axis=1) + neg)
    # equal to the per-half sums only where no Co is negative ...
    assert np.array_equal(hi == cg.sum(axis=1), neg == 0)
    # ... and sixteen pixels of Co = -127 are sixteen off
    lo1, hi1 = halves(fix_up(np.array([16 * (((5 & 0xFFFF) << 16) | (-127 & 0xFFFF))], dtype=np.int64) & M32))
    assert (int(lo1[0]), int(hi1[0])) == (16 * -127, 16 * 5 + 16)


def test_integer_form_reaches_the_covariance_sign():
    """Pixels as (Cg << 16) + Co: sum, fix-up, halves -- the per-half sums, and with them the kernel's half covariance."""
    co, cg = blocks()
    acc = ((cg << 16) + co).sum(axis=1) & M32
    lo, hi = halves(fix_up(acc))
    assert np.array_equal(lo, co.sum(axis=1)) and np.array_equal(hi, cg.sum(axis=1))
    I16, U16 = np.int16, np.uint16
    lo_o, hi_o, lo_g, hi_g = (a.astype(I16) for a in (co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1)))
    mid_o, mid_g = (lo_o + hi_o).astype(I16), (lo_g + hi_g).astype(I16)
    rest_o = ((mid_o.view(U16) << U16(2)).astype(U16) - lo.astype(I16).view(U16)).astype(U16).view(I16)
    rest_g = ((mid_g.view(U16) << U16(2)).astype(U16) - hi.astype(I16).view(U16)).astype(U16).view(I16)
    half_cov = PE.dot2_i16(rest_o, rest_g, mid_g, mid_o, 2 * (co * cg).sum(axis=1))
    want = PE.pair_half_covariance(co, cg, lo_o, hi_o, lo_g, hi_g)
    assert np.array_equal(half_cov, want)
    # (half the covariance itself, from the definition: 4 sum Co Cg - 2 mg sum Co - 2 mo sum Cg + 16 mo mg, halved)
    mo, mg = mid_o.astype(np.int64), mid_g.astype(np.int64)
    cov = 4 * (co * cg).sum(axis=1) - 2 * mg * co.sum(axis=1) - 2 * mo * cg.sum(axis=1) + 16 * mo * mg
    assert np.array_equal(half_cov * 2, cov)
    assert np.array_equal(half_cov < 0, cov < 0)

"""The luma half of the fused Hap Q kernel (hap_amd/csrc/bc_encode_core.hpp: ycocg_weight_rows_biased, ycocg_addend,
luma_block_negated), restated in numpy (tests/_luma_ramp.py) and compared over its whole domain.  CPU only.

  1. Row 0 of the matrix product, weights -64, -128, -64, 0 as signed bytes on the pixel's bytes less 128, addend 32576:
     for all 2^24 (R, G, B) it is 256 (255 - Y) + 64 (3 - f), S = R + 2G + B + 2 = 4Y + f, and lies in 0..65535 -- byte 1
     is 255 - Y exactly, byte 0 is 0, 64, 128 or 192.  The source holds that dword and that addend.
  2. The ramp field.  Was, on a = Y - 128: v_mad_i32_i24, v_lshrrev_b32 by 20, v_alignbit_b32 by 3.  Now, on the row's
     value: v_mad_u32_u24 by 2 * 14 m from start << 9, v_alignbit_b32 by 29 -- stated with the instruction's 24-bit
     operand masks and 32-bit wrap-around.  For every d in 1..255, every a1 in 0..255 - d, every pixel value in
     a1..a1 + d and every junk byte 0, 64, 128, 192: both give (r + 1) mod 8 of the definition's
     r = ((14 u + max(d - 6, 0)) m) >> 20.
  3. Both block forms against oracle/bc_oracle.c's own bytes (through tests/_libs): a Hap Q picture whose blocks hold,
     for every d and a1, the two ends and every value between them, with f = 0..3 from unequal R, G, B -- the eight luma
     bytes of every block from luma_block_negated's model on the row's values, from alpha_block<128>'s model on Y - 128,
     and from the oracle are the same.
"""
import os
import re

import numpy as np

import _data as D
import _libs as L
import _luma_ramp as R
import test_index_selection_identity as I

JUNK = (0, 64, 128, 192)


def test_the_weight_dword_is_the_row_and_the_source_holds_it():
    assert np.array_equal(np.array([R.ROW0_DWORD], dtype="<u4").view(np.int8).astype(np.int64), R.ROW0)
    src = open(os.path.join(os.path.dirname(__file__), "..", "hap_amd", "csrc", "bc_encode_core.hpp")).read()
    helper = src[src.index("unsigned ycocg_weight_rows_biased()"):]
    helper = helper[: helper.index("return r;")]
    assert [int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]{8}", helper)] == [R.ROW0_DWORD, 0x00FE0002, 0x00FF02FF]
    addend = src[src.index("mfma_i32x4 ycocg_addend()"):]
    assert "{%d, 2 + 512, 2 + 512, 0}" % R.ROW0_ADDEND in addend[: addend.index("return c;")]


def test_row_0_for_every_rgb():
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rng = np.random.default_rng(0x14)
    junk = set()
    for r in range(256):
        px = np.empty((256, 256, 4), dtype=np.uint8)
        px[..., 0], px[..., 1], px[..., 2] = r, g, b
        px[..., 3] = rng.integers(0, 256, (256, 256), dtype=np.uint8)           # alpha's weight is 0
        s = px[..., 0].astype(np.int64) + 2 * px[..., 1].astype(np.int64) + px[..., 2].astype(np.int64) + 2
        y, f = s >> 2, s & 3
        row = R.row0(px)
        assert np.array_equal(row, 256 * (255 - y) + 64 * (3 - f)), r
        assert row.min() >= 0 and row.max() <= 65535, r
        assert np.array_equal(row >> 8, 255 - y) and np.array_equal(row & 0xFF00, 256 * (255 - y)), r
        junk |= set(np.unique(row & 0xFF).tolist())
    assert junk == set(JUNK)


def test_two_instruction_field_is_the_three_instruction_field_for_every_range_offset_and_value():
    seen = 0
    for d in range(1, 256):
        a1 = np.arange(0, 256 - d, dtype=np.int64)[:, None]                     # min Y
        y = a1 + np.arange(0, d + 1, dtype=np.int64)[None, :]                   # every value a1..a1 + d
        a0 = a1 + d
        m = (1 << 19) // d + 1
        r = ((14 * (a0 - y) + max(d - 6, 0)) * m) >> 20                         # the definition's position
        assert r.min() == 0 and r.max() == 7
        old = R.old_field(y - 128, a0 - 128, np.int64(d))
        assert np.array_equal(old, (r + 1) & 7), d
        lo = 256 * (255 - a0)                                                   # the smallest row value, byte 0 dropped
        assert 28 * m < (1 << 24)
        for junk in JUNK:
            new = R.new_field(256 * (255 - y) + junk, lo, np.int64(d))
            assert np.array_equal(new, old), (d, junk)
        seen += y.size
    assert seen == sum((256 - d) * (d + 1) for d in range(1, 256))


def every_range_picture():
    """RGBA [4 n, 4, 4] (a column of blocks): for every d, a1 the values a1..a1 + d fourteen a block between the two
    ends; f cycles through 0..3 and the channels are unequal."""
    ys = []
    for d in range(1, 256):
        a1 = np.arange(0, 256 - d, dtype=np.int64)
        inner = np.arange(0, d + 1, dtype=np.int64)
        inner = np.resize(inner, -(-inner.size // 14) * 14).reshape(-1, 14)    # (the last block repeats the first values)
        blk = np.empty((a1.size, len(inner), 16), dtype=np.int64)
        blk[..., 1:15] = a1[:, None, None] + inner[None]
        blk[..., 0], blk[..., 15] = a1[:, None] + d, a1[:, None]
        ys.append(blk.reshape(-1, 16))
    y = np.concatenate(ys)
    idx = np.arange(y.size, dtype=np.int64).reshape(y.shape)
    r, g, b = R.rgb_with(y, idx % 4, idx // 4)
    blocks = np.stack([r, g, b, np.full_like(r, 255)], axis=-1).astype(np.uint8)                # [n, 16, 4]
    return np.ascontiguousarray(blocks.reshape(-1, 4, 4, 4).reshape(-1, 4, 4)), blocks


def test_both_block_forms_write_the_oracles_luma_bytes():
    img, blocks = every_range_picture()
    want = I.le(np.frombuffer(D.oracle_bc_encode(img, L.FMT_YCOCG), dtype=np.uint8).reshape(len(blocks), 16)[:, :8], 8)[:, 0]
    row = R.row0(blocks)
    assert set(np.unique(row & 0xFF).tolist()) == set(JUNK)
    px = blocks.astype(np.int64)
    y = (px[..., 0] + 2 * px[..., 1] + px[..., 2] + 2) >> 2
    assert np.array_equal(I.alpha_block_model(y - 128, 128), want)
    got = R.luma_block_negated_model(row)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), y[bad[0]].tolist())

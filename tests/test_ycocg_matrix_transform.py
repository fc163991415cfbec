"""The YCoCg transform as one 4x4x4 signed-byte matrix product a pixel (hap_amd/csrc/bc_encode_core.hpp, block_of<FMT, true>),
restated in numpy and compared with the definition over its WHOLE input domain, then pinned against oracle/bc_oracle.c
-- the definition -- not against the kernel.  CPU only.

The form: q = p ^ 0x80808080 read as four signed bytes (R', G', B', A' = channel - 128); three weight rows, signed
bytes too, accumulator 2 for every row:

    row 0:  1,  2,  1, 0   -> R + 2G + B + 2 - 512      >> 2  =  Y - 128
    row 1:  2,  0, -2, 0   -> 2 (R - B + 1)             >> 2  =  Co - 128
    row 2: -1,  2, -1, 0   -> -R + 2G - B + 2           >> 2  =  Cg - 128

Y by an arithmetic shift of the 32-bit sum; Co and Cg by packing the LOW HALVES of their sums side by side
(v_perm_b32) and one packed arithmetic shift of both 16-bit halves by 2 (v_pk_ashrrev_i16).  The alpha byte's weight is
zero in every row.
"""
import os
import re

import numpy as np

import _data as D
import _libs as L
import _value_space as V
import test_block_math_identities as B

ROW_DWORDS = (0x00010201, 0x00FE0002, 0x00FF02FF)          # as the kernel holds them: byte k = weight of channel k
ROWS = np.array([[1, 2, 1, 0], [2, 0, -2, 0], [-1, 2, -1, 0]], dtype=np.int64)
ACC = 2


def signed16(x):
    return ((x & 0xFFFF) ^ 0x8000) - 0x8000


def matrix_form(px):
    """px: uint8 [..., 4] -> (Y - 128, Co - 128, Cg - 128), int64, by the kernel's steps."""
    q = (np.asarray(px, dtype=np.uint8) ^ 0x80).view(np.int8).astype(np.int64)           # signed bytes of p ^ 0x80808080
    d = q @ ROWS.T + ACC                                                                # the matrix product, 32-bit sums
    assert int(np.abs(d).max()) < (1 << 15)                                             # (the low halves hold them whole)
    y = d[..., 0] >> 2
    packed = (d[..., 1] & 0xFFFF) | ((d[..., 2] & 0xFFFF) << 16)                          # v_perm_b32, selector 0x05040100
    co = signed16(packed) >> 2                                                          # v_pk_ashrrev_i16 by {2, 2}
    cg = signed16(packed >> 16) >> 2
    return y, co, cg


def definition(px):
    r, g, b = (np.asarray(px, dtype=np.int64)[..., c] for c in range(3))
    return (r + 2 * g + b + 2) >> 2, ((r - b + 1) >> 1) + 128, ((-r + 2 * g - b + 2) >> 2) + 128


def test_the_weight_dwords_are_the_rows_and_the_source_holds_them():
    for dword, row in zip(ROW_DWORDS, ROWS):
        assert np.array_equal(np.array([dword], dtype="<u4").view(np.int8).astype(np.int64), row)
    src = open(os.path.join(os.path.dirname(__file__), "..", "hap_amd", "csrc", "bc_encode_core.hpp")).read()
    helper = src[src.index("unsigned ycocg_weight_rows()"):]
    helper = helper[: helper.index("return r;")]
    assert [int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]{8}", helper)] == list(ROW_DWORDS)
    for operand in ("%[qa]", "%[qb]"):                                                   # the accumulator: the inline constant
        assert src.count("%%[w], %s, %d\\n" % (operand, ACC)) == 2, operand


def test_every_rgb_with_three_alphas():
    """all 2^24 (R, G, B), with alpha 0, 255 and a seeded random byte: 3 x 16 777 216 pixels"""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rng = np.random.default_rng(0x4C4)
    seen = 0
    for r in range(256):
        px = np.empty((256, 256, 4), dtype=np.uint8)
        px[..., 0], px[..., 1], px[..., 2] = r, g, b
        want_y, want_co, want_cg = definition(px)
        for alpha in (0, 255, None):
            px[..., 3] = rng.integers(0, 256, (256, 256), dtype=np.uint8) if alpha is None else alpha
            y, co, cg = matrix_form(px)
            assert np.array_equal(y + 128, want_y), (r, alpha)
            assert np.array_equal(co + 128, want_co), (r, alpha)
            assert np.array_equal(cg + 128, want_cg), (r, alpha)
            seen += y.size
    assert seen == 3 << 24


def test_the_ranges_the_kernel_counts_on():
    corners = np.array([[r, g, b, a] for r in (0, 255) for g in (0, 255) for b in (0, 255) for a in (0, 255)], dtype=np.uint8)
    y, co, cg = matrix_form(corners)
    assert (y.min(), y.max()) == (-128, 127)
    assert (co.min(), co.max()) == (-127, 128) and (cg.min(), cg.max()) == (-127, 128)
    only = np.array([[255, g, 0, 0] for g in range(256)], dtype=np.uint8)                 # Co - 128 = +128: R 255, B 0 alone
    assert (matrix_form(only)[1] == 128).all()


EXTREMES = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255],
                     [255, 0, 255]], dtype=np.uint8)


def pinned_blocks(noise=4096, seed=0x10C0C6):
    """uint8 [n, 16, 4]: every ordered pair of the eight corner colours (the saturated primaries among them), the second
    at each texel position in turn; seeded noise; seeded noise near one colour (small chroma: scales 2 and 4)."""
    rng = np.random.default_rng(seed)
    corners = np.zeros((64 * 16, 16, 4), dtype=np.uint8)
    for i in range(8):
        for j in range(8):
            for k in range(16):
                corners[(i * 8 + j) * 16 + k, :, :3] = EXTREMES[i]
                corners[(i * 8 + j) * 16 + k, k, :3] = EXTREMES[j]
    corners[..., 3] = rng.integers(0, 256, corners.shape[:2])
    rnd = rng.integers(0, 256, (noise, 16, 4)).astype(np.uint8)
    near = (rng.integers(0, 256, (noise, 1, 4)) + rng.integers(-24, 25, (noise, 16, 4))).clip(0, 255).astype(np.uint8)
    return np.concatenate([corners, rnd, near])


def test_against_the_oracle():
    px = pinned_blocks()
    img = V.picture_of_blocks(px)
    px = V.blocks_of_picture(img)                                                        # (with the padding blocks)
    blocks = np.frombuffer(D.oracle_bc_encode(img, L.FMT_YCOCG), dtype=np.uint8).reshape(-1, 16).astype(np.int64)
    y, co, cg = matrix_form(px)
    assert (co == 128).any() and (co == -127).any() and (cg == 128).any() and (cg == -127).any()
    # luma half: a0, a1 and the ramp codes of the oracle's alpha-style block, from the matrix form's Y
    a = y + 128
    a0, a1 = a.max(axis=1), a.min(axis=1)
    assert np.array_equal(blocks[:, 0], a0) and np.array_equal(blocks[:, 1], a1)
    d = a0 - a1
    dd = np.maximum(d, 1)
    m = (1 << 19) // dd + 1
    start = a0 * 14 * m + np.maximum(d - 6, 0) * m + (1 << 20)
    f = ((start[:, None] - a * (14 * m)[:, None]) >> 20) & 7
    lo24 = sum(f[:, k] << (3 * k) for k in range(8))
    hi24 = sum(f[:, 8 + k] << (3 * k) for k in range(8))
    bits = np.where(d > 0, B.ramp_codes(lo24) | (B.ramp_codes(hi24) << 24), 0)
    assert np.array_equal(bits, sum(blocks[:, 2 + k] << (8 * k) for k in range(6)))
    # colour half: the oracle's scaled YCoCg block from the matrix form's Co, Cg
    c0, c1, idx = B._hapq_model_new(co + 128, cg + 128)
    w = blocks[:, 8:]
    assert np.array_equal(w[:, 0] | w[:, 1] << 8, c0) and np.array_equal(w[:, 2] | w[:, 3] << 8, c1)
    assert np.array_equal(w[:, 4] | w[:, 5] << 8 | w[:, 6] << 16 | w[:, 7] << 24, sum(idx[:, k] << (2 * k) for k in range(16)))

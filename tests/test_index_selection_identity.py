"""The index selection and the centred transform of the block encoder (hap_amd/csrc/bc_encode_core.hpp), restated in
numpy next to what they replaced and compared over their whole domains, then pinned to oracle/bc_oracle.c -- the
definition -- not to the kernel.  CPU only.

  1. position of a pixel on the segment.  Was: pos = clamp((t m24) >> 24, 0, 3), the projection t not clamped first.
     Now: tc = clamp(t, 0, top) as the definition states it, v = tc (m24 << 6) in 32 bits, pos = v >> 30, gathered with
     pos2 = pos2 << 2 | pos from the last pixel to the first.  Domain: every len2 the byte channels can give, 16 ..
     3 x 255^2 = 195075, with m24 = floor(3 x 2^24 / len2) and top = len2 + len2 / 6 as index_scale / make_projection
     define them: the product never wraps (top m24 < 2^26), a pixel at or beyond top has position 3
     (top m24 >= 3 x 2^24), and old == new at the edges of the clamp and at 64 seeded t per len2.
  2. Y, Co, Cg less 128.  Was: three unsigned byte dot products with the complements of the negative channels, shifted
     as unsigned values, 128 subtracted downstream where needed.  Now: Y's accumulator starts at 2 - 512 (wrap-around) and
     is shifted arithmetically; Co and Cg are signed byte dot products of the bytes less 128 (xor 0x80 per byte) with
     the weights (1, 0, -1) and (-1, 2, -1) and the accumulators 1 and 2, the low halves packed and shifted
     arithmetically as 16-bit values.  Domain: all 2^24 RGB values.
  3. the three block functions as they now stand -- alpha_block on values less a bias, colour_block through the new
     project4, ycocg_colour_block on the centred pair with the scale in the direction and K' = len2 / 6 + sum of
     dir (128 - p1) -- in the kernel's own wrap-around arithmetic, against the oracle's bytes for DXT1, RGTC1, DXT5 and
     scaled YCoCg-DXT5: 100 000 seeded blocks per format (half uniform, half near one colour, which is where the
     scales 2 and 4 and the short segments live), and the blocks of the pictures the suite already has
     (tests/_value_space.ENCODE_PICTURES, tests/_data.quality_images(); tests/golden holds no picture files).
"""
import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V

M32 = 0xFFFFFFFF
LEN2_MAX = 3 * 255 * 255


# ---- 1. the position ----
def old_position(t, m24):
    return np.clip((t * m24) >> 24, 0, 3)


def new_position(t, m24, top):
    tc = np.clip(t, 0, top)
    return ((tc * (m24 << 6)) & M32) >> 30


def test_scaled_product_gives_the_old_position_for_every_len2():
    len2 = np.arange(16, LEN2_MAX + 1, dtype=np.int64)
    m24 = 50331648 // len2
    top = len2 + len2 // 6
    assert np.all(top * m24 < (1 << 26))                      # v = tc (m24 << 6) stays inside 32 bits
    assert np.all(top * m24 >= 3 << 24)                       # a pixel clamped to top still has position 3
    rng = np.random.default_rng(0x1D5E1)
    fixed = [np.full_like(len2, -(1 << 20)), np.full_like(len2, -1), np.zeros_like(len2), np.ones_like(len2),
             top - 1, top, top + 1, np.full_like(len2, 1 << 20)]
    # 64 seeded values per len2: from half a segment below p1 to half a segment beyond the clamp
    seeded = (rng.random((64, len2.size)) * (2 * top + 2)[None, :]).astype(np.int64) - (top // 2)[None, :]
    for t in fixed + list(seeded):
        old, new = old_position(t, m24), new_position(t, m24, top)
        assert np.array_equal(old, new), int(len2[np.argmax(old != new)])
    assert np.all(new_position(top, m24, top) == 3) and np.all(new_position(top + 1, m24, top) == 3)


def gather_from_the_top(pos):
    """pos int [n, 16] -> the dword after pos2 = pos2 << 2 | pos over the pixels 15 .. 0 (32-bit)."""
    pos2 = np.zeros(len(pos), dtype=np.int64)
    for i in range(15, -1, -1):
        pos2 = ((pos2 << 2) | pos[:, i]) & M32
    return pos2


def indices_of_positions(pos2):
    hi = pos2 & 0xAAAAAAAA
    return (hi ^ ((pos2 << 1) & 0xAAAAAAAA)) | (((~hi & M32) >> 1) & 0x55555555)


def test_reversed_gather_puts_pixel_0_lowest():
    rng = np.random.default_rng(0x6A7)
    pos = rng.integers(0, 4, (4096, 16)).astype(np.int64)
    pos[0] = np.arange(16) % 4
    pos[1] = np.array([0, 1, 2, 3, 3, 1, 0, 2, 1, 1, 3, 0, 2, 3, 0, 1])                   # no palindrome
    want = sum(np.array([1, 3, 2, 0])[pos[:, k]] << (2 * k) for k in range(16))
    assert np.array_equal(indices_of_positions(gather_from_the_top(pos)), want)


# ---- 2. the centred transform ----
def s32(x):
    x = x & M32
    return np.where(x >= 1 << 31, x - (1 << 32), x)


def s16(x):
    x = x & 0xFFFF
    return np.where(x >= 1 << 15, x - (1 << 16), x)


def centred_transform(r, g, b):
    """As block_of forms them: (Y - 128, Co - 128, Cg - 128) of int64 byte values."""
    y = s32(r + 2 * g + b + ((2 - 512) & M32)) >> 2                                        # v_dot4_u32_u8, v_ashrrev_i32
    sb = lambda v: (v ^ 0x80) - 2 * ((v ^ 0x80) & 0x80)                                    # the byte v ^ 0x80 read as a signed byte
    co2 = s32(sb(r) - sb(b) + 1)                                                           # v_dot4_i32_i8, weights 1, 0, -1
    cg4 = s32(-sb(r) + 2 * sb(g) - sb(b) + 2)                                              # weights -1, 2, -1
    return y, s16(co2) >> 1, s16(cg4) >> 2                                                 # v_perm_b32, v_pk_ashrrev_i16


def test_centred_transform_is_the_current_one_less_128_for_every_rgb():
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for r in range(256):
        rr = np.full_like(g, r)
        y = (rr + 2 * g + b + 2) >> 2                                                      # the current ones: 0..255, 1..256
        co, cg = V.ycocg(np.stack([rr, g, b], axis=-1))
        cy, cco, ccg = centred_transform(rr, g, b)
        assert np.array_equal(cy, y - 128) and np.array_equal(cco, co - 128) and np.array_equal(ccg, cg - 128), r
        assert cy.min() >= -128 and cy.max() <= 127 and cco.min() >= -127 and cco.max() <= 128


# ---- 3. the block functions as they stand, against the oracle ----
def alpha_block_model(a, bias):
    """alpha_block<BIAS> on a = values less bias, int64 [n, 16] -> the block's 8 bytes as one integer each."""
    a0, a1 = a.max(axis=1), a.min(axis=1)
    d = a0 - a1
    m = (1 << 19) // np.maximum(d, 1) + 1
    start = a0 * 14 * m + np.maximum(d - 6, 0) * m + (1 << 20)
    f = (s32(start[:, None] - a * (14 * m)[:, None]) >> 20) & 7
    ramp = lambda w: w ^ (~((w >> 1) | (w >> 2)) & 0x249249)
    lo24 = ramp(sum(f[:, k] << (3 * k) for k in range(8)))
    hi24 = ramp(sum(f[:, 8 + k] << (3 * k) for k in range(8)))
    bits = np.where(d > 0, lo24 | (hi24 << 24), 0)
    return ((a0 + (a1 << 8) + bias * 257) & M32) | (bits << 16)


def positions_model(t, m24, top):
    """gather_indices: t int64 [n, 16] (the dot products with their accumulators), per-block m24 and top."""
    assert int(np.abs(t).max(initial=0)) < (1 << 31)
    return indices_of_positions(gather_from_the_top(new_position(t, m24[:, None], top[:, None])))


def colour_block_new(px, raw=False):
    """colour_block / make_projection / project4: px int64 [n, 16, 3] -> (c0 | c1 << 16, index dword); raw: the
    projections before the clamp, their upper bound and which blocks are flat (for tests that build pictures)."""
    mdl = V.colour_block_model(px)                                 # the end points (not touched here)
    c0, c1 = mdl["c0"], mdl["c1"]
    p0 = np.stack([V.E5[c0 >> 11], V.E6[(c0 >> 5) & 63], V.E5[c0 & 31]], axis=-1)
    p1 = np.stack([V.E5[c1 >> 11], V.E6[(c1 >> 5) & 63], V.E5[c1 & 31]], axis=-1)
    dirv = p0 - p1
    adir, flip = np.abs(dirv), np.where(dirv < 0, 0xFF, 0)
    len2 = (adir * adir).sum(axis=1)
    sixth = len2 // 6
    start = sixth - (p1 * dirv).sum(axis=1) - 255 * np.where(dirv < 0, adir, 0).sum(axis=1)
    t = ((px ^ flip[:, None, :]) * adir[:, None, :]).sum(axis=-1) + start[:, None]       # v_dot4_u32_u8
    idx = positions_model(t, 50331648 // np.maximum(len2, 1), len2 + sixth)
    if raw:
        return {"t": t, "top": len2 + sixth, "flat": c0 == c1, "m24": 50331648 // np.maximum(len2, 1)}
    return c0 | (c1 << 16), np.where(c0 != c1, idx, 0)


def ycocg_colour_block_new(co, cg, raw=False):
    """ycocg_colour_block on the centred pair: co, cg int64 [n, 16] (-127..128) -> (c0 | c1 << 16, index dword); raw as
    in colour_block_new, with the scale."""
    lo_o, hi_o, lo_g, hi_g = co.min(axis=1), co.max(axis=1), cg.min(axis=1), cg.max(axis=1)
    m = np.maximum(np.maximum(-lo_o, hi_o), np.maximum(-lo_g, hi_g))
    s = np.where(m <= 31, 4, np.where(m <= 63, 2, 1))
    prod, sum_o, sum_g = (co * cg).sum(axis=1), co.sum(axis=1), cg.sum(axis=1)
    assert np.abs(sum_o).max() < (1 << 15) and np.abs(sum_g).max() < (1 << 15)            # v_pk_add_i16 holds them
    mo, mg = lo_o + hi_o, lo_g + hi_g
    cov = 4 * prod - 2 * mg * sum_o - 2 * mo * sum_g + 16 * mo * mg
    lo_o, hi_o, lo_g, hi_g = lo_o * s + 128, hi_o * s + 128, lo_g * s + 128, hi_g * s + 128
    ins = (hi_o - lo_o) >> 4
    lo_o, hi_o = lo_o + ins, hi_o - ins
    ins = (hi_g - lo_g) >> 4
    lo_g, hi_g = lo_g + ins, hi_g - ins
    ag, bg = np.where(cov < 0, lo_g, hi_g), np.where(cov < 0, hi_g, lo_g)
    qo_a, qo_b, qg_a, qg_b = V.quant5(hi_o), V.quant5(lo_o), V.quant6(ag), V.quant6(bg)
    qa, qb = qo_a << 11 | qg_a << 5 | (s - 1), qo_b << 11 | qg_b << 5 | (s - 1)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    sw = qa < qb
    eo_a, eo_b, eg_a, eg_b = V.E5[qo_a], V.E5[qo_b], V.E6[qg_a], V.E6[qg_b]
    d_o, d_g = np.where(sw, eo_b - eo_a, eo_a - eo_b), np.where(sw, eg_b - eg_a, eg_a - eg_b)
    p1_o, p1_g = np.where(sw, eo_a, eo_b), np.where(sw, eg_a, eg_b)
    len2 = d_o * d_o + d_g * d_g
    sixth = len2 // 6
    K = d_o * (128 - p1_o) + d_g * (128 - p1_g) + sixth
    ds_o, ds_g = d_o * s, d_g * s
    assert np.abs(ds_o).max() <= 1020 and np.abs(ds_g).max() <= 1020                      # the 16-bit direction holds the scale
    t = co * ds_o[:, None] + cg * ds_g[:, None] + K[:, None]                              # v_dot2_i32_i16
    idx = positions_model(t, 50331648 // np.maximum(len2, 1), len2 + sixth)
    if raw:
        return {"t": t, "top": len2 + sixth, "flat": c0 == c1, "m24": 50331648 // np.maximum(len2, 1), "scale": s}
    return c0 | (c1 << 16), np.where(c0 != c1, idx, 0)


def le(words, n):
    """oracle bytes uint8 [blocks, 8 k] -> little-endian integers of n bytes each, [blocks, k]."""
    w = words.astype(np.int64).reshape(len(words), -1, n)
    return sum(w[..., k] << (8 * k) for k in range(n))


def check_picture(img, fmt, what):
    px = V.blocks_of_picture(img).astype(np.int64)
    got = np.frombuffer(D.oracle_bc_encode(img, fmt), dtype=np.uint8).reshape(len(px), -1)
    if fmt == L.FMT_RGTC1:
        assert np.array_equal(le(got, 8)[:, 0], alpha_block_model(px[..., 3], 0)), what
        return
    if fmt == L.FMT_DXT1:
        ends, idx = colour_block_new(px[..., :3])
        colour = got
    elif fmt == L.FMT_DXT5:
        assert np.array_equal(le(got[:, :8], 8)[:, 0], alpha_block_model(px[..., 3], 0)), what
        ends, idx = colour_block_new(px[..., :3])
        colour = got[:, 8:]
    else:
        y, co, cg = centred_transform(px[..., 0], px[..., 1], px[..., 2])
        assert np.array_equal(le(got[:, :8], 8)[:, 0], alpha_block_model(y, 128)), what
        ends, idx = ycocg_colour_block_new(co, cg)
        colour = got[:, 8:]
    w = le(colour, 4)
    assert np.array_equal(w[:, 0], ends), what
    assert np.array_equal(w[:, 1], idx), what


FORMATS = [pytest.param(L.FMT_DXT1, id="dxt1"), pytest.param(L.FMT_RGTC1, id="rgtc1"), pytest.param(L.FMT_DXT5, id="dxt5"),
           pytest.param(L.FMT_YCOCG, id="ycocg")]


@pytest.fixture(scope="module")
def seeded_picture():
    """100 000 blocks: 50 000 uniform, 50 000 within +-24 of one colour."""
    rng = np.random.default_rng(0x1DE9)
    rnd = rng.integers(0, 256, (50000, 16, 4))
    near = (rng.integers(0, 256, (50000, 1, 4)) + rng.integers(-24, 25, (50000, 16, 4))).clip(0, 255)
    blocks = np.concatenate([rnd, near]).astype(np.uint8)
    assert len(blocks) == 100000
    return V.picture_of_blocks(blocks, row=250)


@pytest.mark.parametrize("fmt", FORMATS)
def test_block_functions_against_the_oracle_on_seeded_blocks(seeded_picture, fmt):
    check_picture(seeded_picture, fmt, "seeded")


@pytest.fixture(scope="module")
def suite_pictures():
    pics = {name: make() for name, make in V.ENCODE_PICTURES.items()}
    pics.update(D.quality_images())
    return pics


@pytest.mark.parametrize("fmt", FORMATS)
def test_block_functions_against_the_oracle_on_the_suites_pictures(suite_pictures, fmt):
    for name, img in suite_pictures.items():
        check_picture(np.ascontiguousarray(img), fmt, name)

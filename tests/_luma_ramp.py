"""Inputs and the numpy restatement for the fused Hap Q kernel's luma half (hap_amd/csrc/bc_encode_core.hpp:
ycocg_weight_rows_biased, ycocg_addend, luma_block_negated).  Row 0 of the matrix product delivers
256 (255 - Y) + 64 (3 - f), S = R + 2G + B + 2 = 4Y + f, and the ramp takes it in two instructions a pixel,
v_mad_u32_u24 and v_alignbit_b32 by 29.  Shared by tests/test_luma_row_identity.py (CPU) and
tests/test_luma_ramp_top_bits_gpu.py; no GPU needed here."""
import numpy as np

M24, M32 = 0xFFFFFF, 0xFFFFFFFF
ROW0_DWORD, ROW0, ROW0_ADDEND = 0x00C080C0, np.array([-64, -128, -64, 0], dtype=np.int64), 32576


def row0(px):
    """px: uint8 [..., 4] -> what the matrix instruction leaves in row 0: signed-byte products plus the addend."""
    q = (np.asarray(px, dtype=np.uint8) ^ 0x80).view(np.int8).astype(np.int64)
    return q @ ROW0 + ROW0_ADDEND


def mad_u32_u24(a, b, c):
    """v_mad_u32_u24: the low 24 bits of a and b, the low 32 bits of a b + c."""
    return ((a & M24) * (b & M24) + c) & M32


def s24(x):
    x = x & M24
    return np.where(x >= 1 << 23, x - (1 << 24), x)


def old_field(a, a0, d):
    """alpha_block<128>'s three instructions a pixel on a = Y - 128: v_mad_i32_i24, v_lshrrev_b32 by 20 and the three
    bits v_alignbit_b32 by 3 takes: (r + 1) mod 8."""
    m = (1 << 19) // d + 1
    neg_m14 = -14 * m
    start = (s24(a0) * s24(14 * m) + np.maximum(d - 6, 0) * m + (1 << 20)) & M32
    assert np.all(s24(a) == a) and np.all(s24(neg_m14) == neg_m14)            # the operands fit 24 bits signed
    x = (s24(a) * s24(neg_m14) + start) & M32
    return (x >> 20) & 7


def new_constants(lo, d):
    """Per block: 28 m and start << 9 modulo 2^32 from lo = 256 min(255 - Y) and d, on the 24-bit multiplier."""
    m1 = (1 << 19) // d                                                        # floor(2^19 / d) = m - 1
    m28 = mad_u32_u24(m1, 28, 28)
    d6 = np.maximum(d - 6, 0)
    start9 = (((mad_u32_u24(d6, m1, d6) << 9) & M32) + (1 << 29) - mad_u32_u24(lo, m28, 0)) & M32
    return m28, start9


def new_field(raw, lo, d):
    """The two instructions a pixel on the row's value as it comes (junk in byte 0): v_and_b32 with 0xFF00 (the
    transform's), v_mad_u32_u24, and the three bits v_alignbit_b32 by 29 takes from the top."""
    m28, start9 = new_constants(lo, d)
    return mad_u32_u24(raw & 0xFF00, m28, start9) >> 29


def ramp_codes(w):
    return w ^ (~((w >> 1) | (w >> 2)) & 0x249249)


def luma_block_negated_model(raw):
    """luma_block_negated on the row's values, int64 [n, 16] -> the block's 8 luma bytes as one integer each."""
    v = raw & 0xFF00
    lo, hi = v.min(axis=1), v.max(axis=1)
    d = (hi - lo) >> 8
    m28, start9 = new_constants(lo, np.maximum(d, 1))
    words = []
    for base in (0, 8):
        acc = np.zeros(len(v), dtype=np.int64)
        for i in range(7, -1, -1):                                             # from the last pixel to the first
            x9 = mad_u32_u24(v[:, base + i], m28, start9)
            acc = ((acc << 3) | (x9 >> 29)) & M32                               # v_alignbit_b32(acc, x9, 29)
        words.append(ramp_codes(acc))
    assert all(int(w.max(initial=0)) < (1 << 24) for w in words)
    bits = np.where(d > 0, words[0] | (words[1] << 24), 0)
    return (((lo >> 8) | hi) ^ 0xFFFF) | (bits << 16)


def rgb_with(y, f, k):
    """int64 arrays Y (0..255), f (0..3), k (any) -> R, G, B with R + 2G + B + 2 = 4Y + f where such bytes exist (Y = 0
    has f >= 2 only and Y = 255 f <= 2: f is moved to the nearest that exists), unequal channels chosen by k."""
    y, f, k = np.broadcast_arrays(np.asarray(y, dtype=np.int64), np.asarray(f, dtype=np.int64), np.asarray(k, dtype=np.int64))
    f = np.where(y == 0, np.maximum(f, 2), np.where(y == 255, np.minimum(f, 2), f))
    t = 4 * y + f - 2                                                          # R + 2G + B, 0..1020
    g = np.clip(t // 4 + (k % 7 - 3) * 9, 0, 255)
    g = np.clip(g, (t - 510 + 1) // 2, t // 2)                                 # R + B = t - 2G in 0..510
    rest = t - 2 * g
    r = np.clip(rest // 2 + (k % 5 - 2) * 17, np.maximum(rest - 255, 0), np.minimum(rest, 255))
    b = rest - r
    for c in (r, g, b):
        assert c.min() >= 0 and c.max() <= 255
    assert np.array_equal((r + 2 * g + b + 2) >> 2, y) and np.array_equal((r + 2 * g + b + 2) & 3, f)
    return r, g, b


def rgb_flat(y, f):
    """R, G, B with R + 2G + B + 2 = 4Y + f, Co = 128 and Cg = 128 whatever Y and f are (R = B or B - 1, 2G within
    -2..1 of R + B); where the bytes run out, at the ends of the range, rgb_with's."""
    y, f = np.broadcast_arrays(np.asarray(y, dtype=np.int64), np.asarray(f, dtype=np.int64))
    f = np.where(y == 0, np.maximum(f, 2), np.where(y == 255, np.minimum(f, 2), f))
    t = 4 * y + f - 2
    q = (t + 2) // 2
    q = q - ((q ^ t) & 1)                                                      # R + B: t's parity, (t - 1) / 2 .. (t + 2) / 2
    r = q // 2
    b, g = q - r, (t - q) // 2
    ok = (r >= 0) & (b <= 255) & (g >= 0) & (g <= 255)
    fr, fg, fb = rgb_with(y, f, np.full_like(y, 17))
    r, g, b = np.where(ok, r, fr), np.where(ok, g, fg), np.where(ok, b, fb)
    assert np.array_equal((r + 2 * g + b + 2) >> 2, y) and np.array_equal((r + 2 * g + b + 2) & 3, f)
    co, cg = ((r - b + 1) >> 1) + 128, ((-r + 2 * g - b + 2) >> 2) + 128
    assert np.all((co == 128) & (cg == 128) | ~ok)
    return r, g, b


def ramp_picture():
    """256 x 256 RGBA, 4096 blocks: block (by, bx) has luma range d = 1 + (4 by + bx // 16) mod 255 at one of sixteen
    offsets (bx mod 16) spread over 0 .. 255 - d.  Its pixels lie on both ends and in between: a ramp over the block,
    u = j d / 15 for the j-th pixel of an order that turns with the block, and two seeded values; f = 0..3 a pixel from
    unequal R, G, B of the same Y.  Chroma: flat (Co = Cg = 128) in the left half, busy in the right."""
    by, bx = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    d = 1 + (4 * by + bx // 16) % 255
    assert set(np.unique(d)) == set(range(1, 256))
    a1 = ((bx % 16) * (255 - d)) // 15
    rng = np.random.default_rng(0x14A)
    j = (np.arange(16)[None, None, :] * 7 + (by + bx)[..., None]) % 16         # 7 is odd: every j once a block
    u = (j * d[..., None]) // 15
    for at in (3, 12):
        keep = (j[..., at] == 0) | (j[..., at] == 15)                          # (never one of the two ends)
        u[..., at] = np.where(keep, u[..., at], rng.integers(0, 1 << 30, (64, 64)) % (d + 1))
    assert np.all((u == 0).any(axis=-1) & (u == d[..., None]).any(axis=-1))   # both ends in every block
    y = a1[..., None] + u
    f = (np.arange(16)[None, None, :] + by[..., None] + 2 * bx[..., None]) % 4
    busy = np.broadcast_to((bx >= 32)[..., None], y.shape)
    r, g, b = rgb_flat(y, f)
    wr, wg, wb = rgb_with(y, f, rng.integers(0, 35, y.shape))
    r, g, b = np.where(busy, wr, r), np.where(busy, wg, g), np.where(busy, wb, b)
    blocks = np.stack([r, g, b, rng.integers(0, 256, r.shape)], axis=-1).astype(np.uint8)      # [64, 64, 16, 4]
    return np.ascontiguousarray(blocks.reshape(64, 64, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(256, 256, 4))


def small_picture(img):
    """64 x 68 of ramp_picture(): every fourth block row and the last, the sixteen block columns about the border of
    the two chroma halves -- 272 blocks, no whole number of 512-block fragments."""
    rows = list(range(0, 64, 4)) + [63]
    return np.ascontiguousarray(img.reshape(64, 4, 256, 4)[rows].reshape(68, 256, 4)[:, 96:160])

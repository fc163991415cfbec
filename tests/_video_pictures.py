"""What the video encode tests share: the definition of HapGpuCompressNV12's conversion in numpy, with the coefficient
table derived here from the standards' fractions, and makers of NV12 pictures whose pitches are larger than their width
and whose padding is poisoned.  No GPU, no library."""
from fractions import Fraction

import numpy as np

BT601, BT709 = 0, 1                                        # HapGpuYCbCrMatrix
LIMITED, FULL = 0, 1                                       # HapGpuYCbCrRange
ROWS = [(BT601, LIMITED), (BT601, FULL), (BT709, LIMITED), (BT709, FULL)]
NAMES = {(BT601, LIMITED): "601 limited", (BT601, FULL): "601 full", (BT709, LIMITED): "709 limited", (BT709, FULL): "709 full"}

KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}
EXTREMES = (0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 254, 255)
POISON = 0xE5                                              # (a luma of 229 and a chroma far from grey)


def exact(matrix, range_):
    """The exact rationals: (cy, crv, cbu, cgu, cgv), luma offset -- R = cy y' + crv v, G = cy y' - cgu u - cgv v,
    B = cy y' + cbu u"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    crv, cbu = 2 * (1 - kr), 2 * (1 - kb)
    cgu, cgv = cbu * kb / kg, crv * kr / kg
    luma, chroma = (Fraction(255, 219), Fraction(255, 224)) if range_ == LIMITED else (Fraction(1), Fraction(1))
    return (luma, crv * chroma, cbu * chroma, cgu * chroma, cgv * chroma), (16 if range_ == LIMITED else 0)


def nearest(q):
    """a positive fraction to the nearest integer (no coefficient is a tie)"""
    assert (2 * q).denominator != 1 or q.denominator == 1
    return int((2 * q.numerator + q.denominator) // (2 * q.denominator))


def coefficients(matrix, range_):
    """the definition's integers: the exact rationals times 65536, to nearest; and the luma offset"""
    k, offset = exact(matrix, range_)
    return tuple(nearest(v * 65536) for v in k), offset


def accumulators(y, cb, cr, matrix, range_):
    """(R, G, B) before the shift, as int64 arrays (broadcast over the inputs)"""
    (cy, crv, cbu, cgu, cgv), offset = coefficients(matrix, range_)
    l = cy * (np.asarray(y, dtype=np.int64) - offset)
    u, v = np.asarray(cb, dtype=np.int64) - 128, np.asarray(cr, dtype=np.int64) - 128
    return l + crv * v + 32768, l - cgu * u - cgv * v + 32768, l + cbu * u + 32768


def rgb_of(y, cb, cr, matrix, range_):
    """The definition per sample: three uint8 arrays"""
    return tuple(np.clip(a >> 16, 0, 255).astype(np.uint8) for a in accumulators(y, cb, cr, matrix, range_))


def rgba_of_nv12(y, uv, matrix, range_, coefficients_of=None, rounding=32768):
    """The RGBA8 picture (H, W, 4) of an NV12 picture: y (H, W) uint8, uv (H / 2, W) uint8 of interleaved Cb, Cr -- each
    pair replicated over its 2 x 2 luma samples.  (coefficients_of, rounding: for the deliberately wrong converters of
    the GPU tests.)"""
    y, uv = np.asarray(y), np.asarray(uv)
    h, w = y.shape
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and uv.shape == (h // 2, w) and h % 2 == 0 and w % 2 == 0
    cb = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)
    cr = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)
    (cy, crv, cbu, cgu, cgv), offset = (coefficients_of or coefficients)(matrix, range_)
    l = cy * (y.astype(np.int64) - offset)
    u, v = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    for c, a in enumerate((l + crv * v, l - cgu * u - cgv * v, l + cbu * u)):
        out[..., c] = np.clip((a + rounding) >> 16, 0, 255)
    return out


# --------------------------------------------------------------------------------------------------------- pictures --
def padded(plane, pitch, poison=POISON):
    """`plane` (rows, n) inside a (rows, pitch) array whose padding is `poison`: (the whole array, the view of the plane)"""
    rows, n = plane.shape
    assert pitch >= n
    whole = np.full((rows, pitch), poison, dtype=np.uint8)
    whole[:, :n] = plane
    return whole, whole[:, :n]


def random_nv12(w, h, seed):
    """uniform random bytes: (y (h, w), uv (h / 2, w))"""
    rng = np.random.default_rng([w, h, seed])
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


def extremes_nv12(w, h, seed=0):
    """the extremes of every range in every plane, every (Y, Cb, Cr) combination drawn with equal weight"""
    rng = np.random.default_rng([w, h, seed, 99])
    e = np.array(EXTREMES, dtype=np.uint8)
    return e[rng.integers(0, e.size, (h, w))], e[rng.integers(0, e.size, (h // 2, w))]


def smooth_nv12(w, h, seed):
    """slow ramps in every plane: blocks that repeat, frames that compress"""
    rows, cols = np.arange(h)[:, None], np.arange(w)[None, :]
    y = ((cols // 8) * 9 + (rows // 4) * 5 + 31 * seed + 16) % 220
    crow, pair = np.arange(h // 2)[:, None], np.arange(w // 2)[None, :]
    uv = np.empty((h // 2, w), dtype=np.uint8)
    uv[:, 0::2] = (96 + (pair // 8) * 7 + 3 * seed + 0 * crow) % 256
    uv[:, 1::2] = (160 - (crow // 4) * 11 + 5 * seed + 0 * pair) % 256
    return y.astype(np.uint8), uv


def distinct_chroma_nv12(w, h):
    """a flat grey luma under a chroma that differs in every pair and every chroma row: whichever pair a texel takes
    shows in its colour"""
    y = np.full((h, w), 128, dtype=np.uint8)
    rows, pairs = np.arange(h // 2)[:, None], np.arange(w // 2)[None, :]
    uv = np.empty((h // 2, w), dtype=np.uint8)
    uv[:, 0::2] = (37 * pairs + 101 * rows + 11) % 256
    uv[:, 1::2] = (59 * pairs + 83 * rows + 200) % 256
    return y, uv

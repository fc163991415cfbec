"""What the video decode tests share: the definition of HapGpuDecompressNV12's conversion in numpy -- an RGBA8 picture to
a Y plane and a plane of interleaved Cb, Cr pairs -- with the coefficient table derived here from the standards'
fractions.  The way there (NV12 -> RGBA8) is tests/_video_pictures.py's.  No GPU, no library."""
from fractions import Fraction

import numpy as np

from _video_pictures import BT601, BT709, LIMITED, FULL, ROWS, NAMES, KR_KB, nearest      # noqa: F401 (shared names)

# include/hap_gpu.h's table, as the issue states it: yr, yg, yb, cbr, cbg, ch, crg, crb, lo
TABLE = {
    (BT601, LIMITED): (16829, 33039, 6416, 9714, 19070, 28784, 24103, 4681, 16),
    (BT601, FULL): (19595, 38470, 7471, 11058, 21710, 32768, 27439, 5329, 0),
    (BT709, LIMITED): (11966, 40254, 4064, 6596, 22188, 28784, 26145, 2639, 16),
    (BT709, FULL): (13933, 46871, 4732, 7509, 25259, 32768, 29763, 3005, 0),
}


def exact(matrix, range_):
    """The exact rationals: ((yr, yg, yb), (cbr, cbg, ch), (ch, crg, crb)), lo -- Y = lo + yr R + yg G + yb B,
    Cb = 128 - cbr R - cbg G + ch B, Cr = 128 + ch R - crg G - crb B, R, G, B in 0 .. 255"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fraction(219, 255), Fraction(224, 255)) if range_ == LIMITED else (Fraction(1), Fraction(1))
    half = Fraction(1, 2) * sc
    return ((sy * kr, sy * kg, sy * kb), (half * kr / (1 - kb), half * kg / (1 - kb), half),
            (half, half * kg / (1 - kr), half * kb / (1 - kr))), (16 if range_ == LIMITED else 0)


def coefficients(matrix, range_):
    """the definition's integers (yr, yg, yb, cbr, cbg, ch, crg, crb) and lo: the exact rationals times 65536 to
    nearest, but one per row by subtraction, so that every row sums exactly"""
    ((ykr, _ykg, ykb), (cbr, _cbg, ch), (_ch, _crg, crb)), lo = exact(matrix, range_)
    sy = Fraction(219, 255) if range_ == LIMITED else Fraction(1)
    yr, yb = nearest(ykr * 65536), nearest(ykb * 65536)
    yg = nearest(sy * 65536) - yr - yb
    ch_i, cbr_i, crb_i = nearest(ch * 65536), nearest(cbr * 65536), nearest(crb * 65536)
    return (yr, yg, yb, cbr_i, ch_i - cbr_i, ch_i, ch_i - crb_i, crb_i), lo


def luma_accumulator(r, g, b, matrix, range_):
    """what is shifted right by 16 (int64 arrays, broadcast over the inputs)"""
    (yr, yg, yb, *_rest), _lo = coefficients(matrix, range_)
    r, g, b = (np.asarray(c, dtype=np.int64) for c in (r, g, b))
    return yr * r + yg * g + yb * b + 32768


def luma_of(r, g, b, matrix, range_):
    """Y of one texel: uint8 (no clamp is ever needed: asserted)"""
    _k, lo = coefficients(matrix, range_)
    y = lo + (luma_accumulator(r, g, b, matrix, range_) >> 16)
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def chroma_accumulators(rs, gs, bs, matrix, range_):
    """(Cb, Cr) before the shift by 18, of the sums of R, G, B over a pair's four texels (0 .. 1020 each)"""
    (_yr, _yg, _yb, cbr, cbg, ch, crg, crb), _lo = coefficients(matrix, range_)
    rs, gs, bs = (np.asarray(c, dtype=np.int64) for c in (rs, gs, bs))
    bias = (128 << 18) + (1 << 17)
    return -cbr * rs - cbg * gs + ch * bs + bias, ch * rs - crg * gs - crb * bs + bias


def chroma_of(rs, gs, bs, matrix, range_):
    """(Cb, Cr) of a pair, uint8, from the sums over its 2 x 2 texels"""
    return tuple(np.clip(a >> 18, 0, 255).astype(np.uint8) for a in chroma_accumulators(rs, gs, bs, matrix, range_))


def planes_of_rgba(d, matrix, range_):
    """The NV12 picture of an RGBA8 picture d (H, W, 4) uint8, H and W even: (y (H, W), uv (H / 2, W)) uint8, uv the
    interleaved Cb, Cr pairs.  Alpha is not looked at."""
    d = np.asarray(d)
    h, w = d.shape[:2]
    assert d.dtype == np.uint8 and d.shape[2] == 4 and h % 2 == 0 and w % 2 == 0
    y = luma_of(d[..., 0], d[..., 1], d[..., 2], matrix, range_)
    sums = d[..., :3].astype(np.int64).reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3))
    cb, cr = chroma_of(sums[..., 0], sums[..., 1], sums[..., 2], matrix, range_)
    uv = np.empty((h // 2, w), dtype=np.uint8)
    uv[:, 0::2], uv[:, 1::2] = cb, cr
    return y, uv


def exact_samples(r, g, b, matrix, range_):
    """the exact real (Y, Cb, Cr) of one colour as float64 (for the error bounds: every texel of a pair the same)"""
    (ky, kcb, kcr), lo = exact(matrix, range_)
    r, g, b = (np.asarray(c, dtype=np.float64) for c in (r, g, b))
    f = [[float(v) for v in row] for row in (ky, kcb, kcr)]
    return (lo + f[0][0] * r + f[0][1] * g + f[0][2] * b, 128 - f[1][0] * r - f[1][1] * g + f[1][2] * b,
            128 + f[2][0] * r - f[2][1] * g - f[2][2] * b)

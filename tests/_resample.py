"""The definition of the resized-crop calls (include/hap_gpu.h: HapGpuDecodeFramesPlanesResized) in numpy, in int64:
the taps of one axis and the bytes of a resized crop of an RGBA8 picture.  Nothing here knows the library."""
import numpy as np


def taps(o, c):
    """(i0, i1, w) of every element i = 0 .. o - 1 of an output axis of o elements over a crop axis of c texels"""
    i = np.arange(o, dtype=np.int64)
    num = np.maximum((2 * i + 1) * c - o, 0)
    i0 = np.minimum(num // (2 * o), c - 1)
    i1 = np.minimum(i0 + 1, c - 1)
    frac = num % (2 * o)
    w = (frac * 256 + o) // (2 * o)
    return i0, i1, w


def blend(p00, p01, p10, p11, wx, wy):
    """The byte of four taps (arrays of any one shape, or scalars)"""
    p00, p01, p10, p11, wx, wy = (np.asarray(a, dtype=np.int64) for a in (p00, p01, p10, p11, wx, wy))
    top = p00 * (256 - wx) + p01 * wx
    bot = p10 * (256 - wx) + p11 * wx
    return (top * (256 - wy) + bot * wy + 32768) >> 16


def resample(picture, crop, out_size):
    """picture [h, w, channels] uint8, crop (x, y, cw, ch) in its texels, out_size (ow, oh) -> [oh, ow, channels] uint8"""
    x, y, cw, ch = crop
    ow, oh = out_size
    assert cw >= 1 and ch >= 1 and x + cw <= picture.shape[1] and y + ch <= picture.shape[0]
    x0, x1, wx = taps(ow, cw)
    y0, y1, wy = taps(oh, ch)
    p = picture.astype(np.int64)
    rows0, rows1 = p[y + y0], p[y + y1]                       # [oh, w, channels]
    v = blend(rows0[:, x + x0], rows0[:, x + x1], rows1[:, x + x0], rows1[:, x + x1], wx[None, :, None], wy[:, None, None])
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)

"""Deterministic half-float pictures for the BC6H encoder: uint16 [h, w, 4] half bit patterns, built from integers only
(a half bit pattern of a positive value is monotonic in the value and 1024 patterns are one stop, so a linear ramp of
patterns is an exponential ramp of light).  Alpha is 1.0 (0x3C00) except in `specials`, where it is garbage: the encoder
ignores it."""
import numpy as np

ONE = 0x3C00
W, H = 512, 256


def _hash(x, y):
    h = (x * 0x9E3779B1 + y * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    return h


def _pack(r, g, b, a=None):
    a = np.full(r.shape, ONE, np.int64) if a is None else a
    return np.ascontiguousarray(np.stack([r, g, b, a], -1).astype(np.uint16))


def _sign_magnitude(s):
    """signed integers -> half bit patterns of sign and magnitude (|s| <= 0x7BFF)"""
    return np.where(s < 0, 0x8000 | -s, s)


def hdr_images():
    """name -> picture.  smooth: 2^-8 .. 2^5 (13 stops) along x in R, 11 stops along y in G, both in B; noisy: the same
    with position-hashed noise of +-64 patterns (+-1/16 stop); hard_edge: stripes of a dark (~0.01) and a bright (~100)
    colour with thin lines of ~1000; signed: ramps through zero to +-1.0 and beyond, with noise in B; specials: 16 x 16,
    every special pattern next to ordinary ones."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    r = 0x1C00 + (x * 13 * 1024) // (W - 1)
    g = 0x2000 + (y * 11 * 1024) // (H - 1)
    b = 0x1C00 + ((x + y) * 12 * 1024) // (W + H - 2)
    smooth = _pack(r, g, b)
    h = _hash(x, y)
    noisy = _pack(*[v + ((h >> (7 * c)) & 127) - 64 for c, v in enumerate((r, g, b))])
    stripe = (((x + 2 * y) >> 3) & 1) == 1
    dark, bright, line = (0x211F, 0x251F, 0x2D00), (0x5640, 0x5000, 0x4900), (0x63D0, 0x63D0, 0x63D0)
    edge = [np.where(stripe, bright[c], dark[c]) for c in range(3)]
    edge = [np.where((x % 37) == 0, line[c], e) for c, e in enumerate(edge)]
    hard_edge = _pack(*edge)
    sr = (x - W // 2) * 60
    sg = (y - H // 2) * 130
    sb = (x + y - (W + H) // 2) * 30 + ((h & 255) - 128)
    signed = _pack(_sign_magnitude(sr), _sign_magnitude(sg), _sign_magnitude(sb))
    return {"smooth": smooth, "noisy": noisy, "hard_edge": hard_edge, "signed": signed, "specials": specials()}


SPECIALS = (0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x8000, 0x0000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400,
            0x7BFF, 0xFBFF, 0x3C00, 0xBC00, 0x7BFE, 0x5640)


def specials():
    """16 x 16: +-Inf, NaNs, +-0, denormals, the largest finite values and ordinary ones, in solid blocks, in blocks that
    mix two of them and scattered; alpha is garbage"""
    y, x = np.mgrid[0:16, 0:16].astype(np.int64)
    n = len(SPECIALS)
    sp = np.array(SPECIALS, np.int64)
    blk = (y // 4) * 4 + x // 4
    h = _hash(x, y)
    solid = sp[blk % n]
    pair = np.where((x + y) & 1, sp[(blk * 3 + 1) % n], sp[(blk * 5 + 2) % n])
    scattered = sp[h % n]
    r = np.where(blk < 8, solid, np.where(blk < 12, pair, scattered))
    g = np.where(blk < 4, solid, np.where(blk < 12, sp[(blk + 7) % n], sp[(h >> 8) % n]))
    b = np.where(blk < 4, solid, np.where(blk < 8, 0x3555, sp[(h >> 16) % n]))
    return _pack(r, g, b, (h >> 3) & 0xFFFF)


def from_float16(img):
    """uint8 [h, w, 4] picture -> half picture of img / 255 by numpy's float16 cast"""
    return np.ascontiguousarray((img.astype(np.float32) / 255.0).astype(np.float16).view(np.uint16))

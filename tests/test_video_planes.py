"""The conversion of the video decode road (include/hap_gpu.h: HapGpuDecompressNV12) as tests/_video_planes.py defines it,
without a GPU or the library: the coefficients derived from the standards' fractions are the table the header prints and
the constants hap_amd/csrc/rgb_ycbcr.hpp holds; every row sums exactly, so greys, white and black come out as stated;
over all 2^24 colours with four equal texels every sample is within 0.5021 of the exact real value and the chroma
accumulators stay within 0 .. 2^26; and RGB -> this definition -> HapGpuCompressNV12's (tests/_video_pictures.rgb_of)
comes back within 1, 1, 2 (Limited) and 1, 1, 1 (Full)."""
import os
import re

import numpy as np
import pytest

import _video_pictures as V
import _video_planes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def colours():
    """all 2^24 (R, G, B), broadcastable"""
    return np.arange(256)[:, None, None], np.arange(256)[None, :, None], np.arange(256)[None, None, :]


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_the_derived_coefficients_are_the_tables(row):
    k, lo = P.coefficients(*row)
    assert k + (lo,) == P.TABLE[row]
    yr, yg, yb, cbr, cbg, ch, crg, crb = k
    # the row sums are exact
    sy = 219 * 65536 / 255 if row[1] == P.LIMITED else 65536
    assert yr + yg + yb == round(sy)
    assert cbr + cbg == ch == crg + crb
    assert ch == round((224 * 32768 / 255) if row[1] == P.LIMITED else 32768)
    for v in k:
        assert 0 < v < 2 ** 23                                  # (what lets the device multiply 24-bit factors)


def test_the_headers_hold_the_same_constants():
    text = open(os.path.join(ROOT, "hap_amd", "csrc", "rgb_ycbcr.hpp")).read()
    found = re.findall(r"sample_coefficients\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}\)*;?\s*// (BT601|BT709) (Limited|Full)", text)
    assert len(found) == 4, found
    matrices, ranges = {"BT601": P.BT601, "BT709": P.BT709}, {"Limited": P.LIMITED, "Full": P.FULL}
    assert {(matrices[m], ranges[r]): tuple(int(n) for n in numbers) for *numbers, m, r in found} == P.TABLE
    header = open(os.path.join(ROOT, "include", "hap_gpu.h")).read()
    for (matrix, range_), numbers in P.TABLE.items():
        name = r"%s\s+%s\s+" % ({P.BT601: "BT601", P.BT709: "BT709"}[matrix], {P.LIMITED: "Limited", P.FULL: "Full"}[range_])
        assert re.search(name + r"\s+".join(str(n) for n in numbers) + r"\n", header), (matrix, range_)


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_greys_white_and_black(row):
    grey = np.arange(256)
    cb, cr = P.chroma_of(4 * grey, 4 * grey, 4 * grey, *row)
    assert (cb == 128).all() and (cr == 128).all()
    y = P.luma_of(grey, grey, grey, *row)
    assert (int(y[0]), int(y[255])) == ((16, 235) if row[1] == P.LIMITED else (0, 255))
    assert (np.diff(y.astype(int)) >= 0).all()
    if row[1] == P.FULL:
        assert np.array_equal(y, grey)
    # four different texels with a grey sum are grey too: only the sums are looked at
    assert P.chroma_of(510, 510, 510, *row) == (128, 128)
    d = np.zeros((2, 2, 4), dtype=np.uint8)
    d[0, 0, :3], d[1, 1, :3], d[..., 3] = 255, 255, ((0, 1), (2, 255))
    yy, uv = P.planes_of_rgba(d, *row)
    assert uv.tolist() == [[128, 128]] and yy.tolist() == [[int(y[255]), int(y[0])], [int(y[0]), int(y[255])]]


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_every_colour_is_within_0_5021_and_comes_back(colours, row):
    """All 2^24 colours, four equal texels to a pair"""
    r, g, b = colours
    (_k, lo) = P.coefficients(*row)
    ey, ecb, ecr = P.exact_samples(r, g, b, *row)
    ya = P.luma_accumulator(r, g, b, *row)
    y = lo + (ya >> 16)
    ca, cra = P.chroma_accumulators(4 * r, 4 * g, 4 * b, *row)
    cb, cr = ca >> 18, cra >> 18
    worst = max(float(np.abs(y - ey).max()), float(np.abs(cb - ecb).max()), float(np.abs(cr - ecr).max()))
    print("%s: worst distance %.6f, chroma accumulators %d .. %d, luma accumulator up to %d"
          % (P.NAMES[row], worst, min(ca.min(), cra.min()), max(ca.max(), cra.max()), ya.max()))
    assert worst <= 0.5021
    assert y.min() >= 0 and y.max() <= 255 and ya.min() >= 0 and ya.max() < 2 ** 24        # no clamp is ever needed
    assert min(ca.min(), cra.min()) >= 0 and max(ca.max(), cra.max()) <= 2 ** 26
    # Full range reaches 256 before the clamp: the clamp is part of the definition
    assert max(cb.max(), cr.max()) == (256 if row[1] == P.FULL else 240)
    assert min(cb.min(), cr.min()) == (1 if row[1] == P.FULL else 16)
    y8, (cb8, cr8) = P.luma_of(r, g, b, *row), P.chroma_of(4 * r, 4 * g, 4 * b, *row)
    assert np.array_equal(y8, y) and np.array_equal(cb8, np.clip(cb, 0, 255)) and np.array_equal(cr8, np.clip(cr, 0, 255))
    # ... and back through the encode side's definition
    back = V.rgb_of(np.broadcast_to(y8, (256,) * 3), cb8, cr8, *row)
    distance = [int(np.abs(back[c].astype(np.int64) - np.broadcast_to(colours[c], (256,) * 3)).max()) for c in range(3)]
    assert distance == ([1, 1, 2] if row[1] == P.LIMITED else [1, 1, 1]), distance


def test_the_picture_takes_the_mean_of_two_by_two():
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (4, 8, 4), dtype=np.uint8)
    row = (P.BT601, P.LIMITED)
    y, uv = P.planes_of_rgba(d, *row)
    assert y.shape == (4, 8) and uv.shape == (2, 8) and y.dtype == uv.dtype == np.uint8
    for j in range(2):
        for i in range(4):
            quad = d[2 * j: 2 * j + 2, 2 * i: 2 * i + 2, :3].astype(np.int64).reshape(4, 3).sum(axis=0)
            cb, cr = P.chroma_of(quad[0], quad[1], quad[2], *row)
            assert (int(uv[j, 2 * i]), int(uv[j, 2 * i + 1])) == (int(cb), int(cr))
    for py in range(4):
        for px in range(8):
            assert int(y[py, px]) == int(P.luma_of(*[int(v) for v in d[py, px, :3]], *row))
    # alpha is not looked at
    d2 = d.copy()
    d2[..., 3] = 255 - d[..., 3]
    y2, uv2 = P.planes_of_rgba(d2, *row)
    assert np.array_equal(y, y2) and np.array_equal(uv, uv2)

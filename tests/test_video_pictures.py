"""The conversion of the video encode road (include/hap_gpu.h: HapGpuCompressNV12) as tests/_video_pictures.py defines it,
without a GPU or the library: the coefficients derived from the standards' fractions are the table the issue and the
header print and the constants hap_amd/csrc/ycbcr_rgb.hpp holds; over all 2^24 (Y, Cb, Cr) triples of each of the four
(matrix, range) rows every channel before the clamp is within 0.502 of the exact real value and the accumulators fit
32 bits; and the spot values the definition spells out."""
import os
import re

import numpy as np
import pytest

import _video_pictures as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (cy, crv, cbu, cgu, cgv) as the definition prints them
TABLE = {
    (V.BT601, V.LIMITED): (76309, 104597, 132201, 25675, 53279),
    (V.BT601, V.FULL): (65536, 91881, 116130, 22553, 46802),
    (V.BT709, V.LIMITED): (76309, 117489, 138438, 13975, 34925),
    (V.BT709, V.FULL): (65536, 103206, 121609, 12276, 30679),
}


@pytest.mark.parametrize("row", V.ROWS, ids=lambda r: V.NAMES[r])
def test_the_derived_coefficients_are_the_tables(row):
    k, offset = V.coefficients(*row)
    assert k == TABLE[row]
    assert offset == (16 if row[1] == V.LIMITED else 0)


def test_the_kernels_header_holds_the_same_constants():
    text = open(os.path.join(ROOT, "hap_amd", "csrc", "ycbcr_rgb.hpp")).read()
    found = re.findall(r"coefficients\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}\)*;?\s*// (BT601|BT709) (Limited|Full)", text)
    assert len(found) == 4, found
    matrices, ranges = {"BT601": V.BT601, "BT709": V.BT709}, {"Limited": V.LIMITED, "Full": V.FULL}
    seen = {}
    for *numbers, matrix, range_ in found:
        seen[(matrices[matrix], ranges[range_])] = tuple(int(n) for n in numbers)
    assert seen == {row: V.coefficients(*row)[0] + (V.coefficients(*row)[1],) for row in V.ROWS}
    # the enums' values are the ones the rows are looked up by
    assert re.search(r"enum \{ kBT601 = 0, kBT709 = 1 \}", text) and re.search(r"enum \{ kLimited = 0, kFull = 1 \}", text)
    header = open(os.path.join(ROOT, "include", "hap_gpu.h")).read()
    assert "HapGpuYCbCrMatrix_BT601 = 0, HapGpuYCbCrMatrix_BT709 = 1" in header
    assert "HapGpuYCbCrRange_Limited = 0, HapGpuYCbCrRange_Full = 1" in header


@pytest.mark.parametrize("row", V.ROWS, ids=lambda r: V.NAMES[r])
def test_every_triple_is_within_0_502_of_the_exact_value_and_fits_32_bits(row):
    """All 2^24 triples, a luma value at a time over the 256 x 256 (Cb, Cr) plane"""
    exact, offset = V.exact(*row)
    ey, erv, ebu, egu, egv = (float(v) for v in exact)
    (cy, crv, cbu, cgu, cgv), _offset = V.coefficients(*row)
    cb, cr = np.arange(256)[:, None], np.arange(256)[None, :]
    u, v = (cb - 128).astype(np.float64), (cr - 128).astype(np.float64)
    worst, largest, off_by_one, triples = 0.0, 0, 0, 0
    for y in range(256):
        l = ey * (y - offset)
        reals = (l + erv * v + 0.0 * u, l - egu * u - egv * v, l + ebu * u + 0.0 * v)
        accs = V.accumulators(y, cb, cr, *row)
        got = V.rgb_of(y, cb, cr, *row)
        for real, acc, channel in zip(reals, accs, got):
            acc = np.broadcast_to(acc, (256, 256))
            before = acc >> 16
            worst = max(worst, float(np.abs(before - real).max()))
            largest = max(largest, int(np.abs(acc).max()), int(np.abs(acc - 32768).max()))
            # after the clamp: the clip of what was there before it
            assert np.array_equal(np.broadcast_to(channel, (256, 256)), np.clip(before, 0, 255))
            off_by_one += int((before != np.rint(real)).sum())
            triples += before.size
        # (the partial sums of G too: the order of its two subtractions is the implementation's)
        largest = max(largest, int(np.abs(cy * (y - offset) - cgu * (cb - 128)).max()), int(np.abs(32768 - cgu * (cb - 128) - cgv * (cr - 128)).max()))
    print(f"{V.NAMES[row]}: worst distance {worst:.6f}, largest accumulator {largest}, "
          f"{100.0 * off_by_one / triples:.4f} % of channel values not the correctly rounded one")
    assert triples == 3 * 2 ** 24
    assert worst <= 0.502
    assert largest < 3.6e7 < 2 ** 31
    assert off_by_one / triples < 0.002                         # next to a tie, never more than one away
    for k in (cy, crv, cbu, cgu, cgv):
        assert 0 < k < 2 ** 23                                  # (what lets the device multiply 24-bit factors)


def test_the_spot_values():
    for matrix in (V.BT601, V.BT709):
        assert V.rgb_of(16, 128, 128, matrix, V.LIMITED) == (0, 0, 0)
        assert V.rgb_of(235, 128, 128, matrix, V.LIMITED) == (255, 255, 255)
        assert V.rgb_of(255, 128, 128, matrix, V.FULL) == (255, 255, 255)
        assert V.rgb_of(0, 128, 128, matrix, V.FULL) == (0, 0, 0)
        assert V.rgb_of(126, 128, 128, matrix, V.FULL) == (126, 126, 126)
        # outside the nominal range: clamped, as defined
        assert V.rgb_of(0, 128, 128, matrix, V.LIMITED) == (0, 0, 0) and V.rgb_of(255, 128, 128, matrix, V.LIMITED) == (255, 255, 255)
        for range_ in (V.LIMITED, V.FULL):
            # Y = Cb = Cr = 0: no red, no blue, and all the green the two negative chroma terms give back
            r, g, b = V.rgb_of(0, 0, 0, matrix, range_)
            accs = V.accumulators(0, 0, 0, matrix, range_)
            assert (r, b) == (0, 0) and accs[0] < 0 and accs[2] < 0
            assert g == min(255, max(0, int(accs[1]) >> 16)) and g > 0
            # Y = Cb = Cr = 255: red and blue at the top, green held down
            r, g, b = V.rgb_of(255, 255, 255, matrix, range_)
            assert (r, b) == (255, 255) and 0 < g < 255
    assert V.rgb_of(0, 0, 0, V.BT601, V.FULL) == (0, 135, 0)
    assert V.rgb_of(0, 0, 0, V.BT709, V.LIMITED) == (0, 77, 0)


def test_the_picture_replicates_each_pair_over_two_by_two():
    y, uv = V.distinct_chroma_nv12(8, 4)
    pic = V.rgba_of_nv12(y, uv, V.BT709, V.FULL)
    assert pic.shape == (4, 8, 4) and (pic[..., 3] == 255).all()
    for py in range(4):
        for px in range(8):
            cb, cr = uv[py >> 1, 2 * (px >> 1)], uv[py >> 1, 2 * (px >> 1) + 1]
            assert tuple(pic[py, px, :3]) == tuple(int(c) for c in V.rgb_of(y[py, px], cb, cr, V.BT709, V.FULL))
    quads = pic.reshape(2, 2, 4, 2, 4).transpose(0, 2, 1, 3, 4).reshape(8, 4, 4)
    assert all((q == q[0]).all() for q in quads) and len({q.tobytes() for q in quads}) == 8
    whole, view = V.padded(y, 12)
    assert whole.shape == (4, 12) and (whole[:, 8:] == V.POISON).all() and np.array_equal(view, y)

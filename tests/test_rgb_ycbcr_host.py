"""The conversion of the video decode road (hap_amd/csrc/rgb_ycbcr.hpp) against its definition, without a GPU.

The header's functions are __host__ __device__: tests/c/rgb_ycbcr_host.hip compiles them for the host (no device pass).
For each of the four (matrix, range) rows the luma of all 2^24 colours, the chroma of all 2^24 colours as four equal
texels (through the packed sums the kernel takes), the chroma of 2^24 seeded random sums (Rs, Gs, Bs) in 0 .. 1020 with
every corner added, and whole blocks of random texels come out byte for byte as tests/_video_planes.py makes them.  On
the device the products are 24-bit multiplies of the same factors: tests/test_video_decode_gpu.py's part."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import _video_planes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rgb_ycbcr") / "librgb_ycbcr_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "rgb_ycbcr_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    u, vp, n = ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t
    for name in ("rgb_ycbcr_luma_all", "rgb_ycbcr_chroma_all", "rgb_ycbcr_coefficients"):
        getattr(lib, name).argtypes = [u, u, vp]
    lib.rgb_ycbcr_chroma_of_sums.argtypes = [u, u, n, vp, vp, vp, vp]
    lib.rgb_ycbcr_blocks.argtypes = [u, u, n, vp, vp]
    return lib


@pytest.fixture(scope="module")
def sums():
    """2^24 seeded random (Rs, Gs, Bs) in 0 .. 1020, every corner added: made once, read-only"""
    rng = np.random.default_rng(1020)
    corners = np.array(list(itertools.product((0, 1020), repeat=3)), dtype=np.uint16)
    s = np.concatenate([rng.integers(0, 1021, (1 << 24, 3), dtype=np.uint16), corners])
    planes = tuple(np.ascontiguousarray(s[:, c]) for c in range(3))
    for p in planes:
        p.setflags(write=False)
    return planes


def pairs(cb, cr):
    return cb.astype(np.uint16) | cr.astype(np.uint16) << 8


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_every_colour_is_the_definitions(host, row):
    r, g, b = np.arange(256)[:, None, None], np.arange(256)[None, :, None], np.arange(256)[None, None, :]
    out = np.full(1 << 24, 0x5A, dtype=np.uint8)
    assert host.rgb_ycbcr_luma_all(row[0], row[1], out.ctypes.data) == 0
    want = P.luma_of(r, g, b, *row).reshape(-1)
    wrong = np.nonzero(out != want)[0]
    assert wrong.size == 0, [(int(i) >> 16, (int(i) >> 8) & 255, int(i) & 255, int(out[i]), int(want[i])) for i in wrong[:8]]
    out = np.full(1 << 24, 0x5A5A, dtype=np.uint16)
    assert host.rgb_ycbcr_chroma_all(row[0], row[1], out.ctypes.data) == 0
    want = pairs(*P.chroma_of(4 * r, 4 * g, 4 * b, *row)).reshape(-1)
    wrong = np.nonzero(out != want)[0]
    assert wrong.size == 0, [(int(i) >> 16, (int(i) >> 8) & 255, int(i) & 255, hex(int(out[i])), hex(int(want[i]))) for i in wrong[:8]]


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_random_sums_and_every_corner_are_the_definitions(host, sums, row):
    rs, gs, bs = sums
    out = np.full(rs.size, 0x5A5A, dtype=np.uint16)
    assert host.rgb_ycbcr_chroma_of_sums(row[0], row[1], rs.size, rs.ctypes.data, gs.ctypes.data, bs.ctypes.data,
                                         out.ctypes.data) == 0
    want = pairs(*P.chroma_of(rs, gs, bs, *row))
    wrong = np.nonzero(out != want)[0]
    assert wrong.size == 0, [(int(rs[i]), int(gs[i]), int(bs[i]), hex(int(out[i])), hex(int(want[i]))) for i in wrong[:8]]
    if row[1] == P.FULL:
        assert (want[-8:] & 0xFF).max() == 255 and (want[-8:] >> 8).max() == 255           # (the clamp was needed)


@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: P.NAMES[r])
def test_blocks_of_different_texels_are_the_definitions(host, row):
    """whole blocks the way the kernel stores them: four rows of Y and two rows of two pairs, a word each"""
    rng = np.random.default_rng([7, row[0], row[1]])
    n = 4096
    texels = rng.integers(0, 256, (n, 4, 4, 4), dtype=np.uint8)
    texels[:8] = np.array([0, 255], dtype=np.uint8)[rng.integers(0, 2, (8, 4, 4, 4))]
    out = np.zeros((n, 6), dtype=np.uint32)
    assert host.rgb_ycbcr_blocks(row[0], row[1], n, np.ascontiguousarray(texels).view(np.uint32).ctypes.data, out.ctypes.data) == 0
    picture = texels.transpose(1, 0, 2, 3).reshape(4, 4 * n, 4)                             # the blocks side by side
    y, uv = P.planes_of_rgba(picture, *row)
    want = np.concatenate([y.reshape(4, n, 4).transpose(1, 0, 2).reshape(n, 16), uv.reshape(2, n, 4).transpose(1, 0, 2).reshape(n, 8)],
                          axis=1)
    got = out.view(np.uint8).reshape(n, 24)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    assert wrong.size == 0, [(int(i), got[i].tolist(), want[i].tolist()) for i in wrong[:2]]


def test_the_table_and_the_refusals(host):
    for row in P.ROWS:
        out = (ctypes.c_int * 9)()
        assert host.rgb_ycbcr_coefficients(row[0], row[1], out) == 0
        assert tuple(out) == P.TABLE[row]
    guard = np.full(16, 0x5A5A5A5A, dtype=np.uint32)
    at = guard.ctypes.data
    for matrix, range_ in ((2, 0), (0, 2), (0xFFFFFFFF, 0), (1, 0xFFFFFFFF)):
        assert host.rgb_ycbcr_luma_all(matrix, range_, at) == 1
        assert host.rgb_ycbcr_chroma_all(matrix, range_, at) == 1
        assert host.rgb_ycbcr_coefficients(matrix, range_, at) == 1
        assert host.rgb_ycbcr_chroma_of_sums(matrix, range_, 4, at, at, at, at) == 1
        assert host.rgb_ycbcr_blocks(matrix, range_, 1, at, at) == 1
    assert (guard == 0x5A5A5A5A).all()

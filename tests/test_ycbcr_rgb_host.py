"""The conversion of the video encode road (hap_amd/csrc/ycbcr_rgb.hpp) against its definition, without a GPU.

The header's functions are __host__ __device__: tests/c/ycbcr_rgb_host.hip compiles them for the host (no device pass) and
all 2^24 (Y, Cb, Cr) triples of each of the four (matrix, range) rows come out byte for byte as tests/_video_pictures.py
makes them -- through the one-sample form and through the kernel's form, a pair's terms once and a luma sample under
them.  On the device the products are 24-bit multiplies of the same factors: tests/test_video_encode_gpu.py's part."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _video_pictures as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ycbcr_rgb") / "libycbcr_rgb_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "ycbcr_rgb_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    for name in ("ycbcr_rgb_all", "ycbcr_rgb_all_by_pair", "ycbcr_rgb_coefficients"):
        getattr(lib, name).argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def wanted():
    """the definition's packed texels of all 2^24 triples, per row: made once"""
    y, cb, cr = np.arange(256)[:, None, None], np.arange(256)[None, :, None], np.arange(256)[None, None, :]
    made = {}

    def of(row):
        if row not in made:
            r, g, b = (np.broadcast_to(c, (256, 256, 256)).astype(np.uint32) for c in V.rgb_of(y, cb, cr, *row))
            packed = (r | g << 8 | b << 16 | np.uint32(0xFF000000)).reshape(-1)
            packed.setflags(write=False)
            made[row] = packed
        return made[row]
    return of


@pytest.mark.parametrize("form", ["ycbcr_rgb_all", "ycbcr_rgb_all_by_pair"])
@pytest.mark.parametrize("row", V.ROWS, ids=lambda r: V.NAMES[r])
def test_every_triple_is_the_definitions(host, wanted, row, form):
    out = np.zeros(1 << 24, dtype=np.uint32)
    assert getattr(host, form)(row[0], row[1], out.ctypes.data) == 0
    want = wanted(row)
    wrong = np.nonzero(out != want)[0]
    assert wrong.size == 0, [(int(i) >> 16, (int(i) >> 8) & 255, int(i) & 255, hex(int(out[i])), hex(int(want[i]))) for i in wrong[:8]]


def test_the_table_and_the_refusals(host):
    for row in V.ROWS:
        out = (ctypes.c_int * 6)()
        assert host.ycbcr_rgb_coefficients(row[0], row[1], out) == 0
        k, offset = V.coefficients(*row)
        assert tuple(out) == k + (offset,)
    guard = np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    for matrix, range_ in ((2, 0), (0, 2), (0xFFFFFFFF, 0)):
        assert host.ycbcr_rgb_all(matrix, range_, guard.ctypes.data) == 1
        assert host.ycbcr_rgb_coefficients(matrix, range_, guard.ctypes.data) == 1
    assert (guard == 0x5A5A5A5A).all()

"""The Hap HDR picture entry points without a GPU: HapGpuDecompressRGBAHalf and HapGpuDecodeFramesRGBAHalf are
exported and refuse a missing context or missing arrays before they touch a device."""
import ctypes as C

import pytest

import _libs as L


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_half_picture_entry_points_without_a_gpu(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    u, ul, vp = C.c_uint, C.c_ulong, C.c_void_p
    tex = (C.c_ubyte * 16)()
    pic = (C.c_ubyte * 32)()
    for fmt in (L.FMT_BC6U, L.FMT_BC6S):
        assert lib.HapGpuDecompressRGBAHalf(None, tex, 16, fmt, 4, 4, pic, 32) == bad
        assert lib.HapGpuDecompressRGBAHalf(None, None, 0, fmt, 4, 4, None, 32) == bad
    res = (u * 2)(7, 7)
    assert lib.HapGpuDecodeFramesRGBAHalf(None, 2, None, None, None, 4, 4, 32, res, 0) == bad
    assert lib.HapGpuDecodeFramesRGBAHalf(None, 0, None, None, None, 4, 4, 32, None, 0) == bad
    frames, lens, pics = (vp * 1)(None), (ul * 1)(0), (vp * 1)(None)
    assert lib.HapGpuDecodeFramesRGBAHalf(None, 1, frames, lens, pics, 4, 4, 32, res, 0) == bad
    # the Python methods exist and take the documented arguments
    assert callable(hap.Context.decompress_rgba_half) and callable(hap.Context.decode_frames_rgba_half)

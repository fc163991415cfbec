"""The Hap HDR encode entry points without a GPU: HapGpuCompressRGBAHalf, HapGpuEncodeFramesRGBAHalf and
HapGpuEncodeFramesRGBAHalfBegin are declared, exported and refuse a missing context or missing buffers before they touch
a device; the Python methods exist."""
import ctypes as C
import inspect
import os
import re

import pytest

import _libs as L

NAMES = ("HapGpuCompressRGBAHalf", "HapGpuEncodeFramesRGBAHalf", "HapGpuEncodeFramesRGBAHalfBegin")


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_the_three_functions_are_declared_and_exported(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name in NAMES:
        assert re.search(r"unsigned int %s\(" % name, text), name
        assert hasattr(lib, name), name


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    used = C.c_ulong(7)
    pic = (C.c_ubyte * 128)()
    out = (C.c_ubyte * 64)()
    for fmt in (L.FMT_BC6U, L.FMT_BC6S, L.FMT_BC7):
        assert lib.HapGpuCompressRGBAHalf(None, pic, 4, 4, 32, fmt, out, 16, C.byref(used)) == bad
        assert lib.HapGpuCompressRGBAHalf(None, None, 4, 4, 32, fmt, None, 0, None) == bad
    assert used.value == 7
    pics = (C.c_void_p * 1)(C.addressof(pic))
    outs = (C.c_void_p * 1)(C.addressof(out))
    caps = (C.c_ulong * 1)(64)
    useds = (C.c_ulong * 1)(7)
    res = (C.c_uint * 1)(77)
    for fn in (lib.HapGpuEncodeFramesRGBAHalf, lib.HapGpuEncodeFramesRGBAHalfBegin):
        assert fn(None, 1, pics, 4, 4, 32, L.FMT_BC6U, L.COMP_SNAPPY, 1, outs, caps, useds, res, 0) == bad
        assert fn(None, 1, None, 4, 4, 32, L.FMT_BC6U, L.COMP_SNAPPY, 1, None, None, None, None, 0) == bad
    assert useds[0] == 7 and res[0] == 77


def test_the_python_methods_exist(hap):
    for name, last in (("compress_rgba_half", "output"), ("encode_frames_rgba_half", "flags"),
                       ("encode_frames_rgba_half_begin", "flags")):
        params = list(inspect.signature(getattr(hap.Context, name)).parameters)
        assert params[1:6] == [params[1], "width", "height", "row_bytes", "texture_format"] and params[-1] == last, name
    assert hasattr(hap.Context, "encode_finish")

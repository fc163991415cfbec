"""The Hap R encode entry point without a GPU: HapGpuCompressRGBAFlags is declared, exported and refuses a missing context
or missing buffers before it touches a device; the Python flag matches the header."""
import ctypes as C
import os
import re

import pytest

import _libs as L


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_compress_rgba_flags_is_declared_and_exported(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    assert re.search(r"unsigned int HapGpuCompressRGBAFlags\(", text)
    m = re.search(r"#define HAPGPU_ENCODE_BPTC_BLOCKS (0x[0-9A-Fa-f]+)u", text)
    assert m and int(m.group(1), 16) == 0x10
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    assert hasattr(lib, "HapGpuCompressRGBAFlags")


def test_compress_rgba_flags_refuses_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    used = C.c_ulong(7)
    pic = (C.c_ubyte * 64)()
    out = (C.c_ubyte * 16)()
    for flags in (0, hap.ENCODE_BPTC_BLOCKS):
        for fmt in (L.FMT_BC7, L.FMT_DXT5, L.FMT_BC6U):
            assert lib.HapGpuCompressRGBAFlags(None, pic, 4, 4, 16, fmt, flags, out, 16, C.byref(used)) == bad
            assert lib.HapGpuCompressRGBAFlags(None, None, 4, 4, 16, fmt, flags, None, 0, None) == bad
    assert used.value == 7


def test_python_flag_and_keyword(hap):
    import inspect
    assert hap.ENCODE_BPTC_BLOCKS == 0x10
    from hap_amd import api
    assert api.ENCODE_BPTC_BLOCKS == 0x10
    assert inspect.signature(hap.Context.compress_rgba).parameters["flags"].default == 0

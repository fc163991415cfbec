"""The Hap Alpha-Only entry points without a GPU: HapGpuCompressAlpha, HapGpuDecompressAlpha, HapGpuEncodeFramesAlpha,
HapGpuEncodeFramesAlphaBegin and HapGpuDecodeFramesAlpha are declared in the header, let out by the export map, exported
by the built library, bound by hap_amd._lib, and refuse a missing context before they touch a device or a client's
array; the Python methods exist."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = ("HapGpuCompressAlpha", "HapGpuDecompressAlpha", "HapGpuEncodeFramesAlpha", "HapGpuEncodeFramesAlphaBegin",
         "HapGpuDecodeFramesAlpha")


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_the_five_functions_are_declared_listed_exported_and_bound(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name in NAMES:
        assert re.search(r"unsigned int %s\(" % name, text), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes and bound.argtypes[0] is C.c_void_p, name
    # the argument lists the header gives them
    counts = {n: len(getattr(hap._lib.lib, n).argtypes) for n in NAMES}
    assert counts == {"HapGpuCompressAlpha": 8, "HapGpuDecompressAlpha": 7, "HapGpuEncodeFramesAlpha": 13,
                      "HapGpuEncodeFramesAlphaBegin": 13, "HapGpuDecodeFramesAlpha": 10}


def test_the_header_states_the_rules_and_the_old_calls_name_the_new_ones():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    assert "no pixel decoder here" not in text
    rgba_decode = text[text.index("Frames in, pixels out"): text.index("unsigned int HapGpuDecodeFramesRGBA(")]
    assert "HapGpuDecodeFramesAlpha" in rgba_decode
    decompress = text[text.index("Block-compressed texture -> RGBA8"): text.index("unsigned int HapGpuDecompressRGBA(")]
    assert "HapGpuDecompressAlpha" in decompress


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    used = C.c_ulong(7)
    pic = (C.c_ubyte * 16)(*([0x5A] * 16))
    tex = (C.c_ubyte * 8)()
    assert lib.HapGpuCompressAlpha(None, pic, 4, 4, 4, tex, 8, C.byref(used)) == bad
    assert lib.HapGpuCompressAlpha(None, None, 4, 4, 4, None, 0, None) == bad
    assert used.value == 7
    assert lib.HapGpuDecompressAlpha(None, tex, 8, 4, 4, pic, 4) == bad
    assert lib.HapGpuDecompressAlpha(None, None, 0, 4, 4, None, 4) == bad
    assert bytes(pic) == b"\x5a" * 16
    pics = (C.c_void_p * 1)(C.addressof(pic))
    outs = (C.c_void_p * 1)(C.addressof(tex))
    caps = (C.c_ulong * 1)(8)
    useds = (C.c_ulong * 1)(7)
    res = (C.c_uint * 1)(77)
    for fn in (lib.HapGpuEncodeFramesAlpha, lib.HapGpuEncodeFramesAlphaBegin):
        assert fn(None, 1, pics, 4, 4, 4, L.COMP_SNAPPY, 1, outs, caps, useds, res, 0) == bad
        assert fn(None, 1, None, 4, 4, 4, L.COMP_SNAPPY, 1, None, None, None, None, 0) == bad
    assert lib.HapGpuDecodeFramesAlpha(None, 1, outs, caps, pics, 4, 4, 4, res, 0) == bad
    assert lib.HapGpuDecodeFramesAlpha(None, 1, None, None, None, 4, 4, 4, None, 0) == bad
    assert useds[0] == 7 and res[0] == 77 and bytes(pic) == b"\x5a" * 16


def test_the_python_methods_exist(hap):
    want = {"compress_alpha": ["alpha", "width", "height", "row_bytes", "output"],
            "decompress_alpha": ["texture", "width", "height", "out", "row_bytes"],
            "encode_frames_alpha": ["alpha_frames", "width", "height", "row_bytes", "compressor", "chunk_count", "outputs",
                                    "flags"],
            "encode_frames_alpha_begin": ["alpha_frames", "width", "height", "row_bytes", "compressor", "chunk_count",
                                          "outputs", "flags"],
            "decode_frames_alpha": ["frames", "frame_bytes", "pictures", "width", "height", "row_bytes", "flags"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(hap.Context, name)).parameters)[1:] == params, name
    assert hasattr(hap.Context, "encode_finish")

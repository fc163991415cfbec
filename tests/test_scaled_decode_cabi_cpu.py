"""The half- and quarter-size picture decoders without a GPU: HapGpuDecompressRGBAScaled and HapGpuDecodeFramesRGBAScaled
are declared in the header, let out by the export map, exported by the built library, bound by hap_amd._lib with the
header's argument counts, and refuse a missing context before they touch a device or a client's array; the Python
methods exist."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuDecompressRGBAScaled": 11, "HapGpuDecodeFramesRGBAScaled": 12}


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_the_two_functions_are_declared_listed_exported_and_bound(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
        assert declared, name
        # the argument list the header gives it
        assert len(declared.group(1).split(",")) == count, name
        assert "scaleLog2" in declared.group(1), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name


def test_the_header_states_the_rule_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name in NAMES:
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = comment[comment.rindex("/*"):]
        assert "Bad_Arguments" in comment and "RGBA16F" in comment and "A8" in comment, name
    single = text[: text.index("unsigned int HapGpuDecompressRGBAScaled(")]
    single = single[single.rindex("/*"):]
    assert "(1 << (2 * scaleLog2 - 1))" in single and "16 >> scaleLog2" in single


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    pic = (C.c_ubyte * 16)(*([0x5A] * 16))
    tex = (C.c_ubyte * 16)()
    for scale in (1, 2):
        assert lib.HapGpuDecompressRGBAScaled(None, tex, 16, L.FMT_DXT5, None, 0, 4, 4, scale, pic, 8) == bad
        assert lib.HapGpuDecompressRGBAScaled(None, None, 0, L.FMT_DXT5, None, 0, 4, 4, scale, None, 8) == bad
    assert bytes(pic) == b"\x5a" * 16
    frames = (C.c_void_p * 1)(C.addressof(tex))
    lens = (C.c_ulong * 1)(16)
    pics = (C.c_void_p * 1)(C.addressof(pic))
    res = (C.c_uint * 1)(77)
    for scale in (0, 1, 2, 3):
        assert lib.HapGpuDecodeFramesRGBAScaled(None, 1, frames, lens, 1, pics, 4, 4, scale, 8, res, 0) == bad
        assert lib.HapGpuDecodeFramesRGBAScaled(None, 1, None, None, 1, None, 4, 4, scale, 8, None, 0) == bad
    assert res[0] == 77 and bytes(pic) == b"\x5a" * 16


def test_the_python_methods_exist(hap):
    want = {"decompress_rgba_scaled": ["texture", "texture_format", "width", "height", "scale_log2", "rgba", "alpha",
                                       "row_bytes"],
            "decode_frames_rgba_scaled": ["frames", "frame_bytes", "texture_count", "rgba_frames", "width", "height",
                                          "scale_log2", "row_bytes", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.decompress_rgba_scaled)
    assert [sig.parameters[p].default for p in ("rgba", "alpha", "row_bytes")] == [None, None, None]
    sig = inspect.signature(hap.Context.decode_frames_rgba_scaled)
    assert sig.parameters["row_bytes"].default is None and sig.parameters["flags"].default == 0

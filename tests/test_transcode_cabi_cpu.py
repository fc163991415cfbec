"""The transcode calls without a GPU: HapGpuTranscodeTexture and HapGpuTranscodeFrames are declared in the header, let
out by the export map, exported by the built library, bound by hap_amd._lib with the header's argument counts, and
refuse a missing context before they touch a device or a client's array; the Python methods exist."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuTranscodeTexture": 14, "HapGpuTranscodeFrames": 18}


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


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name in NAMES:
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = comment[comment.rindex("/*"):]
        assert "Bad_Arguments" in comment, name
        # what is out of scope: BC7 / BC6H through the kernel, A8 and RGBA16F, rectangles
        assert "Out of scope" in comment and "BC7" in comment and "BC6H" in comment, name
        assert "A8" in comment and "RGBA16F" in comment and "ectangles" in comment, name
    frames = text[: text.index("unsigned int HapGpuTranscodeFrames(")]
    frames = frames[frames.rindex("/*"):]
    # the definition, the pass-through rule, the forms that do not exist
    assert "byte for byte" in frames and "HapGpuEncodeFramesRGBA" in frames and "HapGpuDecodeFramesRGBAScaled" in frames
    assert "Pass-through" in frames and "generation loss" in frames and "A_RGTC1" in frames
    assert "Begin" in frames and "OnDevices" in frames and "Sequence" in frames
    assert "Internal_Error" in frames and "Buffer_Too_Small" in frames


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    tex = (C.c_ubyte * 16)()
    out = (C.c_ubyte * 16)(*([0x5A] * 16))
    fmts = (C.c_uint * 1)(L.FMT_DXT5)
    outs = (C.c_void_p * 1)(C.addressof(out))
    lens = (C.c_ulong * 1)(16)
    used = (C.c_ulong * 1)(77)
    for scale in (0, 1, 2, 3):
        assert lib.HapGpuTranscodeTexture(None, tex, 16, L.FMT_YCOCG, None, 0, 4 << scale, 4 << scale, scale, 1, fmts,
                                          outs, lens, used) == bad
        assert lib.HapGpuTranscodeTexture(None, None, 0, L.FMT_YCOCG, None, 0, 4, 4, scale, 1, None, None, None, None) == bad
    assert bytes(out) == b"\x5a" * 16 and used[0] == 77
    frames = (C.c_void_p * 1)(C.addressof(tex))
    ones = (C.c_uint * 1)(1)
    res = (C.c_uint * 1)(77)
    for scale in (0, 1, 2, 3):
        assert lib.HapGpuTranscodeFrames(None, 1, frames, lens, 1, 4 << scale, 4 << scale, scale, 1, fmts, ones, ones, outs,
                                         lens, used, res, 0, 0) == bad
        assert lib.HapGpuTranscodeFrames(None, 1, None, None, 1, 4, 4, scale, 1, None, None, None, None, None, None, None,
                                         0, 0) == bad
    assert res[0] == 77 and used[0] == 77 and bytes(out) == b"\x5a" * 16


def test_the_python_methods_exist(hap):
    want = {"transcode_texture": ["texture", "texture_format", "width", "height", "scale_log2", "output_formats", "alpha",
                                  "outputs"],
            "transcode_frames": ["frames", "frame_bytes", "source_texture_count", "width", "height", "scale_log2",
                                 "formats", "compressors", "chunk_counts", "outputs", "decode_flags", "encode_flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.transcode_texture)
    assert [sig.parameters[p].default for p in ("alpha", "outputs")] == [None, None]
    sig = inspect.signature(hap.Context.transcode_frames)
    assert [sig.parameters[p].default for p in ("decode_flags", "encode_flags")] == [0, 0]

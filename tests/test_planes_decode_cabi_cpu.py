"""The planar float decoders without a GPU: HapGpuDecompressPlanes and HapGpuDecodeFramesPlanes are declared in the header,
let out by the export map, exported by the built library, bound by hap_amd._lib with the header's argument counts, and
refuse a missing context before they touch a device or a client's array; the Python methods exist and refuse tensors
they cannot take before they need a context."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuDecompressPlanes": 16, "HapGpuDecodeFramesPlanes": 17}


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
        for word in ("scaleLog2", "channels", "element", "planeBytes", "rowBytes", "scale", "bias"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    enum = re.search(r"enum HapGpuPlaneElement \{([^}]*)\}", text)
    assert enum and [w.strip() for w in enum.group(1).split(",")] == [
        "HapGpuPlaneElement_F16 = 0", "HapGpuPlaneElement_BF16 = 1", "HapGpuPlaneElement_F32 = 2"]


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name in NAMES:
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])       # (one line: words wrap anywhere)
        assert "Bad_Arguments" in comment, name
        for word in ("BC7", "BC6H", "A_RGTC1", "ectangles", "ost tensors"):
            assert word in comment, (name, word)
        # two roundings: a multiply, then an add, and not a fused one
        assert "multiply" in comment and "add" in comment and re.search(r"(?i)not\s+(a\s+)?fused", comment), name
    single = text[: text.index("unsigned int HapGpuDecompressPlanes(")]
    single = single[single.rindex("/*"):]
    assert "4 >> scaleLog2" in single and "n * e" in single and "subnormal" in single


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    guard = 0x5A
    out = (C.c_ubyte * 128)(*([guard] * 128))
    tex = (C.c_ubyte * 16)()
    scale = (C.c_float * 8)(*([0.5] * 8))             # four floats the call may read, four behind them
    bias = (C.c_float * 8)(*([0.25] * 8))
    for s in (0, 1, 2):
        assert lib.HapGpuDecompressPlanes(None, tex, 16, L.FMT_DXT5, None, 0, 4, 4, s, 4, 0, out, 32, 8, scale, bias) == bad
        assert lib.HapGpuDecompressPlanes(None, None, 0, L.FMT_DXT5, None, 0, 4, 4, s, 4, 0, None, 32, 8, None, None) == bad
    assert bytes(out) == bytes([guard]) * 128
    frames = (C.c_void_p * 2)(C.addressof(tex), 0x5A5A)
    lens = (C.c_ulong * 2)(16, 0x5A5A)
    outs = (C.c_void_p * 2)(C.addressof(out), 0x5A5A)
    res = (C.c_uint * 2)(77, 78)
    for s in (0, 1, 2, 3):
        assert lib.HapGpuDecodeFramesPlanes(None, 1, frames, lens, 1, outs, 4, 4, s, 4, 0, 32, 8, scale, bias, res, 0) == bad
        assert lib.HapGpuDecodeFramesPlanes(None, 1, None, None, 1, None, 4, 4, s, 4, 0, 32, 8, None, None, None, 0) == bad
    # the guard entries behind every client array, and the arrays themselves
    assert list(res) == [77, 78] and bytes(out) == bytes([guard]) * 128
    assert list(frames) == [C.addressof(tex), 0x5A5A] and list(lens) == [16, 0x5A5A]
    assert list(outs) == [C.addressof(out), 0x5A5A]
    assert list(scale) == [0.5] * 8 and list(bias) == [0.25] * 8 and bytes(tex) == bytes(16)


def test_the_python_methods_exist(hap):
    want = {"decompress_planes": ["texture", "texture_format", "width", "height", "out", "scale_log2", "scale", "bias",
                                  "alpha"],
            "decode_frames_planes": ["frames", "frame_bytes", "texture_count", "out", "width", "height", "scale_log2",
                                     "scale", "bias", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.decompress_planes)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "alpha")] == [0, None, None, None]
    sig = inspect.signature(hap.Context.decode_frames_planes)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "flags")] == [0, None, None, 0]


def test_decode_frames_planes_refuses_tensors_it_cannot_take(hap):
    torch = pytest.importorskip("torch")
    frame = bytes(16)
    # (no context is needed: the tensors are looked at before anything else)
    method = hap.Context.decode_frames_planes                   # (unbound: self is never looked at)
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [16], 1, torch.zeros((1, 3, 4, 4), dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [16], 1, [torch.zeros((3, 4, 4), dtype=torch.uint8)], 4, 4)
    wide = torch.zeros((1, 3, 4, 8), dtype=torch.float16)[..., ::2]
    assert wide.shape == (1, 3, 4, 4) and wide.stride(-1) == 2
    with pytest.raises(ValueError, match="stride"):
        method(None, [frame], [16], 1, wide, 4, 4)
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [16], 1, torch.zeros((1, 3, 4, 8), dtype=torch.float16), 4, 4)
    with pytest.raises(ValueError):
        hap.Context.decompress_planes(None, frame, L.FMT_DXT5, 4, 4, torch.zeros((3, 4, 4), dtype=torch.uint8))

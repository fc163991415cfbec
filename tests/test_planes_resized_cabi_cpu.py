"""The planar float decoders of a resized crop without a GPU: HapGpuDecompressPlanesResized and
HapGpuDecodeFramesPlanesResized are declared in the header, let out by the export map, exported by the built library,
bound by hap_amd._lib with the header's argument counts, and refuse before they touch a device or a client's array; the
header states the definition and the limits; the Python methods exist and refuse tensors and crop lists they cannot
take before they need a context; the host asks hap_region.h's rules whether a crop's blocks are a rectangle."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuDecompressPlanesResized": 22, "HapGpuDecodeFramesPlanesResized": 23}


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def header_comment(text, name):
    """The comment in front of a declaration, on one line (words wrap anywhere)"""
    comment = text[: text.index("unsigned int %s(" % name)]
    return re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])


def test_the_two_functions_are_declared_listed_exported_and_bound(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
        assert declared, name
        assert len(declared.group(1).split(",")) == count, name
        for word in ("outWidth", "outHeight", "scaleLog2", "channels", "element", "planeBytes", "rowBytes", "scale", "bias"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    single = re.search(r"unsigned int HapGpuDecompressPlanesResized\(([^;]*)\);", text).group(1)
    for word in ("cropX,", "cropY,", "cropWidth,", "cropHeight,"):
        assert word in single, word
    frames = re.search(r"unsigned int HapGpuDecodeFramesPlanesResized\(([^;]*)\);", text).group(1)
    for word in ("cropXs", "cropYs", "cropWidths", "cropHeights"):
        assert "const unsigned int *%s" % word in frames, word


def test_the_header_states_the_definition_the_limits_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    frames = header_comment(text, "HapGpuDecodeFramesPlanesResized")
    assert "The definition, and the only one" in frames
    # the taps and the blend, as formulas
    for formula in ("num = max((2 * i + 1) * c - o, 0)", "i0 = min(num / (2 * o), c - 1)", "i1 = min(i0 + 1, c - 1)",
                    "frac = num % (2 * o)", "w = (frac * 256 + o) / (2 * o)",
                    "v = (top * (256 - wy) + bot * wy + 32768) >> 16"):
        assert formula in re.sub(r"\s+", " ", frames), formula
    assert "multiply" in frames and "add" in frames and re.search(r"(?i)not\s+(a\s+)?fused", frames)
    assert "exact crop" in frames and "bit for bit" in frames and "HapGpuDecodeFramesPlanesRegion" in frames
    assert "HapGpuDecodeFramesRGBA " in frames and "HapGpuDecodeFramesRGBAScaled" in frames
    # the limits
    for word in ("16384", "cw <= 4 * outWidth", "ch <= 4 * outHeight", "at most 2", "multiples of e", "Bad_Arguments",
                 "Internal_Error", "its tensor is untouched", "NULL crop array", "HapGpuSkippedTextureBytes"):
        assert word in frames, word
    # out of scope
    for word in ("BC7", "BC6H", "A_RGTC1", "ost tensors", "output size per frame", "ther filters", "OnDevices", "Sequence",
                 "RGBA8 output"):
        assert word in frames, word
    single = header_comment(text, "HapGpuDecompressPlanesResized")
    for word in ("HapGpuDecodeFramesPlanesResized", "Bad_Arguments", "multiples of e", "16384", "BC7", "ost tensors",
                 "not fused"):
        assert word in single, word
    # the calls it extends point at it, and say what they said
    for name in ("HapGpuDecodeFramesPlanes", "HapGpuDecodeFramesPlanesRegion"):
        assert "HapGpuDecodeFramesPlanesResized" in header_comment(text, name), name
    region = header_comment(text, "HapGpuDecodeFramesPlanesRegion")
    assert "rectangles of different sizes in one call" in region and "rectangles off the block grid" in region


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    guard = 0x5A
    out = (C.c_ubyte * 128)(*([guard] * 128))
    tex = (C.c_ubyte * 64)()
    scale = (C.c_float * 8)(*([0.5] * 8))             # four floats the call may read, four behind them
    bias = (C.c_float * 8)(*([0.25] * 8))
    for s in (0, 1, 2, 3):
        for crop in ((0, 0, 4, 4), (1, 1, 3, 2), (0, 0, 8, 8), (7, 7, 2, 2), (0, 0, 0, 1)):
            for size in ((2, 2), (0, 2), (2, 16385)):
                assert lib.HapGpuDecompressPlanesResized(None, tex, 64, L.FMT_DXT5, None, 0, 8, 8, s, *crop, *size, 4, 0, out,
                                                         32, 8, scale, bias) == bad
                assert lib.HapGpuDecompressPlanesResized(None, None, 0, L.FMT_DXT5, None, 0, 8, 8, s, *crop, *size, 4, 0,
                                                         None, 32, 8, None, None) == bad
    assert bytes(out) == bytes([guard]) * 128
    frames = (C.c_void_p * 2)(C.addressof(tex), 0x5A5A)
    lens = (C.c_ulong * 2)(64, 0x5A5A)
    outs = (C.c_void_p * 2)(C.addressof(out), 0x5A5A)
    xs, ys = (C.c_uint * 2)(1, 0x5A5A), (C.c_uint * 2)(0, 0x5A5A)
    ws, hs = (C.c_uint * 2)(3, 0x5A5A), (C.c_uint * 2)(5, 0x5A5A)
    res = (C.c_uint * 2)(77, 78)
    for s in (0, 1, 2, 3):
        for size in ((4, 4), (1, 1), (0, 4), (4, 16385)):
            assert lib.HapGpuDecodeFramesPlanesResized(None, 1, frames, lens, 1, outs, 8, 8, s, xs, ys, ws, hs, *size, 4, 0,
                                                       32, 8, scale, bias, res, 0) == bad
            assert lib.HapGpuDecodeFramesPlanesResized(None, 1, None, None, 1, None, 8, 8, s, None, None, None, None, *size,
                                                       4, 0, 32, 8, None, None, None, 0) == bad
    # the guard entries behind every client array, and the arrays themselves
    assert list(res) == [77, 78] and bytes(out) == bytes([guard]) * 128
    assert list(frames) == [C.addressof(tex), 0x5A5A] and list(lens) == [64, 0x5A5A]
    assert list(outs) == [C.addressof(out), 0x5A5A]
    assert list(xs) == [1, 0x5A5A] and list(ys) == [0, 0x5A5A] and list(ws) == [3, 0x5A5A] and list(hs) == [5, 0x5A5A]
    assert list(scale) == [0.5] * 8 and list(bias) == [0.25] * 8 and bytes(tex) == bytes(64)


def test_the_python_methods_exist(hap):
    want = {"decompress_planes_resized": ["texture", "texture_format", "width", "height", "crop", "out", "scale_log2",
                                          "scale", "bias", "alpha"],
            "decode_frames_planes_resized": ["frames", "frame_bytes", "texture_count", "out", "width", "height", "crops",
                                             "out_size", "scale_log2", "scale", "bias", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.decompress_planes_resized)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "alpha")] == [0, None, None, None]
    sig = inspect.signature(hap.Context.decode_frames_planes_resized)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "flags")] == [0, None, None, 0]


def test_the_python_methods_refuse_tensors_and_crops_they_cannot_take(hap):
    torch = pytest.importorskip("torch")
    frame = bytes(64)
    # (no context is needed: the tensors and the crops are looked at before anything else)
    method = hap.Context.decode_frames_planes_resized            # (unbound: self is never looked at)
    crop = (1, 1, 5, 3)
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 4, 4), dtype=torch.uint8), 8, 8, [crop], (4, 4))
    wide = torch.zeros((1, 3, 4, 8), dtype=torch.float16)[..., ::2]
    with pytest.raises(ValueError, match="stride"):
        method(None, [frame], [64], 1, wide, 8, 8, [crop], (4, 4))
    # the tensor is the output's size whatever the crop and the scale are
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 3, 5), dtype=torch.float16), 8, 8, [crop], (4, 4))
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 2, 2), dtype=torch.float16), 8, 8, [crop], (4, 4), scale_log2=1)
    with pytest.raises(ValueError, match="device memory"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 4, 4), dtype=torch.float16), 8, 8, [crop], (4, 4), scale_log2=1)
    host = torch.zeros((2, 3, 4, 4), dtype=torch.float16)
    for crops in ([crop], [crop] * 3, [], [crop, (4, 4)], [crop, (0, 0, 4, 4, 4)]):
        with pytest.raises(ValueError, match="one crop"):
            method(None, [frame, frame], [64, 64], 1, host, 8, 8, crops, (4, 4))
    with pytest.raises(ValueError):
        hap.Context.decompress_planes_resized(None, frame, L.FMT_DXT5, 8, 8, crop, torch.zeros((3, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out_h, out_w"):
        hap.Context.decompress_planes_resized(None, frame, L.FMT_DXT5, 8, 8, crop, torch.zeros((1, 3, 4, 4), dtype=torch.float16))
    with pytest.raises(ValueError, match="device memory"):
        hap.Context.decompress_planes_resized(None, frame, L.FMT_DXT5, 8, 8, crop, torch.zeros((3, 7, 9), dtype=torch.float16))


def test_the_new_road_restates_nothing():
    """hap_region.h stays the one predicate: the host turns a crop into the rectangle of its blocks and asks
    hapb_region_fits; the kernel and the host test share one text of the taps."""
    csrc = os.path.join(L.ROOT, "hap_amd", "csrc")
    sources = {name: open(os.path.join(csrc, name)).read() for name in sorted(os.listdir(csrc))
               if name.endswith((".c", ".h", ".hip", ".hpp"))}
    for function in ("hap_region_needs_bytes", "hap_region_valid", "hap_region_geometry_valid"):
        defined = [name for name, text in sources.items() if re.search(r"\bint %s\(" % function, text)]
        assert defined == ["hap_region.h"], (function, defined)
    pictures = sources["hap_pictures.c"]
    body = pictures[pictures.index("int hapb_resize_region("):]
    body = body[: body.index("\n}\n")]
    assert "return hapb_region_fits(region, height);" in body
    assert "refused = !hapb_resize_region(resize, done + f, width, height, scale_log2, &own)" in pictures
    api = sources["hap_api.c"]
    for name in NAMES:
        body = api[api.index("unsigned int %s(" % name):]
        assert "hapb_resize_out_valid(" in body[: body.index("\n}\n")], name
    defined = [name for name, text in sources.items() if re.search(r"\btap tap_of\(", text)]
    assert defined == ["resample_taps.hpp"], defined
    kernel = sources["bc_resample_planes.hip"]
    assert '#include "resample_taps.hpp"' in kernel and "tap_of(" in kernel and "blend_texel(" in kernel
    assert "bc_decode_body<FMT, HAS_ALPHA, false, true>" in kernel and "bc_decode_scaled_body<FMT, HAS_ALPHA, S, true>" in kernel
    host = open(os.path.join(L.ROOT, "tests", "c", "resample_taps_host.hip")).read()
    assert '#include "resample_taps.hpp"' in host

"""The planar float decoders of a rectangle without a GPU: HapGpuDecompressPlanesRegion and HapGpuDecodeFramesPlanesRegion
are declared in the header, let out by the export map, exported by the built library, bound by hap_amd._lib with the
header's argument counts, and refuse a missing context before they touch a device or a client's array; the header states
the definition; the Python methods exist and refuse tensors and origin lists they cannot take before they need a
context; hap_region.h is still the one definition of what a rectangle needs."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuDecompressPlanesRegion": 20, "HapGpuDecodeFramesPlanesRegion": 21}


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
        for word in ("regionWidth", "regionHeight", "scaleLog2", "channels", "element", "planeBytes", "rowBytes", "scale",
                     "bias"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    single = re.search(r"unsigned int HapGpuDecompressPlanesRegion\(([^;]*)\);", text).group(1)
    assert "regionX," in single and "regionY," in single
    frames = re.search(r"unsigned int HapGpuDecodeFramesPlanesRegion\(([^;]*)\);", text).group(1)
    assert "const unsigned int *regionXs" in frames and "const unsigned int *regionYs" in frames


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name in NAMES:
        comment = header_comment(text, name)
        assert "Bad_Arguments" in comment, name
        # the definition: the crop, bit for bit, of the whole-frame call's tensor; two roundings, not a fused one
        assert "bit for bit" in comment and "The definition, and the only one" in comment, name
        assert "multiply" in comment and "add" in comment and re.search(r"(?i)not\s+(a\s+)?fused", comment), name
        assert "box mean never spans two blocks" in comment, name
        assert "n * e" in comment and "4 >> scaleLog2" in comment, name
        for word in ("BC7", "BC6H", "A_RGTC1", "ost tensors", "off the block grid"):
            assert word in comment, (name, word)
    frames = header_comment(text, "HapGpuDecodeFramesPlanesRegion")
    for word in ("regionXs", "regionYs", "HapGpuDecodeFramesPlanes ", "rectangles of different sizes", "OnDevices", "Sequence",
                 "rectangle together with scaleLog2", "Internal_Error", "its tensor is untouched"):
        assert word in frames, word
    # the calls it joins point at it
    for name in ("HapGpuDecompressPlanes", "HapGpuDecodeFramesPlanes", "HapGpuDecodeFramesRGBARegion"):
        assert "PlanesRegion" in header_comment(text, name), name


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    guard = 0x5A
    out = (C.c_ubyte * 128)(*([guard] * 128))
    tex = (C.c_ubyte * 64)()
    scale = (C.c_float * 8)(*([0.5] * 8))             # four floats the call may read, four behind them
    bias = (C.c_float * 8)(*([0.25] * 8))
    for s in (0, 1, 2):
        for region in ((0, 0, 4, 4), (4, 4, 4, 4), (0, 0, 8, 8), (2, 0, 4, 4), (8, 0, 4, 4)):
            assert lib.HapGpuDecompressPlanesRegion(None, tex, 64, L.FMT_DXT5, None, 0, 8, 8, *region, s, 4, 0, out, 32, 8,
                                                    scale, bias) == bad
            assert lib.HapGpuDecompressPlanesRegion(None, None, 0, L.FMT_DXT5, None, 0, 8, 8, *region, s, 4, 0, None, 32, 8,
                                                    None, None) == bad
    assert bytes(out) == bytes([guard]) * 128
    frames = (C.c_void_p * 2)(C.addressof(tex), 0x5A5A)
    lens = (C.c_ulong * 2)(64, 0x5A5A)
    outs = (C.c_void_p * 2)(C.addressof(out), 0x5A5A)
    xs, ys = (C.c_uint * 2)(4, 0x5A5A), (C.c_uint * 2)(0, 0x5A5A)
    res = (C.c_uint * 2)(77, 78)
    for s in (0, 1, 2, 3):
        for size in ((4, 4), (8, 8), (0, 4), (12, 4)):
            assert lib.HapGpuDecodeFramesPlanesRegion(None, 1, frames, lens, 1, outs, 8, 8, xs, ys, *size, s, 4, 0, 32, 8,
                                                      scale, bias, res, 0) == bad
            assert lib.HapGpuDecodeFramesPlanesRegion(None, 1, None, None, 1, None, 8, 8, None, None, *size, s, 4, 0, 32, 8,
                                                      None, None, None, 0) == bad
    # the guard entries behind every client array, and the arrays themselves
    assert list(res) == [77, 78] and bytes(out) == bytes([guard]) * 128
    assert list(frames) == [C.addressof(tex), 0x5A5A] and list(lens) == [64, 0x5A5A]
    assert list(outs) == [C.addressof(out), 0x5A5A]
    assert list(xs) == [4, 0x5A5A] and list(ys) == [0, 0x5A5A]
    assert list(scale) == [0.5] * 8 and list(bias) == [0.25] * 8 and bytes(tex) == bytes(64)


def test_the_python_methods_exist(hap):
    want = {"decompress_planes_region": ["texture", "texture_format", "width", "height", "region", "out", "scale_log2",
                                         "scale", "bias", "alpha"],
            "decode_frames_planes_region": ["frames", "frame_bytes", "texture_count", "out", "width", "height", "origins",
                                            "region_size", "scale_log2", "scale", "bias", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.decompress_planes_region)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "alpha")] == [0, None, None, None]
    sig = inspect.signature(hap.Context.decode_frames_planes_region)
    assert [sig.parameters[p].default for p in ("scale_log2", "scale", "bias", "flags")] == [0, None, None, 0]


def test_the_python_methods_refuse_tensors_and_origins_they_cannot_take(hap):
    torch = pytest.importorskip("torch")
    frame = bytes(64)
    # (no context is needed: the tensors and the origins are looked at before anything else)
    method = hap.Context.decode_frames_planes_region            # (unbound: self is never looked at)
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 4, 4), dtype=torch.uint8), 8, 8, [(0, 0)], (4, 4))
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [64], 1, [torch.zeros((3, 4, 4), dtype=torch.uint8)], 8, 8, [(0, 0)], (4, 4))
    wide = torch.zeros((1, 3, 4, 8), dtype=torch.float16)[..., ::2]
    assert wide.shape == (1, 3, 4, 4) and wide.stride(-1) == 2
    with pytest.raises(ValueError, match="stride"):
        method(None, [frame], [64], 1, wide, 8, 8, [(0, 0)], (4, 4))
    # the tensor is the rectangle's scaled size, not the frame's
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 8, 8), dtype=torch.float16), 8, 8, [(0, 0)], (4, 4))
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 4, 4), dtype=torch.float16), 8, 8, [(0, 0)], (4, 4), scale_log2=1)
    with pytest.raises(ValueError, match="device memory"):
        method(None, [frame], [64], 1, torch.zeros((1, 3, 4, 4), dtype=torch.float16), 8, 8, [(0, 0)], (4, 4))
    # (the origins are counted first: a tensor in device memory is not needed to be told)
    host = torch.zeros((2, 3, 4, 4), dtype=torch.float16)
    for origins in ([(0, 0)], [(0, 0), (4, 4), (0, 4)], [], [(0, 0), (4,)], [(0, 0), (4, 4, 4)]):
        with pytest.raises(ValueError, match="one origin per frame"):
            method(None, [frame, frame], [64, 64], 1, host, 8, 8, origins, (4, 4))
    with pytest.raises(ValueError):
        hap.Context.decompress_planes_region(None, frame, L.FMT_DXT5, 8, 8, (0, 0, 4, 4),
                                             torch.zeros((3, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="per frame"):
        hap.Context.decompress_planes_region(None, frame, L.FMT_DXT5, 8, 8, (0, 0, 4, 4),
                                             torch.zeros((3, 8, 8), dtype=torch.float16))


def test_the_predicate_still_has_one_definition_and_the_new_road_restates_nothing():
    """The spirit of test_region_decode_cabi_cpu.test_there_is_one_definition_of_the_predicate for the new users: the
    per-job skip asks hap_region.h, the host builds rectangles and asks hapb_region_fits, and nobody writes the
    arithmetic of a block row's bytes again."""
    csrc = os.path.join(L.ROOT, "hap_amd", "csrc")
    sources = {name: open(os.path.join(csrc, name)).read() for name in sorted(os.listdir(csrc))
               if name.endswith((".c", ".h", ".hip", ".hpp"))}
    for function in ("hap_region_needs_bytes", "hap_region_valid", "hap_region_geometry_valid"):
        defined = [name for name, text in sources.items() if re.search(r"\bint %s\(" % function, text)]
        assert defined == ["hap_region.h"], (function, defined)
    kernel = sources["snappy_decode.hip"]
    # one kernel blanks units, for one rectangle and for a rectangle per job, and it asks the header
    assert len(re.findall(r"__global__[^;{]*\bskip_units_kernel\(", kernel)) == 1
    body = kernel[kernel.index("void skip_units_kernel("):]
    body = body[: body.index("\n}\n")]
    assert "job_regions[u.job]" in body and "hap_region_needs_bytes(" in body and "hap_region_valid(" in body
    assert not re.search(r"/\s*4u?\b", body), "the kernel divides by the block size itself"
    for entry in ("hapgpu_k_skip_units", "hapgpu_k_skip_units_per_job"):
        assert re.search(r"\bint %s\(" % entry, sources["hapgpu_abi.h"]), entry
        assert re.search(r'extern "C" int %s\(' % entry, kernel), entry
    # the host: whether a frame's rectangle is one is hapb_region_fits' answer (hap_region_geometry_valid and the height)
    pictures = sources["hap_pictures.c"]
    assert "hapgpu_k_skip_units_per_job(" in sources["hap_batch.c"] and "decode_regions" in pictures
    fits = pictures[pictures.index("int hapb_region_fits("):]
    assert "hap_region_geometry_valid(" in fits[: fits.index("\n}\n")]
    assert "refused = !hapb_region_fits(&own, height)" in pictures
    api = sources["hap_api.c"]
    for name in NAMES:
        body = api[api.index("unsigned int %s(" % name):]
        assert "hapb_region_fits(" in body[: body.index("\n}\n")], name

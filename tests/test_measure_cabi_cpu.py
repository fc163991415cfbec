"""The measuring calls without a GPU: HapGpuMeasureTexture and HapGpuMeasureFrames are declared in the header, let out by
the export map, exported by the built library, bound by hap_amd._lib with the header's argument counts, and refuse a
missing context or a missing output before they touch a device or a client's array; HapGpuPictureError is 72 bytes in the
header's layout and in the ctypes mirror; hap_amd.psnr is plain arithmetic."""
import ctypes as C
import fnmatch
import inspect
import math
import os
import re
import subprocess

import pytest

import _libs as L

NAMES = {"HapGpuMeasureTexture": 11, "HapGpuMeasureFrames": 12}


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
        assert len(declared.group(1).split(",")) == count, name
        assert "HapGpuPictureError *" in declared.group(1) and "rowBytes" in declared.group(1), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name


def test_the_library_exports_nothing_outside_its_name_spaces():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(L.ROOT, "hap_amd", "libhap_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert "HapGpuMeasureTexture" in names and "HapGpuMeasureFrames" in names
    assert not [n for n in names if "measure" in n.lower() and not n.startswith("HapGpu")]


def test_the_struct_is_72_bytes_in_the_header_and_in_the_mirror(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    body = re.search(r"typedef struct HapGpuPictureError \{(.*?)\} HapGpuPictureError;", text, re.S)
    assert body
    fields = re.findall(r"unsigned long long (\w+)(?:\[(\d+)\])?;", body.group(1))
    assert fields == [("sse", "4"), ("sad", "4"), ("texels", "")]
    # (nine 8-byte members, naturally aligned: no padding on any ABI the library is built for)
    assert sum(int(n or 1) for _name, n in fields) * C.sizeof(C.c_ulonglong) == 72
    mirror = hap._lib.HapGpuPictureError
    assert C.sizeof(mirror) == 72
    assert [(n, C.sizeof(t)) for n, t in mirror._fields_] == [("sse", 32), ("sad", 32), ("texels", 8)]
    assert (mirror.sse.offset, mirror.sad.offset, mirror.texels.offset) == (0, 32, 64)


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name, sibling in (("HapGpuMeasureTexture", "HapGpuDecompressRGBA"), ("HapGpuMeasureFrames", "HapGpuDecodeFramesRGBA")):
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])       # (one line: words wrap anywhere)
        # the definition: d is the sibling call's byte, p the picture's; exact sums of squares and of absolute values
        for word in ("The definition, and the only one", sibling, "(d - p)^2", "|d - p|", "exact integers", "A = 255",
                     "width x height texels", "DEVICE", "16-byte aligned", "multiple of 16", "Bad_Arguments"):
            assert word in comment, (name, word)
        assert re.search(r"[Tt]wo calls give the same struct", comment), name
        for word in ("BC7", "BC6H", "A_RGTC1", "A8 pictures", "RGBA16F pictures", "scaled or rectangular", "ost pictures"):
            assert word in comment.split("Out of scope:")[1], (name, word)
    frames = text[: text.index("unsigned int HapGpuMeasureFrames(")]
    frames = re.sub(r"\s*\n \*\s*", " ", frames[frames.rindex("/*"):])
    for word in ("...OnDevices", "...Sequence", "HAPGPU_DECODE_BPTC_PICTURES", "all zero", "HOST arrays"):
        assert word in frames, word


def test_they_refuse_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    guard = 0x5A
    picture = (C.c_ubyte * 128)(*([guard] * 128))
    tex = (C.c_ubyte * 16)()
    error = (hap._lib.HapGpuPictureError * 2)()
    C.memset(error, guard, C.sizeof(error))
    # no context, with and without everything else; a context is not needed to see that there is no output
    assert lib.HapGpuMeasureTexture(None, tex, 16, L.FMT_DXT5, None, 0, 4, 4, picture, 16, error) == bad
    assert lib.HapGpuMeasureTexture(None, None, 0, L.FMT_DXT5, None, 0, 4, 4, None, 16, None) == bad
    fake = C.c_void_p(0x5A5A5A50)                     # (never looked into: the missing output is seen first)
    assert lib.HapGpuMeasureTexture(fake, tex, 16, L.FMT_DXT5, None, 0, 4, 4, picture, 16, None) == bad
    frames = (C.c_void_p * 2)(C.addressof(tex), 0x5A5A)
    lens = (C.c_ulong * 2)(16, 0x5A5A)
    pictures = (C.c_void_p * 2)(C.addressof(picture), 0x5A5A)
    res = (C.c_uint * 2)(77, 78)
    assert lib.HapGpuMeasureFrames(None, 1, frames, lens, 1, pictures, 4, 4, 16, error, res, 0) == bad
    assert lib.HapGpuMeasureFrames(None, 1, None, None, 1, None, 4, 4, 16, None, None, 0) == bad
    assert list(res) == [77, 78]
    # no errors array: the whole call is refused, the frame's result says so, the entry behind it stays
    assert lib.HapGpuMeasureFrames(fake, 1, frames, lens, 1, pictures, 4, 4, 16, None, res, 0) == bad
    assert list(res) == [bad, 78]
    assert lib.HapGpuMeasureFrames(fake, 1, frames, lens, 1, pictures, 4, 4, 16, None, None, 0) == bad
    assert bytes(error) == bytes([guard]) * C.sizeof(error) and bytes(picture) == bytes([guard]) * 128
    assert list(frames) == [C.addressof(tex), 0x5A5A] and list(lens) == [16, 0x5A5A]
    assert list(pictures) == [C.addressof(picture), 0x5A5A] and bytes(tex) == bytes(16)


def test_the_python_methods_exist(hap):
    want = {"measure_texture": ["texture", "texture_format", "width", "height", "picture", "alpha", "row_bytes"],
            "measure_frames": ["frames", "frame_bytes", "texture_count", "pictures", "width", "height", "row_bytes",
                               "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.measure_texture)
    assert [sig.parameters[p].default for p in ("alpha", "row_bytes")] == [None, None]
    sig = inspect.signature(hap.Context.measure_frames)
    assert [sig.parameters[p].default for p in ("row_bytes", "flags")] == [None, 0]
    with pytest.raises(ValueError, match="one picture per frame"):
        hap.Context.measure_frames(None, [bytes(16)], [16], 1, [], 4, 4)
    e = hap.PictureError((1, 2, 3, 4), (5, 6, 7, 8), 9)
    assert (e.sse, e.sad, e.texels) == ((1, 2, 3, 4), (5, 6, 7, 8), 9)
    assert e == hap.PictureError((1, 2, 3, 4), (5, 6, 7, 8), 9) and e != hap.PictureError()


def test_psnr_on_known_values(hap):
    assert hap.psnr(0, 16) == math.inf
    assert hap.psnr(0, 0) == math.inf
    # every texel off by the peak: 0 dB; off by one: 20 log10(255)
    assert hap.psnr(255 * 255 * 16, 16) == 0.0
    assert hap.psnr(16, 16) == pytest.approx(20.0 * math.log10(255.0), abs=1e-12)
    # a mean squared error of 100 is 28.13 dB (10 log10(650.25))
    assert hap.psnr(100 * 4096, 4096) == pytest.approx(28.1308036087, abs=1e-9)
    # another peak; ten times the error is ten dB less
    assert hap.psnr(7, 7, peak=1.0) == 0.0
    assert hap.psnr(10, 1) == pytest.approx(hap.psnr(1, 1) - 10.0, abs=1e-12)
    # sums beyond 2^32, as whole streams give them
    assert hap.psnr(1 << 40, 1 << 40) == pytest.approx(20.0 * math.log10(255.0), abs=1e-12)
    assert hap.PictureError((4, 4, 4, 0), (0,) * 4, 4).psnr() == pytest.approx(20.0 * math.log10(255.0), abs=1e-12)

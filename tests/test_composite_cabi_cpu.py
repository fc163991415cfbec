"""The compositing calls without a GPU: HapGpuCompositeTextures and HapGpuCompositeFrames are declared in the header with
their argument counts, let out by the export map, exported by the built library, bound by hap_amd._lib with the same
counts, and refuse what is wrong with a call whatever its layers hold before they look at the context, a device or a
client's picture; the header states the definition and what is out of scope."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

import _composite as K
import _libs as L

NAMES = {"HapGpuCompositeTextures": 13, "HapGpuCompositeFrames": 14}
GUARD = 0x5A


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def header():
    return open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()


def test_the_two_functions_are_declared_listed_exported_and_bound(hap):
    text = header()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
        assert declared, name
        assert len(declared.group(1).split(",")) == count, name
        for word in ("opacities", "background", "rowBytes"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    assert re.search(r"#define HAPGPU_COMPOSITE_MAX_LAYERS 16u\b", text)
    assert hap.COMPOSITE_MAX_LAYERS == K.MAX_LAYERS == 16


def test_the_library_exports_nothing_outside_its_name_spaces():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(L.ROOT, "hap_amd", "libhap_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert "HapGpuCompositeTextures" in names and "HapGpuCompositeFrames" in names
    assert not [n for n in names if "composite" in n.lower() and not n.startswith("HapGpu")]


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = header()
    for name, sibling in (("HapGpuCompositeTextures", "HapGpuDecompressRGBA"), ("HapGpuCompositeFrames", "HapGpuDecodeFramesRGBA")):
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])       # (one line: words wrap anywhere)
        comment = re.sub(r" +", " ", comment)                                       # (and formulas are aligned in columns)
        # the three formulas, rdiv255, the canvas and the layers
        for word in ("The definition, and the only one", sibling, "a = rdiv255(As * o)", "Cd = rdiv255(Cs * a + Cd * (255 - a))",
                     "Ad = a + rdiv255(Ad * (255 - a))", "t = x + 128; (t + (t >> 8)) >> 8", "integer nearest to x / 255",
                     "premultiplied", "straight alpha", "As = 255", "a = 255 replaces", "a = 0 leaves", "byte for byte",
                     "multiple of 16", "16-byte aligned", "row by row", "Bad_Arguments", "Internal_Error",
                     "HAPGPU_COMPOSITE_MAX_LAYERS", "0, 0, 0, 255", "all 255"):
            assert word in comment, (name, word)
        assert re.search(r"[Tt]wo calls give the same bytes", comment), name
        scope = comment.split("Out of scope:")[1]
        for word in ("other sizes", "at an offset", "scaled or rectangular", 'other than "over"', "existing picture",
                     "Hap R", "Hap HDR", "Hap Alpha-Only", "planar or RGBA16F", "hidden under an opaque"):
            assert word in scope, (name, word)
    frames = text[: text.index("unsigned int HapGpuCompositeFrames(")]
    frames = re.sub(r"\s*\n \*\s*", " ", frames[frames.rindex("/*"):])
    frames = re.sub(r" +", " ", frames)
    for word in ("...OnDevices", "...Sequence", "HAPGPU_DECODE_BPTC_PICTURES", "HOST array", "f * layerCount + l",
                 "if and only if", "first failure", "other than 1 or 2", "no device touched", "4 GiB", "32768"):
        assert word in frames, word


def test_the_frames_call_refuses_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    picture = (C.c_ubyte * 256)(*([GUARD] * 256))
    frame = (C.c_ubyte * 16)()
    fake = C.c_void_p(0x5A5A5A50)                     # (never looked into: what is wrong is seen first)

    def call(context, layers, counts, width, results, frames=1, row=None, inputs=True, pictures=True):
        n = frames * layers
        ptrs = (C.c_void_p * max(1, n))(*([C.addressof(frame)] * n))
        lens = (C.c_ulong * max(1, n))(*([16] * n))
        pics = (C.c_void_p * frames)(*([C.addressof(picture)] * frames))
        tc = (C.c_uint * max(1, layers))(*counts) if counts is not None else None
        return lib.HapGpuCompositeFrames(context, frames, layers, ptrs if inputs else None, lens, tc, None, None,
                                         pics if pictures else None, width, 4, width * 4 if row is None else row, results, 0)

    def fresh(n):
        return (C.c_uint * (n + 1))(*([77] * (n + 1)))

    # a NULL context: refused, and the results are left alone (nothing says whose they are)
    res = fresh(2)
    assert call(None, 1, None, 4, res, frames=2) == bad and list(res) == [77] * 3
    # a NULL results: nothing to set
    assert call(fake, 1, None, 4, None) == bad
    # layerCount 0: no entry to set
    res = fresh(2)
    assert call(fake, 0, None, 4, res, frames=2) == bad and list(res) == [77] * 3
    # layerCount 17; a width of 6; a textureCounts entry of 3; rows short or off 16; a missing array: every entry set,
    # the one behind them left alone
    for name, kw in (("17 layers", dict(layers=17, counts=None, width=4)), ("width 6", dict(layers=2, counts=None, width=6)),
                     ("count 3", dict(layers=2, counts=[1, 3], width=4)), ("count 0", dict(layers=2, counts=[0, 1], width=4)),
                     ("short rows", dict(layers=2, counts=None, width=8, row=16)),
                     ("rows off 16", dict(layers=2, counts=None, width=4, row=24)),
                     ("no inputs", dict(layers=2, counts=None, width=4, inputs=False)),
                     ("no pictures", dict(layers=2, counts=None, width=4, pictures=False))):
        n = 2 * kw["layers"]
        res = fresh(n)
        assert call(fake, results=res, frames=2, **kw) == bad, name
        assert list(res) == [bad] * n + [77], name
    assert bytes(picture) == bytes([GUARD]) * 256 and bytes(frame) == bytes(16)


def test_the_textures_call_refuses_before_touching_a_device(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    picture = (C.c_ubyte * 256)(*([GUARD] * 256))
    tex = (C.c_ubyte * 16)()
    fake = C.c_void_p(0x5A5A5A50)

    def call(context, layers, width, row=None, textures=True, rgba=True):
        n = max(1, layers)
        ptrs = (C.c_void_p * n)(*([C.addressof(tex)] * n))
        lens = (C.c_ulong * n)(*([16] * n))
        fmts = (C.c_uint * n)(*([L.FMT_DXT5] * n))
        return lib.HapGpuCompositeTextures(context, layers, ptrs if textures else None, lens, fmts, None, None, None, None,
                                           width, 4, picture if rgba else None, width * 4 if row is None else row)

    assert call(None, 1, 4) == bad
    assert call(fake, 0, 4) == bad
    assert call(fake, 17, 4) == bad
    assert call(fake, 1, 6) == bad
    assert call(fake, 1, 8, row=16) == bad
    assert call(fake, 1, 4, row=24) == bad
    assert call(fake, 1, 4, textures=False) == bad
    assert call(fake, 1, 4, rgba=False) == bad
    assert bytes(picture) == bytes([GUARD]) * 256 and bytes(tex) == bytes(16)


def test_the_python_methods_exist(hap):
    want = {"composite_textures": ["layers", "width", "height", "opacities", "background", "rgba", "row_bytes"],
            "composite_frames": ["frames", "frame_bytes", "texture_counts", "rgba_frames", "width", "height", "opacities",
                                 "background", "row_bytes", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.composite_textures)
    assert [sig.parameters[p].default for p in ("opacities", "background", "rgba", "row_bytes")] == [None] * 4
    sig = inspect.signature(hap.Context.composite_frames)
    assert [sig.parameters[p].default for p in ("opacities", "background", "row_bytes", "flags")] == [None, None, None, 0]
    with pytest.raises(ValueError, match="one picture per output frame"):
        hap.Context.composite_frames(None, [[bytes(16)]], None, None, [], 4, 4)
    with pytest.raises(ValueError, match="same number of layers"):
        hap.Context.composite_frames(None, [[bytes(16)], [bytes(16), bytes(16)]], None, None, [None, None], 4, 4)

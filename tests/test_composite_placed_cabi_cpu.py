"""The placed compositing calls without a GPU: HapGpuCompositeTexturesPlaced and HapGpuCompositeFramesPlaced are declared
in the header with their argument counts, exported by the built library and bound by hap_amd._lib with the same counts;
the header's comments state the definition -- coverage, source texel, clipping, the NULL default and the refusals; and
every refusal of a placement or a layer size is Bad_Arguments with every result set, before a context, a device or a
client's picture is looked at."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _composite_placed as KP
import _libs as L

NAMES = {"HapGpuCompositeTexturesPlaced": 16, "HapGpuCompositeFramesPlaced": 17}
GUARD = 0x5A


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def header():
    return open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()


def comment_of(text, name):
    comment = text[: text.index("unsigned int %s(" % name)]
    comment = re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])           # (one line: words wrap anywhere)
    return re.sub(r" +", " ", comment)                                              # (and formulas are aligned in columns)


def test_the_two_functions_are_declared_exported_and_bound(hap):
    text = header()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
        assert declared, name
        assert len(declared.group(1).split(",")) == count, name
        for word in ("layerWidths", "layerHeights", "const HapGpuPlacement *placements", "opacities", "background", "rowBytes"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    # declared after the two calls they extend, which stay as they are
    assert text.index("unsigned int HapGpuCompositeFrames(") < text.index("typedef struct HapGpuPlacement {") < \
        text.index("unsigned int HapGpuCompositeTexturesPlaced(") < text.index("unsigned int HapGpuCompositeFramesPlaced(")
    # the struct, field for field, and its binding
    struct = re.search(r"typedef struct HapGpuPlacement \{(.*?)\} HapGpuPlacement;", text, re.S).group(1)
    assert re.search(r"unsigned int srcX, srcY, width, height;", struct) and re.search(r"\bint dstX, dstY;", struct)
    fields = hap._lib.HapGpuPlacement._fields_
    assert [n for n, _t in fields] == ["srcX", "srcY", "width", "height", "dstX", "dstY"]
    assert [t for _n, t in fields] == [C.c_uint] * 4 + [C.c_int] * 2 and C.sizeof(hap._lib.HapGpuPlacement) == 24


def test_the_header_states_the_definition():
    text = header()
    for name, sibling, base in (("HapGpuCompositeTexturesPlaced", "HapGpuDecompressRGBA", "HapGpuCompositeTextures"),
                                ("HapGpuCompositeFramesPlaced", "HapGpuDecodeFramesRGBA", "HapGpuCompositeFrames")):
        comment = comment_of(text, name)
        for word in ("The definition, and the only one", sibling, base + "'",
                     # coverage and the source texel
                     "dstX <= x < dstX + width and dstY <= y < dstY + height", "(srcX + x - dstX, srcY + y - dstY)",
                     "three formulas apply unchanged", "a = rdiv255(As * o)", "Cd = rdiv255(Cs * a + Cd * (255 - a))",
                     "Ad = a + rdiv255(Ad * (255 - a))",
                     # what is not covered, clipping, the default
                     "not covered is left as the canvas has it", "falls outside the canvas is clipped",
                     "wholly outside contributes nothing and is no error", "placements == NULL means every layer whole at (0, 0)",
                     "{0, 0, layerWidths[l], layerHeights[l], 0, 0}", "byte for byte",
                     # the refusals
                     "Bad_Arguments", "not a multiple of 4", "width or height of 0", "rectangle that leaves its layer",
                     "|dstX| or |dstY| above 1 << 20", "layer size that is 0 or no multiple of 4", "refuses already",
                     "no device touched", "multiples of 4"):
            assert word in comment, (name, word)
        assert re.search(r"[Tt]wo calls give the same bytes", comment), name
        scope = comment.split("Out of scope:")[1]
        for word in ("off the block grid", "scaled or rotated", 'other than "over"', "existing picture", "Hap R", "Hap HDR",
                     "Hap Alpha-Only", "planar, NV12 or encoded"):
            assert word in scope, (name, word)
    frames = comment_of(text, "HapGpuCompositeFramesPlaced")
    for word in ("placements[f * layerCount + l]", "the same in every output frame", "exactly layerWidths[l] x layerHeights[l]",
                 "RGTC1 plane of the same size", "that output frame is untouched", "decodes every layer's whole frame",
                 "if and only if", "every result set", "4 GiB", "32768", "...OnDevices", "...Sequence"):
        assert word in frames, word
    struct = text[: text.index("typedef struct HapGpuPlacement {")]
    assert "multiples of 4" in struct[struct.rindex("/*"):]


# what the definition refuses of a placement of a 32 x 32 layer, and of a layer's size: (name, placement, layer size)
WHOLE = (0, 0, 32, 32, 0, 0)
REFUSED = [("%s off the grid by %d" % (field, off), tuple(v + (off if i == at else 0) for i, v in enumerate((4, 4, 8, 8, 8, -8))),
            (32, 32))
           for at, field in enumerate(("srcX", "srcY", "width", "height", "dstX", "dstY")) for off in (1, 2, 3)]
REFUSED += [("width 0", (0, 0, 0, 4, 0, 0), (32, 32)), ("height 0", (0, 0, 4, 0, 0, 0), (32, 32)),
            ("leaves the layer rightwards", (28, 0, 8, 4, 0, 0), (32, 32)), ("leaves the layer downwards", (0, 28, 4, 8, 0, 0), (32, 32)),
            ("begins behind the layer", (32, 0, 4, 4, 0, 0), (32, 32)), ("wider than the layer", (0, 0, 36, 32, 0, 0), (32, 32)),
            ("a sum that wraps", (0xFFFFFFFC, 0, 8, 4, 0, 0), (32, 32)), ("a height that wraps", (0, 8, 4, 0xFFFFFFFC, 0, 0), (32, 32)),
            ("dstX above 1 << 20", (0, 0, 4, 4, (1 << 20) + 4, 0), (32, 32)), ("dstY above 1 << 20", (0, 0, 4, 4, 0, (1 << 20) + 4), (32, 32)),
            ("dstX below -(1 << 20)", (0, 0, 4, 4, -(1 << 20) - 4, 0), (32, 32)), ("dstY below -(1 << 20)", (0, 0, 4, 4, 0, -(1 << 20) - 4), (32, 32)),
            ("dstX the least int", (0, 0, 4, 4, -(1 << 31), 0), (32, 32)),
            ("layer width 0", None, (0, 32)), ("layer height 0", None, (32, 0)), ("layer width 30", None, (30, 32)),
            ("layer height 34", None, (32, 34)), ("layer width 0, placed", (0, 0, 4, 4, 0, 0), (0, 32))]
ACCEPTED = [WHOLE, (28, 28, 4, 4, 1 << 20, -(1 << 20)), (0, 0, 4, 4, -(1 << 20), 1 << 20), (4, 8, 28, 24, -4, 4)]


def test_the_refusals_are_the_definitions():
    """(the table above against tests/_composite_placed.py's form of the rules)"""
    for name, placement, size in REFUSED:
        bad_size = size[0] == 0 or size[1] == 0 or size[0] % 4 or size[1] % 4
        assert bad_size or not KP.valid(placement, size), name
    for placement in ACCEPTED:
        assert KP.valid(placement, (32, 32)), placement


def placement_array(hap, placements):
    return (hap._lib.HapGpuPlacement * len(placements))(*[hap._lib.HapGpuPlacement(*p) for p in placements])


@pytest.mark.parametrize("context", (None, 0x5A5A5A50), ids=("null_context", "fake_context"))
def test_the_frames_call_refuses_before_touching_a_device(hap, context):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    picture = (C.c_ubyte * 256)(*([GUARD] * 256))
    frame = (C.c_ubyte * 16)()
    context = C.c_void_p(context) if context else None      # (the fake one is never looked into: what is wrong is seen first)
    frames, layers = 2, 2
    n = frames * layers

    def call(placements, sizes, results, widths=True, heights=True, canvas=(4, 4), row=None, counts=None, layer_count=layers):
        m = frames * layer_count
        ptrs = (C.c_void_p * m)(*([C.addressof(frame)] * m))
        lens = (C.c_ulong * m)(*([16] * m))
        pics = (C.c_void_p * frames)(*([C.addressof(picture)] * frames))
        lws = (C.c_uint * layer_count)(*[sizes[l % len(sizes)][0] for l in range(layer_count)])
        lhs = (C.c_uint * layer_count)(*[sizes[l % len(sizes)][1] for l in range(layer_count)])
        tc = (C.c_uint * layer_count)(*counts) if counts is not None else None
        places = placement_array(hap, placements) if placements is not None else None
        return lib.HapGpuCompositeFramesPlaced(context, frames, layer_count, ptrs, lens, tc, lws if widths else None,
                                               lhs if heights else None, places, None, None, pics, canvas[0], canvas[1],
                                               canvas[0] * 4 if row is None else row, results, 0)

    def fresh(m=n):
        return (C.c_uint * (m + 1))(*([77] * (m + 1)))

    # a NULL results: nothing to set
    assert call([WHOLE] * n, [(32, 32)], None) == bad
    # every refusal of the definition, as the last placement of the call (the first three are in order) or as the second
    # layer's size: every entry set, the one behind them left alone
    for name, placement, size in REFUSED:
        res = fresh()
        placements = None if placement is None else [WHOLE] * (n - 1) + [placement]
        assert call(placements, [(32, 32), size], res) == bad, name
        assert list(res) == [bad] * n + [77], name
    # ... and as the first placement
    res = fresh()
    assert call([(0, 0, 36, 32, 0, 0)] + [WHOLE] * (n - 1), [(32, 32)], res) == bad and list(res) == [bad] * n + [77]
    # no layer sizes at all
    for kw in (dict(widths=False), dict(heights=False)):
        res = fresh()
        assert call(None, [(32, 32)], res, **kw) == bad and list(res) == [bad] * n + [77], kw
    # everything HapGpuCompositeFrames refuses already: a canvas off the grid, rows short or off 16, a count of 3, 17 layers
    for name, kw in (("width 6", dict(canvas=(6, 4))), ("height 0", dict(canvas=(4, 0))), ("short rows", dict(canvas=(8, 4), row=16)),
                     ("rows off 16", dict(row=24)), ("count 3", dict(counts=[1, 3])), ("count 0", dict(counts=[0, 1]))):
        res = fresh()
        assert call([WHOLE] * n, [(32, 32)], res, **kw) == bad, name
        assert list(res) == [bad] * n + [77], name
    res = fresh(frames * 17)
    assert call(None, [(32, 32)], res, layer_count=17) == bad and list(res) == [bad] * (frames * 17) + [77]
    assert bytes(picture) == bytes([GUARD]) * 256 and bytes(frame) == bytes(16)
    # what is in order gets as far as the context: a NULL one is refused with the results left alone, as
    # HapGpuCompositeFrames leaves them
    if context is None:
        for placement in ACCEPTED:
            res = fresh()
            assert call([placement] * n, [(32, 32)], res) == bad and list(res) == [77] * (n + 1), placement
        assert bytes(picture) == bytes([GUARD]) * 256


@pytest.mark.parametrize("context", (None, 0x5A5A5A50), ids=("null_context", "fake_context"))
def test_the_textures_call_refuses_before_touching_a_device(hap, context):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    picture = (C.c_ubyte * 256)(*([GUARD] * 256))
    tex = (C.c_ubyte * 1024)()
    context = C.c_void_p(context) if context else None
    layers = 2

    def call(placements, sizes, widths=True, heights=True, canvas=(4, 4), row=None, layer_count=layers, textures=True, rgba=True):
        ptrs = (C.c_void_p * layer_count)(*([C.addressof(tex)] * layer_count))
        lens = (C.c_ulong * layer_count)(*([1024] * layer_count))
        fmts = (C.c_uint * layer_count)(*([L.FMT_DXT5] * layer_count))
        lws = (C.c_uint * layer_count)(*[sizes[l % len(sizes)][0] for l in range(layer_count)])
        lhs = (C.c_uint * layer_count)(*[sizes[l % len(sizes)][1] for l in range(layer_count)])
        places = placement_array(hap, placements) if placements is not None else None
        return lib.HapGpuCompositeTexturesPlaced(context, layer_count, ptrs if textures else None, lens, fmts, None, None,
                                                 lws if widths else None, lhs if heights else None, places, None, None,
                                                 canvas[0], canvas[1], picture if rgba else None,
                                                 canvas[0] * 4 if row is None else row)

    for name, placement, size in REFUSED:
        assert call(None if placement is None else [WHOLE, placement], [(32, 32), size]) == bad, name
    assert call([(0, 0, 36, 32, 0, 0), WHOLE], [(32, 32)]) == bad
    assert call(None, [(32, 32)], widths=False) == bad and call(None, [(32, 32)], heights=False) == bad
    assert call([WHOLE] * 2, [(32, 32)], canvas=(6, 4)) == bad and call([WHOLE] * 2, [(32, 32)], canvas=(8, 4), row=16) == bad
    assert call([WHOLE] * 2, [(32, 32)], row=24) == bad and call(None, [(32, 32)], layer_count=17) == bad
    assert call([WHOLE] * 2, [(32, 32)], textures=False) == bad and call([WHOLE] * 2, [(32, 32)], rgba=False) == bad
    if context is None:
        for placement in ACCEPTED:
            assert call([placement] * 2, [(32, 32)]) == bad
    assert bytes(picture) == bytes([GUARD]) * 256 and bytes(tex) == bytes(1024)


def test_the_python_methods_exist(hap):
    want = {"composite_textures_placed": ["layers", "layer_sizes", "width", "height", "placements", "opacities", "background",
                                          "rgba", "row_bytes"],
            "composite_frames_placed": ["frames", "frame_bytes", "texture_counts", "layer_sizes", "rgba_frames", "width",
                                        "height", "placements", "opacities", "background", "row_bytes", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["placements"].default is None, name
    with pytest.raises(ValueError, match="one picture per output frame"):
        hap.Context.composite_frames_placed(None, [[bytes(16)]], None, None, [(4, 4)], [], 4, 4)
    with pytest.raises(ValueError, match="one size per layer"):
        hap.Context.composite_frames_placed(None, [[bytes(16)]], None, None, [(4, 4), (4, 4)], [None], 4, 4)
    with pytest.raises(ValueError, match="one placement per output frame and layer"):
        hap.Context.composite_frames_placed(None, [[bytes(16)]], None, None, [(4, 4)], [None], 4, 4, placements=[[WHOLE, WHOLE]])
    with pytest.raises(ValueError, match="six numbers"):
        hap.Context.composite_textures_placed(None, [(bytes(16), L.FMT_DXT5, None)], [(4, 4)], 4, 4, placements=[(0, 0, 4, 4)])

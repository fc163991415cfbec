"""The compositing calls that end in textures and frames, without a GPU: HapGpuCompositeTexturesEncoded and
HapGpuCompositeFramesEncoded are declared in the header with their argument counts, exported by the built library -- and
nothing else new is --, and bound by hap_amd._lib with the same counts; the header's comments hold the definition and
the out-of-scope list; and what is wrong with a call itself is Bad_Arguments with every entry of both result arrays set,
before a context, a device or a client's buffer is looked at."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

import _libs as L

NAMES = {"HapGpuCompositeTexturesEncoded": 19, "HapGpuCompositeFramesEncoded": 24}
GUARD = 0x5A
WHOLE = (0, 0, 32, 32, 0, 0)


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
    return re.sub(r" +", " ", comment)


def arguments(text, name):
    declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
    assert declared, name
    return [a.strip() for a in declared.group(1).split(",")]


def kind(argument):
    """what a declared argument is to ctypes: 'p' a pointer of any kind, else the integer type's name"""
    if "*" in argument:
        return "p"
    return "ulong" if argument.startswith("unsigned long") else "uint"


def test_the_two_functions_are_declared_exported_and_bound(hap):
    text = header()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        args = arguments(text, name)
        assert len(args) == count, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        # the prototype in _lib.py, argument for argument
        assert len(bound.argtypes) == count, name
        for at, (arg, ctype) in enumerate(zip(args, bound.argtypes)):
            got = "p" if (ctype is C.c_void_p or hasattr(ctype, "contents")) else {C.c_uint: "uint", C.c_ulong: "ulong"}[ctype]
            assert got == kind(arg), (name, at, arg, ctype)
            if "HapGpuPlacement" in arg:
                assert ctype._type_ is hap._lib.HapGpuPlacement, name
    # the input side is the placed calls', the output side the transcode calls'
    for word in ("layerWidths", "layerHeights", "const HapGpuPlacement *placements", "opacities", "background"):
        assert all(any(word in a for a in arguments(text, n)) for n in NAMES), word
    textures = arguments(text, "HapGpuCompositeTexturesEncoded")
    assert [a.split()[-1].lstrip("*") for a in textures[-5:]] == ["count", "outputFormats", "outputs", "outputsBytes", "outputsBytesUsed"]
    assert [a.split()[-1].lstrip("*") for a in textures[-5:]] == \
        [a.split()[-1].lstrip("*") for a in arguments(text, "HapGpuTranscodeTexture")[-5:]]
    frames = [a.split()[-1].lstrip("*") for a in arguments(text, "HapGpuCompositeFramesEncoded")]
    assert frames[-11:] == ["count", "textureFormats", "compressors", "chunkCounts", "outputBuffers", "outputBuffersBytes",
                            "outputBuffersBytesUsed", "layerResults", "results", "decodeFlags", "encodeFlags"]
    assert not any("rowBytes" in a or "rgba" in a for n in NAMES for a in arguments(text, n))
    assert text.index("unsigned int HapGpuCompositeFramesPlaced(") < text.index("unsigned int HapGpuCompositeTexturesEncoded(") < \
        text.index("unsigned int HapGpuCompositeFramesEncoded(")


def test_nothing_else_new_is_exported():
    """what the library exports is what the two public headers declare, these two among it"""
    from hap_amd.build import build
    build()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(L.ROOT, "hap_amd", "libhap_amd.so")], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if " T " in line}
    declared = set()
    for name in ("hap.h", "hap_gpu.h", "hap_sequence.h"):
        text = open(os.path.join(L.ROOT, "include", name)).read()
        declared |= set(re.findall(r"\b((?:HapGpu|HapSequence|Hap)[A-Z][A-Za-z0-9]*)\s*\(", text))
    composite = {n for n in exported if n.startswith("HapGpuComposite")}
    assert composite == {"HapGpuCompositeTextures", "HapGpuCompositeFrames", "HapGpuCompositeTexturesPlaced",
                         "HapGpuCompositeFramesPlaced"} | set(NAMES)
    assert {n for n in exported if n.startswith(("HapGpu", "HapSequence"))} <= declared
    assert not any("composite_encode" in n for n in exported)      # (the kernel's launcher and the host side stay inside)


def test_the_header_states_the_definition():
    text = header()
    textures = comment_of(text, "HapGpuCompositeTexturesEncoded")
    frames = comment_of(text, "HapGpuCompositeFramesEncoded")
    for word in ("The definition, and the only one", "byte for byte", "HapGpuCompressRGBA", "HapGpuCompositeTexturesPlaced writes",
                 "rowBytes = width * 4"):
        assert word in textures, word
    for word in ("The definition, and the only one", "byte for byte", "HapGpuEncodeFramesRGBA", "HapGpuCompositeFramesPlaced writes",
                 "the same layers, placements, opacities and background", "HAPGPU_ENCODE_BPTC_BLOCKS",
                 "HAPGPU_ENCODE_REFINE_ENDPOINTS", "ignored", "layerResults[f * layerCount + l]", "if and only if all its layers are No_Error",
                 "first failing layer's code", "outputBuffersBytesUsed[f] is 0", "untouched", "Buffer_Too_Small",
                 "does not disturb its neighbours", "before the context is looked at", "4 GiB", "32768",
                 "every entry of results and of layerResults set"):
        assert word in frames, word
    for name, comment in (("textures", textures), ("frames", frames)):
        for word in ("canvas bytes go to the encoder as they are", "premultiplied", "opaque background", "result is opaque",
                     "RGB_DXT1", "RGBA_DXT5", "YCoCg_DXT5 then A_RGTC1", "Bad_Arguments", "count of 0 or above 2",
                     "any other destination set", "65535 block rows", "no device touched"):
            assert word in comment, (name, word)
        assert re.search(r"[Tt]wo calls give the same bytes", comment), name
        scope = comment.split("Out of scope:")[1]
        for word in ("scaled or rotated layers", "BC7", "BC6H", "Alpha-Only", "layers or destinations", "refined end points",
                     "NV12 or planar output", "un-premultiplying"):
            assert word in scope, (name, word)
    scope = frames.split("Out of scope:")[1]
    for word in ("...OnDevices", "...Sequence", "...Begin"):
        assert word in scope, word
    # the comments this closes a gap of stay as they were
    for name in ("HapGpuCompositeTexturesPlaced", "HapGpuCompositeFramesPlaced"):
        assert "planar, NV12 or encoded output" in comment_of(text, name).split("Out of scope:")[1]


def placement_array(hap, placements):
    return (hap._lib.HapGpuPlacement * len(placements))(*[hap._lib.HapGpuPlacement(*p) for p in placements])


# what is wrong with a frames call itself: (name, keyword arguments of call() below)
OFF_GRID = [("%s off the grid by %d" % (field, off), dict(last=tuple(v + (off if i == at else 0) for i, v in enumerate((4, 4, 8, 8, 8, -8)))))
            for at, field in enumerate(("srcX", "srcY", "width", "height", "dstX", "dstY")) for off in (1, 2, 3)]
REFUSED = OFF_GRID + [
    ("count 3", dict(formats=[L.FMT_YCOCG, L.FMT_RGTC1, L.FMT_DXT1])),
    ("count 0", dict(formats=[])),
    ("the pair the other way round", dict(formats=[L.FMT_RGTC1, L.FMT_YCOCG])),
    ("YCoCg then DXT5", dict(formats=[L.FMT_YCOCG, L.FMT_DXT5])),
    ("a BC7 destination", dict(formats=[L.FMT_BC7])),
    ("a BC6H destination", dict(formats=[L.FMT_BC6U])),
    ("a lone RGTC1 destination", dict(formats=[L.FMT_RGTC1])),
    ("a compressor nobody knows", dict(compressors=[7])),
    ("a chunk count of 0", dict(chunks=[0])),
    # everything the placed call refuses already
    ("a placement that leaves its layer", dict(last=(28, 0, 8, 4, 0, 0))),
    ("dstX above 1 << 20", dict(last=(0, 0, 4, 4, (1 << 20) + 4, 0))),
    ("a layer width of 30", dict(sizes=[(32, 32), (30, 32)], placements=False)),
    ("no layer widths", dict(widths=False)), ("no layer heights", dict(heights=False)),
    ("a canvas width of 6", dict(canvas=(6, 4))), ("a canvas height of 0", dict(canvas=(4, 0))),
    ("a texture count of 3", dict(counts=[1, 3])),
    ("17 layers", dict(layer_count=17)), ("no layers", dict(layer_count=0)),
    ("more than 65535 block rows", dict(canvas=(4, 65536 * 4))),
    ("no inputs", dict(inputs=False)), ("no outputs", dict(outputs=False)), ("no compressors", dict(compressors=None)),
    ("no chunk counts", dict(chunks=None)), ("no formats", dict(formats=None)), ("no used", dict(used=False)),
]


@pytest.mark.parametrize("context", (None, 0x5A5A5A50), ids=("null_context", "fake_context"))
def test_the_frames_call_refuses_before_touching_a_device(hap, context):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    out = (C.c_ubyte * 256)(*([GUARD] * 256))
    frame = (C.c_ubyte * 16)()
    context = C.c_void_p(context) if context else None      # (the fake one is never looked into: what is wrong is seen first)
    frames = 2

    def arr(values):
        return None if values is None else (C.c_uint * max(1, len(values)))(*values)

    def call(layer_results, results, last=WHOLE, sizes=((32, 32),), placements=True, widths=True, heights=True, canvas=(4, 4),
             counts=None, layer_count=2, formats=(L.FMT_DXT1,), compressors=(L.COMP_SNAPPY,), chunks=(1,), inputs=True,
             outputs=True, used=True):
        m = frames * layer_count
        ptrs = (C.c_void_p * max(1, m))(*([C.addressof(frame)] * m))
        lens = (C.c_ulong * max(1, m))(*([16] * m))
        outs = (C.c_void_p * frames)(*([C.addressof(out)] * frames))
        caps = (C.c_ulong * frames)(*([256] * frames))
        taken = (C.c_ulong * (frames + 1))(*([77] * (frames + 1)))
        lws = (C.c_uint * max(1, layer_count))(*[sizes[l % len(sizes)][0] for l in range(layer_count)])
        lhs = (C.c_uint * max(1, layer_count))(*[sizes[l % len(sizes)][1] for l in range(layer_count)])
        places = placement_array(hap, [WHOLE] * (m - 1) + [last]) if placements and m else None
        count = len(formats) if formats is not None else 1
        r = lib.HapGpuCompositeFramesEncoded(context, frames, layer_count, ptrs if inputs else None, lens, arr(counts),
                                             lws if widths else None, lhs if heights else None, places, None, None,
                                             canvas[0], canvas[1], count, arr(formats),
                                             arr(list(compressors) * max(1, count) if compressors is not None else None),
                                             arr(list(chunks) * max(1, count) if chunks is not None else None),
                                             outs if outputs else None, caps, taken if used else None, layer_results,
                                             results, 0, 0)
        assert list(taken) == [77] * (frames + 1)
        return r

    def fresh(m):
        return (C.c_uint * (m + 1))(*([77] * (m + 1)))

    for name, kw in REFUSED:
        m = frames * kw.get("layer_count", 2)
        layer_results, results = fresh(m), fresh(frames)
        assert call(layer_results, results, **kw) == bad, name
        assert list(layer_results) == [bad] * m + [77], name
        assert list(results) == [bad] * frames + [77], name
    # a NULL results or layerResults: a call wrong in itself, and the array there is is set
    layer_results, results = fresh(4), fresh(frames)
    assert call(None, results) == bad and list(results) == [bad] * frames + [77]
    assert call(layer_results, None) == bad and list(layer_results) == [bad] * 4 + [77]
    assert call(None, None) == bad
    assert bytes(out) == bytes([GUARD]) * 256 and bytes(frame) == bytes(16)
    # what is in order gets as far as the context: a NULL one is refused with the results left alone
    if context is None:
        for kw in (dict(), dict(formats=[L.FMT_YCOCG, L.FMT_RGTC1]), dict(formats=[L.FMT_DXT5], compressors=(L.COMP_NONE,)),
                   dict(last=(28, 28, 4, 4, 1 << 20, -(1 << 20))), dict(canvas=(4, 65535 * 4))):
            layer_results, results = fresh(4), fresh(frames)
            assert call(layer_results, results, **kw) == bad, kw
            assert list(layer_results) == [77] * 5 and list(results) == [77] * (frames + 1), kw
        assert bytes(out) == bytes([GUARD]) * 256


@pytest.mark.parametrize("context", (None, 0x5A5A5A50), ids=("null_context", "fake_context"))
def test_the_textures_call_refuses_before_touching_a_device(hap, context):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    out = (C.c_ubyte * 1024)(*([GUARD] * 1024))
    tex = (C.c_ubyte * 1024)()
    context = C.c_void_p(context) if context else None
    layers = 2

    def call(last=WHOLE, size=(32, 32), canvas=(4, 4), formats=(L.FMT_DXT1,), layer_count=layers, textures=True, outputs=True,
             widths=True):
        ptrs = (C.c_void_p * layer_count)(*([C.addressof(tex)] * layer_count))
        lens = (C.c_ulong * layer_count)(*([1024] * layer_count))
        fmts = (C.c_uint * layer_count)(*([L.FMT_DXT5] * layer_count))
        lws = (C.c_uint * layer_count)(*([size[0]] * layer_count))
        lhs = (C.c_uint * layer_count)(*([size[1]] * layer_count))
        places = placement_array(hap, [WHOLE] * (layer_count - 1) + [last])
        count = len(formats)
        outs = (C.c_void_p * max(1, count))(*([C.addressof(out)] * count))
        caps = (C.c_ulong * max(1, count))(*([1024] * count))
        taken = (C.c_ulong * max(1, count))(*([77] * max(1, count)))
        r = lib.HapGpuCompositeTexturesEncoded(context, layer_count, ptrs if textures else None, lens, fmts, None, None,
                                               lws if widths else None, lhs, places, None, None, canvas[0], canvas[1], count,
                                               (C.c_uint * max(1, count))(*formats), outs if outputs else None, caps, taken)
        assert list(taken) == [77] * max(1, count)
        return r

    for _name, kw in OFF_GRID:
        assert call(**kw) == bad, kw
    for kw in (dict(formats=[L.FMT_YCOCG, L.FMT_RGTC1, L.FMT_DXT1]), dict(formats=[]), dict(formats=[L.FMT_YCOCG, L.FMT_DXT5]),
               dict(formats=[L.FMT_BC7]), dict(formats=[L.FMT_RGTC1]), dict(size=(30, 32)), dict(canvas=(6, 4)),
               dict(canvas=(4, 65536 * 4)), dict(layer_count=17), dict(textures=False), dict(outputs=False), dict(widths=False)):
        assert call(**kw) == bad, kw
    if context is None:
        assert call() == bad and call(formats=[L.FMT_YCOCG, L.FMT_RGTC1]) == bad
    assert bytes(out) == bytes([GUARD]) * 1024 and bytes(tex) == bytes(1024)


def test_the_python_methods_exist(hap):
    want = {"composite_textures_encoded": ["layers", "layer_sizes", "width", "height", "output_formats", "placements", "opacities",
                                           "background", "outputs"],
            "composite_frames_encoded": ["frames", "frame_bytes", "texture_counts", "layer_sizes", "width", "height", "formats",
                                         "compressors", "chunk_counts", "outputs", "placements", "opacities", "background",
                                         "decode_flags", "encode_flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["placements"].default is None, name
    with pytest.raises(ValueError, match="one output per output frame"):
        hap.Context.composite_frames_encoded(None, [[bytes(16)]], None, None, [(4, 4)], 4, 4, [L.FMT_DXT1], [1], [1], [])
    with pytest.raises(ValueError, match="one size per layer"):
        hap.Context.composite_frames_encoded(None, [[bytes(16)]], None, None, [(4, 4), (4, 4)], 4, 4, [L.FMT_DXT1], [1], [1], [None])
    with pytest.raises(ValueError, match="one placement per output frame and layer"):
        hap.Context.composite_frames_encoded(None, [[bytes(16)]], None, None, [(4, 4)], 4, 4, [L.FMT_DXT1], [1], [1], [None],
                                             placements=[[WHOLE, WHOLE]])
    with pytest.raises(ValueError, match="six numbers"):
        hap.Context.composite_textures_encoded(None, [(bytes(16), L.FMT_DXT5, None)], [(4, 4)], 4, 4, [L.FMT_DXT1],
                                               placements=[(0, 0, 4, 4)])

"""The planar float encoders without a GPU: HapGpuCompressPlanes, HapGpuEncodeFramesPlanes and HapGpuEncodeFramesPlanesBegin
are declared in the header, let out by the export map, exported by the built library, bound by hap_amd._lib with the
header's argument counts, and refuse every whole-call mistake without a context, a device or a write outside results[];
the Python methods exist and refuse tensors they cannot take before they need a context."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L

NAMES = {"HapGpuCompressPlanes": 14, "HapGpuEncodeFramesPlanes": 20, "HapGpuEncodeFramesPlanesBegin": 20}


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_the_three_functions_are_declared_listed_exported_and_bound(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned int %s\(([^;]*)\);" % name, text)
        assert declared, name
        assert len(declared.group(1).split(",")) == count, name
        for word in ("channels", "element", "planeBytes", "rowBytes", "scale", "bias", "width", "height"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    # the frame calls are HapGpuEncodeFramesRGBA's with the tensors' description in place of rowBytes
    rgba = re.search(r"unsigned int HapGpuEncodeFramesRGBA\(([^;]*)\);", text).group(1).split(",")
    assert NAMES["HapGpuEncodeFramesPlanes"] == len(rgba) + 5
    assert hap._lib.lib.HapGpuEncodeFramesPlanes.argtypes == hap._lib.lib.HapGpuEncodeFramesPlanesBegin.argtypes


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    for name in ("HapGpuCompressPlanes", "HapGpuEncodeFramesPlanes"):
        comment = text[: text.index("unsigned int %s(" % name)]
        comment = re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])       # (one line: words wrap anywhere)
        assert "Bad_Arguments" in comment, name
        # two roundings: a multiply, then an add, and not a fused one
        assert "multiply" in comment and "add" in comment and "not fused" in comment, name
        # the tie rule and what a NaN becomes
        assert "halves to even" in comment and "0.5 -> 0" in comment and "1.5 -> 2" in comment, name
        assert "NaN -> 0" in comment, name
        for word in ("BC7", "BC6H", "one-plane tensor", "ost tensors", "caled or rectangular"):
            assert word in comment, (name, word)
    frames = text[: text.index("unsigned int HapGpuEncodeFramesPlanes(")]
    frames = re.sub(r"\s*\n \*\s*", " ", frames[frames.rindex("/*"):])
    for word in ("OnDevices", "Sequence", "fused compress kernel", "HAPGPU_ENCODE_BPTC_BLOCKS is ignored", "copied by the call"):
        assert word in frames, word
    single = text[: text.index("unsigned int HapGpuCompressPlanes(")]
    single = single[single.rindex("/*"):]
    assert "4 * e" in single and "subnormal" in single and "254.5 -> 254" in single
    # the decode comments point at the way back
    for name, target in (("HapGpuDecompressPlanes", "HapGpuCompressPlanes"), ("HapGpuDecodeFramesPlanes", "HapGpuEncodeFramesPlanes")):
        comment = text[: text.index("unsigned int %s(" % name)]
        assert target in comment[comment.rindex("/*"):], name


GUARD = 0x5A


class Call:
    """The arguments of one HapGpuEncodeFramesPlanes call of two frames, all in order, with guards behind every array"""

    def __init__(self):
        self.tensor = (C.c_ubyte * 4096)(*([GUARD] * 4096))
        self.out = (C.c_ubyte * 256)(*([GUARD] * 256))
        self.frames = (C.c_void_p * 3)(C.addressof(self.tensor), C.addressof(self.tensor), 0x5A5A)
        self.outs = (C.c_void_p * 3)(C.addressof(self.out), C.addressof(self.out) + 128, 0x5A5A)
        self.caps = (C.c_ulong * 3)(128, 128, 0x5A5A)
        self.used = (C.c_ulong * 3)(71, 72, 73)
        self.res = (C.c_uint * 3)(77, 78, 79)
        self.scale = (C.c_float * 8)(*([0.5] * 8))
        self.bias = (C.c_float * 8)(*([0.25] * 8))
        self.formats = (C.c_uint * 3)(L.FMT_YCOCG, L.FMT_RGTC1, 0x5A5A)
        self.compressors = (C.c_uint * 3)(1, 1, 0x5A5A)
        self.chunks = (C.c_uint * 3)(1, 1, 0x5A5A)
        # 8 x 8 half elements, four planes: rowBytes 16, planeBytes 128
        self.a = dict(frameCount=2, planeFrames=self.frames, channels=4, element=0, planeBytes=128, rowBytes=16,
                      scale=self.scale, bias=self.bias, width=8, height=8, count=1, textureFormats=self.formats,
                      compressors=self.compressors, chunkCounts=self.chunks, outputBuffers=self.outs,
                      outputBuffersBytes=self.caps, outputBuffersBytesUsed=self.used, results=self.res, flags=0)

    ORDER = ["frameCount", "planeFrames", "channels", "element", "planeBytes", "rowBytes", "scale", "bias", "width",
             "height", "count", "textureFormats", "compressors", "chunkCounts", "outputBuffers", "outputBuffersBytes",
             "outputBuffersBytesUsed", "results", "flags"]

    def args(self, **change):
        a = dict(self.a, **change)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        assert bytes(self.out) == bytes([GUARD]) * 256 and bytes(self.tensor) == bytes([GUARD]) * 4096
        assert list(self.used) == [71, 72, 73] and list(self.caps) == [128, 128, 0x5A5A]
        assert list(self.outs) == [C.addressof(self.out), C.addressof(self.out) + 128, 0x5A5A]
        assert list(self.scale) == [0.5] * 8 and list(self.bias) == [0.25] * 8
        assert list(self.formats)[2] == 0x5A5A and list(self.compressors) == [1, 1, 0x5A5A]
        # results[f] of the call's frames may have been set (to Bad_Arguments); the entry behind them never
        assert self.res[2] == 79


# every whole-call mistake the header names: what to change in a call that is otherwise in order
WHOLE_CALL = {
    "planeFrames NULL": dict(planeFrames=None), "scale NULL": dict(scale=None), "bias NULL": dict(bias=None),
    "textureFormats NULL": dict(textureFormats=None), "compressors NULL": dict(compressors=None),
    "chunkCounts NULL": dict(chunkCounts=None), "outputBuffers NULL": dict(outputBuffers=None),
    "outputBuffersBytes NULL": dict(outputBuffersBytes=None), "outputBuffersBytesUsed NULL": dict(outputBuffersBytesUsed=None),
    "width 6": dict(width=6), "height 6": dict(height=6), "width 0": dict(width=0), "height 0": dict(height=0),
    "channels 2": dict(channels=2), "channels 5": dict(channels=5), "channels 1": dict(channels=1),
    "element 3": dict(element=3),
    "rowBytes short": dict(rowBytes=8), "rowBytes no multiple of 4 e": dict(rowBytes=20),
    "rowBytes of floats no multiple of 16": dict(element=2, rowBytes=40, planeBytes=320),
    "planeBytes short": dict(planeBytes=120), "planeBytes no multiple of 4 e": dict(planeBytes=132),
    "planeBytes short for long rows": dict(rowBytes=32, planeBytes=232),
    "more than 65535 block rows": dict(height=4 * 65536, planeBytes=16 * 4 * 65536),
    "BC7": dict(textureFormats=(C.c_uint * 1)(L.FMT_BC7), flags=0x10), "BC6H": dict(textureFormats=(C.c_uint * 1)(0x8E8F)),
    "count 0": dict(count=0), "count 3": dict(count=3),
    "pair in the wrong order": dict(count=2, textureFormats=(C.c_uint * 2)(L.FMT_RGTC1, L.FMT_YCOCG)),
    "pair of DXT5 and RGTC1": dict(count=2, textureFormats=(C.c_uint * 2)(L.FMT_DXT5, L.FMT_RGTC1)),
}


@pytest.mark.parametrize("case", list(WHOLE_CALL))
@pytest.mark.parametrize("begin", [False, True], ids=["call", "begin"])
def test_whole_call_mistakes_are_refused_without_a_context(hap, case, begin):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    fn = lib.HapGpuEncodeFramesPlanesBegin if begin else lib.HapGpuEncodeFramesPlanes
    c = Call()
    assert fn(None, *c.args(**WHOLE_CALL[case])) == bad, case
    c.untouched()
    assert list(c.res) == [bad, bad, 79], case                      # every results[f] set, the guard behind them not
    # ... and without results to set
    c = Call()
    assert fn(None, *c.args(**dict(WHOLE_CALL[case], results=None))) == bad, case
    c.untouched()
    assert list(c.res) == [77, 78, 79]


def test_a_call_in_order_still_needs_a_context(hap):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    for fn in (lib.HapGpuEncodeFramesPlanes, lib.HapGpuEncodeFramesPlanesBegin):
        c = Call()
        assert fn(None, *c.args()) == bad
        c.untouched()
        assert list(c.res) == [77, 78, 79]
        # the pair, and the long-row slice that the "short" case above falls one short of, are in order too
        assert fn(None, *c.args(count=2)) == bad and fn(None, *c.args(rowBytes=32, planeBytes=240)) == bad
        assert list(c.res) == [77, 78, 79]
    assert lib.HapGpuEncodeFramesFinish(None) == bad


TEXTURE_MISTAKES = {
    "planes NULL": dict(planes=None), "output NULL": dict(output=None), "scale NULL": dict(scale=None),
    "bias NULL": dict(bias=None), "width 6": dict(width=6), "height 6": dict(height=6), "channels 2": dict(channels=2),
    "channels 5": dict(channels=5), "element 3": dict(element=3), "rowBytes short": dict(rowBytes=8),
    "rowBytes no multiple of 4 e": dict(rowBytes=20), "planeBytes short": dict(planeBytes=120),
    "planeBytes no multiple of 4 e": dict(planeBytes=132),
    "more than 65535 block rows": dict(height=4 * 65536, planeBytes=16 * 4 * 65536),
    "BC7": dict(textureFormat=L.FMT_BC7), "BC6H": dict(textureFormat=0x8E8E), "in order": dict(),
}


@pytest.mark.parametrize("case", list(TEXTURE_MISTAKES))
def test_compress_planes_refuses_without_a_context(hap, case):
    lib = hap._lib.lib
    c = Call()
    used = (C.c_ulong * 2)(71, 72)
    a = dict(planes=c.tensor, planeBytes=128, rowBytes=16, channels=4, element=0, scale=c.scale, bias=c.bias, width=8,
             height=8, textureFormat=L.FMT_YCOCG, output=c.out, outputBytes=256, outputBytesUsed=used)
    a.update(TEXTURE_MISTAKES[case])
    order = ["planes", "planeBytes", "rowBytes", "channels", "element", "scale", "bias", "width", "height", "textureFormat",
             "output", "outputBytes", "outputBytesUsed"]
    assert lib.HapGpuCompressPlanes(None, *[a[k] for k in order]) == hap.HapResult.Bad_Arguments, case
    c.untouched()
    assert list(used) == [71, 72] and list(c.res) == [77, 78, 79]


def test_the_python_methods_exist(hap):
    want = {"compress_planes": ["planes", "width", "height", "texture_format", "scale", "bias", "output"],
            "encode_frames_planes": ["planes", "width", "height", "formats", "compressors", "chunk_counts", "outputs",
                                     "scale", "bias", "flags"],
            "encode_frames_planes_begin": ["planes", "width", "height", "formats", "compressors", "chunk_counts", "outputs",
                                           "scale", "bias", "flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["scale"].default is None and sig.parameters["bias"].default is None, name
    # scale=None means 255, bias=None means 0
    sc, bi = hap.api._plane_constants(None, None, 3, 255.0)
    assert list(sc) == [255.0] * 3 and list(bi) == [0.0] * 3
    sc, _bi = hap.api._plane_constants(None, None, 4)                       # (the decode side's default stays)
    assert [float(v) for v in sc] == [C.c_float(1.0 / 255.0).value] * 4


def test_the_python_methods_refuse_tensors_they_cannot_take(hap):
    torch = pytest.importorskip("torch")
    out = bytearray(64)
    # (no context is needed: the tensors are looked at before anything else; unbound: self is never looked at)
    for method, tail in ((hap.Context.encode_frames_planes, ([L.FMT_DXT5], [1], [1], [out])),
                         (hap.Context.encode_frames_planes_begin, ([L.FMT_DXT5], [1], [1], [out]))):
        with pytest.raises(ValueError, match="dtype"):
            method(None, torch.zeros((1, 3, 4, 4), dtype=torch.uint8), 4, 4, *tail)
        with pytest.raises(ValueError, match="dtype"):
            method(None, [torch.zeros((3, 4, 4), dtype=torch.float64)], 4, 4, *tail)
        wide = torch.zeros((1, 3, 4, 8), dtype=torch.float16)[..., ::2]
        assert wide.shape == (1, 3, 4, 4) and wide.stride(-1) == 2
        with pytest.raises(ValueError, match="stride"):
            method(None, wide, 4, 4, *tail)
        with pytest.raises(ValueError, match="per frame"):
            method(None, torch.zeros((1, 3, 4, 8), dtype=torch.float16), 4, 4, *tail)
        with pytest.raises(ValueError, match="device memory"):
            method(None, torch.zeros((1, 3, 4, 4), dtype=torch.float16), 4, 4, *tail)
    for bad in (torch.zeros((3, 4, 4), dtype=torch.uint8), torch.zeros((3, 4, 4), dtype=torch.float32),
                torch.zeros((3, 4, 8), dtype=torch.bfloat16)[..., ::2], torch.zeros((2, 4, 4), dtype=torch.float16)):
        with pytest.raises(ValueError):
            hap.Context.compress_planes(None, bad, 4, 4, L.FMT_DXT5)

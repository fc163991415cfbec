"""The video encoders without a GPU: HapGpuCompressNV12, HapGpuEncodeFramesNV12 and HapGpuEncodeFramesNV12Begin are
declared in the header, let out by the export map, exported by the built library, bound by hap_amd._lib with the header's
argument counts, and refuse every whole-call mistake without a context, a device or a write outside results[]; the
header states the definition and what is out of scope; the Python methods exist and refuse planes they cannot take before
they need a context."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L
import _video_pictures as V

NAMES = {"HapGpuCompressNV12": 13, "HapGpuEncodeFramesNV12": 19, "HapGpuEncodeFramesNV12Begin": 19}


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
        for word in ("uma", "lumaRowBytes", "hroma", "chromaRowBytes", "matrix", "range", "width", "height"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    # the frame calls are HapGpuEncodeFramesRGBA's with the planes' description in place of the pictures and rowBytes
    rgba = re.search(r"unsigned int HapGpuEncodeFramesRGBA\(([^;]*)\);", text).group(1).split(",")
    assert NAMES["HapGpuEncodeFramesNV12"] == len(rgba) + 4
    assert hap._lib.lib.HapGpuEncodeFramesNV12.argtypes == hap._lib.lib.HapGpuEncodeFramesNV12Begin.argtypes
    for name, value in (("YCBCR_BT601", 0), ("YCBCR_BT709", 1), ("YCBCR_LIMITED", 0), ("YCBCR_FULL", 1)):
        assert name in hap._API_NAMES and getattr(hap, name) == value, name
    assert (hap.YCBCR_BT601, hap.YCBCR_BT709, hap.YCBCR_LIMITED, hap.YCBCR_FULL) == (V.BT601, V.BT709, V.LIMITED, V.FULL)
    assert "enum HapGpuYCbCrMatrix { HapGpuYCbCrMatrix_BT601 = 0, HapGpuYCbCrMatrix_BT709 = 1 }" in text
    assert "enum HapGpuYCbCrRange { HapGpuYCbCrRange_Limited = 0, HapGpuYCbCrRange_Full = 1 }" in text


def comment_before(text, name):
    comment = text[: text.index("unsigned int %s(" % name)]
    return re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])          # (one line: words wrap anywhere)


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    single, frames = comment_before(text, "HapGpuCompressNV12"), comment_before(text, "HapGpuEncodeFramesNV12")
    for name, comment in (("HapGpuCompressNV12", single), ("HapGpuEncodeFramesNV12", frames)):
        assert "Bad_Arguments" in comment, name
        # which samples a texel takes, and that nothing is filtered
        assert "UV[y >> 1][2 * (x >> 1)]" in comment and "UV[y >> 1][2 * (x >> 1) + 1]" in comment, name
        assert "replicated" in comment and "no filtering" in comment, name
        # the arithmetic
        for word in ("y' = Y - 16", "u = Cb - 128", "v = Cr - 128", "clamp255((cy * y' + crv * v", "- cgu * u - cgv * v",
                     "cbu * u", "+ 32768) >> 16", "A = 255", "32-bit"):
            assert word in comment, (name, word)
        # what is out of scope
        for word in ("way back", "P010", "I420", "4:2:2", "4:4:4", "iltered or sited chroma", "A8 plane", "Hap Alpha",
                     "Hap Q Alpha", "Alpha-Only", "BC7", "BC6H", "ost pictures"):
            assert word in comment, (name, word)
        # the rules
        for word in ("DEVICE", "multiples of 4", "65535 block rows", "RGB_DXT1", "YCoCg_DXT5", "byte for byte"):
            assert word in comment, (name, word)
    # the table, every row derived in tests/_video_pictures.py
    for row in V.ROWS:
        k, _offset = V.coefficients(*row)
        assert re.search(r"\s+".join(str(v) for v in k), single), row
    for word in ("0.299", "0.114", "0.2126", "0.0722", "255/219", "255/224", "times 65536", "3.6e7", "0.5016", "clamped",
                 "no direct YCbCr -> YCoCg", "lumaRowBytes >= width", "chromaRowBytes >= width"):
        assert word in single, word
    for word in ("OnDevices", "Sequence", "fused compress kernel", "HAPGPU_ENCODE_BPTC_BLOCKS is ignored",
                 "HAPGPU_ENCODE_REFINE_ENDPOINTS is honoured", "copied by the call", "count == 1", "count == 2",
                 "HapGpuEncodeFramesPlanes'", "Bad_Arguments alone", "32768 frames", "HapGpuEncodeFramesFinish"):
        assert word in frames, word


GUARD = 0x5A


class Call:
    """The arguments of one HapGpuEncodeFramesNV12 call of two 8 x 8 frames, all in order, with guards behind every array"""

    def __init__(self):
        self.planes = (C.c_ubyte * 4096)(*([GUARD] * 4096))
        self.out = (C.c_ubyte * 256)(*([GUARD] * 256))
        base = C.addressof(self.planes)
        self.luma = (C.c_void_p * 3)(base, base + 1024, 0x5A5A)
        self.chroma = (C.c_void_p * 3)(base + 2048, base + 3072, 0x5A5A)
        self.outs = (C.c_void_p * 3)(C.addressof(self.out), C.addressof(self.out) + 128, 0x5A5A)
        self.caps = (C.c_ulong * 3)(128, 128, 0x5A5A)
        self.used = (C.c_ulong * 3)(71, 72, 73)
        self.res = (C.c_uint * 3)(77, 78, 79)
        self.formats = (C.c_uint * 3)(L.FMT_YCOCG, L.FMT_RGTC1, 0x5A5A)
        self.compressors = (C.c_uint * 3)(1, 1, 0x5A5A)
        self.chunks = (C.c_uint * 3)(1, 1, 0x5A5A)
        self.a = dict(frameCount=2, lumaPlanes=self.luma, lumaRowBytes=16, chromaPlanes=self.chroma, chromaRowBytes=12,
                      matrix=V.BT709, range=V.LIMITED, width=8, height=8, count=1, textureFormats=self.formats,
                      compressors=self.compressors, chunkCounts=self.chunks, outputBuffers=self.outs,
                      outputBuffersBytes=self.caps, outputBuffersBytesUsed=self.used, results=self.res, flags=0)

    ORDER = ["frameCount", "lumaPlanes", "lumaRowBytes", "chromaPlanes", "chromaRowBytes", "matrix", "range", "width",
             "height", "count", "textureFormats", "compressors", "chunkCounts", "outputBuffers", "outputBuffersBytes",
             "outputBuffersBytesUsed", "results", "flags"]

    def args(self, **change):
        a = dict(self.a, **change)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        base = C.addressof(self.planes)
        assert bytes(self.out) == bytes([GUARD]) * 256 and bytes(self.planes) == bytes([GUARD]) * 4096
        assert list(self.used) == [71, 72, 73] and list(self.caps) == [128, 128, 0x5A5A]
        assert list(self.outs) == [C.addressof(self.out), C.addressof(self.out) + 128, 0x5A5A]
        assert list(self.luma) == [base, base + 1024, 0x5A5A] and list(self.chroma) == [base + 2048, base + 3072, 0x5A5A]
        assert list(self.formats) == [L.FMT_YCOCG, L.FMT_RGTC1, 0x5A5A] and list(self.compressors) == [1, 1, 0x5A5A]
        # results[f] of the call's frames may have been set (to Bad_Arguments); the entry behind them never
        assert self.res[2] == 79


# every whole-call mistake the header names: what to change in a call that is otherwise in order
WHOLE_CALL = {
    "lumaPlanes NULL": dict(lumaPlanes=None), "chromaPlanes NULL": dict(chromaPlanes=None),
    "textureFormats NULL": dict(textureFormats=None), "compressors NULL": dict(compressors=None),
    "chunkCounts NULL": dict(chunkCounts=None), "outputBuffers NULL": dict(outputBuffers=None),
    "outputBuffersBytes NULL": dict(outputBuffersBytes=None), "outputBuffersBytesUsed NULL": dict(outputBuffersBytesUsed=None),
    "width 6": dict(width=6), "height 6": dict(height=6), "width 2": dict(width=2), "width 0": dict(width=0),
    "height 0": dict(height=0),
    "matrix 2": dict(matrix=2), "matrix -1": dict(matrix=0xFFFFFFFF), "range 2": dict(range=2), "range -1": dict(range=0xFFFFFFFF),
    "lumaRowBytes short": dict(lumaRowBytes=4), "lumaRowBytes no multiple of 4": dict(lumaRowBytes=18),
    "lumaRowBytes 0": dict(lumaRowBytes=0),
    "chromaRowBytes short": dict(chromaRowBytes=4), "chromaRowBytes no multiple of 4": dict(chromaRowBytes=10),
    "chromaRowBytes of width / 2": dict(width=16, lumaRowBytes=16, chromaRowBytes=8),
    "more than 65535 block rows": dict(height=4 * 65536),
    "DXT5": dict(textureFormats=(C.c_uint * 1)(L.FMT_DXT5)), "RGTC1": dict(textureFormats=(C.c_uint * 1)(L.FMT_RGTC1)),
    "BC7": dict(textureFormats=(C.c_uint * 1)(L.FMT_BC7), flags=0x10), "BC6H": dict(textureFormats=(C.c_uint * 1)(L.FMT_BC6U)),
    "count 0": dict(count=0), "count 2": dict(count=2), "count 3": dict(count=3),
    "count 2, DXT1 first": dict(count=2, textureFormats=(C.c_uint * 2)(L.FMT_DXT1, L.FMT_RGTC1)),
}


@pytest.mark.parametrize("case", list(WHOLE_CALL))
@pytest.mark.parametrize("begin", [False, True], ids=["call", "begin"])
def test_whole_call_mistakes_are_refused_without_a_context(hap, case, begin):
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    fn = lib.HapGpuEncodeFramesNV12Begin if begin else lib.HapGpuEncodeFramesNV12
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
    for fn in (lib.HapGpuEncodeFramesNV12, lib.HapGpuEncodeFramesNV12Begin):
        c = Call()
        assert fn(None, *c.args()) == bad
        c.untouched()
        assert list(c.res) == [77, 78, 79]
        # every row of the table, both formats, and pitches of exactly the width are in order too
        for matrix, range_ in V.ROWS:
            assert fn(None, *c.args(matrix=matrix, range=range_, textureFormats=(C.c_uint * 1)(L.FMT_DXT1))) == bad
        assert fn(None, *c.args(lumaRowBytes=8, chromaRowBytes=8)) == bad
        assert list(c.res) == [77, 78, 79]
    # a ...Begin of more frames than a slice holds is refused before anything is looked at or set
    c = Call()
    assert lib.HapGpuEncodeFramesNV12Begin(None, *c.args(frameCount=32769)) == bad
    assert list(c.res) == [77, 78, 79]
    assert lib.HapGpuEncodeFramesFinish(None) == bad


TEXTURE_MISTAKES = {
    "luma NULL": dict(luma=None), "chroma NULL": dict(chroma=None), "output NULL": dict(output=None),
    "width 6": dict(width=6), "height 6": dict(height=6), "width 0": dict(width=0), "height 0": dict(height=0),
    "matrix 2": dict(matrix=2), "range 2": dict(range=2),
    "lumaRowBytes short": dict(lumaRowBytes=4), "lumaRowBytes no multiple of 4": dict(lumaRowBytes=18),
    "chromaRowBytes short": dict(chromaRowBytes=4), "chromaRowBytes no multiple of 4": dict(chromaRowBytes=10),
    "more than 65535 block rows": dict(height=4 * 65536),
    "DXT5": dict(textureFormat=L.FMT_DXT5), "RGTC1": dict(textureFormat=L.FMT_RGTC1), "BC7": dict(textureFormat=L.FMT_BC7),
    "BC6H": dict(textureFormat=L.FMT_BC6S), "in order": dict(),
}


@pytest.mark.parametrize("case", list(TEXTURE_MISTAKES))
def test_compress_nv12_refuses_without_a_context(hap, case):
    lib = hap._lib.lib
    c = Call()
    used = (C.c_ulong * 2)(71, 72)
    base = C.addressof(c.planes)
    a = dict(luma=base, lumaRowBytes=16, chroma=base + 2048, chromaRowBytes=12, matrix=V.BT601, range=V.FULL, width=8,
             height=8, textureFormat=L.FMT_YCOCG, output=c.out, outputBytes=256, outputBytesUsed=used)
    a.update(TEXTURE_MISTAKES[case])
    order = ["luma", "lumaRowBytes", "chroma", "chromaRowBytes", "matrix", "range", "width", "height", "textureFormat",
             "output", "outputBytes", "outputBytesUsed"]
    assert lib.HapGpuCompressNV12(None, *[a[k] for k in order]) == hap.HapResult.Bad_Arguments, case
    c.untouched()
    assert list(used) == [71, 72] and list(c.res) == [77, 78, 79]


def test_the_python_methods_exist(hap):
    tail = ["matrix", "range", "luma_row_bytes", "chroma_row_bytes"]
    frames = ["luma_planes", "chroma_planes", "width", "height", "formats", "compressors", "chunk_counts", "outputs"]
    want = {"compress_nv12": ["luma", "chroma", "width", "height", "texture_format"] + tail + ["output"],
            "encode_frames_nv12": frames + tail + ["flags"], "encode_frames_nv12_begin": frames + tail + ["flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["matrix"].default == hap.YCBCR_BT709 and sig.parameters["range"].default == hap.YCBCR_LIMITED


def test_the_python_methods_refuse_planes_they_cannot_take(hap):
    torch = pytest.importorskip("torch")
    out = bytearray(64)
    y, uv = torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 2, 4), dtype=torch.uint8)
    tail = ([L.FMT_DXT1], [1], [1], [out])
    # (no context is needed: the planes are looked at before anything else; unbound: self is never looked at)
    for method in (hap.Context.encode_frames_nv12, hap.Context.encode_frames_nv12_begin):
        with pytest.raises(ValueError, match="dtype"):
            method(None, y.to(torch.float16), uv, 4, 4, *tail)
        with pytest.raises(ValueError, match="dtype"):
            method(None, [0x1000], [uv[0].to(torch.int8)], 4, 4, *tail, luma_row_bytes=4)
        with pytest.raises(ValueError, match="per frame"):
            method(None, torch.zeros((1, 4, 8), dtype=torch.uint8), uv, 4, 4, *tail)
        with pytest.raises(ValueError, match="per frame"):
            method(None, [0x1000], torch.zeros((1, 4, 4), dtype=torch.uint8), 4, 4, *tail, luma_row_bytes=4)
        with pytest.raises(ValueError, match="one chroma plane"):
            method(None, [0x1000], [0x2000, 0x3000], 4, 4, *tail, luma_row_bytes=4, chroma_row_bytes=4)
        with pytest.raises(ValueError, match="stride"):
            method(None, torch.zeros((1, 4, 8), dtype=torch.uint8)[..., ::2], uv, 4, 4, *tail)
        with pytest.raises(ValueError, match="device memory"):
            method(None, y, uv, 4, 4, *tail)
        with pytest.raises(ValueError, match="row_bytes"):
            method(None, [0x1000], [0x2000], 4, 4, *tail)
    for bad in (torch.zeros((4, 4), dtype=torch.float32), torch.zeros((4, 8), dtype=torch.uint8)[:, ::2],
                torch.zeros((8, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            hap.Context.compress_nv12(None, bad, uv[0], 4, 4, L.FMT_DXT1)
    # pairs as a last dimension of two are the same plane
    planes, pitch, _keep = hap.api._video_planes([0x1000, None], False, 2, 4, 8, "chroma")
    assert planes == [0x1000, None] and pitch == 8

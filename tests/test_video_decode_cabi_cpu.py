"""The video decoders without a GPU: HapGpuDecompressNV12 and HapGpuDecodeFramesNV12 are declared in the header, let out
by the export map, exported by the built library, bound by hap_amd._lib with the header's argument counts, and refuse
every whole-call mistake without a context, a device or a write outside results[]; the header states the definition, its
table and what is out of scope; the Python methods exist and refuse planes they cannot take before they need a context."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

import _libs as L
import _video_planes as P

NAMES = {"HapGpuDecompressNV12": 13, "HapGpuDecodeFramesNV12": 16}


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
        for word in ("uma", "lumaRowBytes", "hroma", "chromaRowBytes", "matrix", "range", "width", "height", "scaleLog2"):
            assert word in declared.group(1), (name, word)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert bound.restype is C.c_uint and bound.argtypes[0] is C.c_void_p, name
        assert len(bound.argtypes) == count, name
    # the frame call is HapGpuDecodeFramesRGBAScaled's with the planes' description in place of the pictures and rowBytes
    scaled = re.search(r"unsigned int HapGpuDecodeFramesRGBAScaled\(([^;]*)\);", text).group(1).split(",")
    assert NAMES["HapGpuDecodeFramesNV12"] == len(scaled) + 4
    # the launcher is declared where the host side finds it
    abi = open(os.path.join(L.ROOT, "hap_amd", "csrc", "hapgpu_abi.h")).read()
    assert re.search(r"int hapgpu_k_block_decode_video\(hapgpu_rt \*rt, const HapGpuPictureTable \*table,", abi)
    assert (hap.YCBCR_BT601, hap.YCBCR_BT709, hap.YCBCR_LIMITED, hap.YCBCR_FULL) == (P.BT601, P.BT709, P.LIMITED, P.FULL)


def comment_before(text, name):
    comment = text[: text.index("unsigned int %s(" % name)]
    return re.sub(r"\s*\n \*\s*", " ", comment[comment.rindex("/*"):])          # (one line: words wrap anywhere)


def test_the_header_states_the_definition_and_what_is_out_of_scope():
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    single, frames = comment_before(text, "HapGpuDecompressNV12"), comment_before(text, "HapGpuDecodeFramesNV12")
    for name, comment in (("HapGpuDecompressNV12", single), ("HapGpuDecodeFramesNV12", frames)):
        assert "Bad_Arguments" in comment, name
        # the arithmetic
        for word in ("lo + ((yr * R + yg * G + yb * B + 32768) >> 16)", "d(2i..2i+1, 2j..2j+1)",
                     "clamp255((-cbr * Rs - cbg * Gs + ch * Bs + (128 << 18) + (1 << 17)) >> 18)",
                     "clamp255(( ch * Rs - crg * Gs - crb * Bs + (128 << 18) + (1 << 17)) >> 18)", "32-bit", "lpha i"):
            assert word in comment, (name, word)
        # what is out of scope
        for word in ("Hap R", "Hap HDR", "Alpha-Only", "A8 plane beside the NV12", "P010", "I420", "4:2:2", "4:4:4",
                     "sited or filtered chroma", "rectangles", "host planes"):
            assert word in comment, (name, word)
        # the rules
        for word in ("DEVICE", "multiples of 4", "4 << scaleLog2", "65535 output block rows", "scaleLog2 0 to 2",
                     "lumaRowBytes >= W", "chromaRowBytes >= W", "Only the samples are written", "way back"):
            assert word in comment, (name, word)
    # the table, every row derived in tests/_video_planes.py
    for row in P.ROWS:
        k, lo = P.coefficients(*row)
        assert re.search(r"\s+".join(str(v) for v in k + (lo,)), single), row
    for word in ("0.299", "0.114", "0.2126", "0.0722", "219/255", "224/255", "times 65536", "yg = round(65536 * sy) - yr - yb",
                 "cbg = ch - cbr", "crg = ch - crb", "Cb = Cr = 128 exactly", "235 / 16", "255 / 0", "0 .. 2^26",
                 "reaches 256 before the clamp", "0.5021", "four different texels", "0.5024", "1, 1, 2", "1, 1, 1",
                 "HapGpuDecompressRGBAScaled", "RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5", "one rounding", "no filtering"):
        assert word in single, word
    for word in ("OnDevices", "Sequence", "HAPGPU_DECODE_BPTC_PICTURES is ignored", "never block-decoded",
                 "Hap, Hap Alpha, Hap Q, and Hap Q Alpha with textureCount 2", "HapGpuDecodeFramesRGBA's", "fails alone",
                 "left untouched", "first failure", "every results[f] set", "HapGpuEncodeFramesFinish", "Internal_Error",
                 "16 + 64 + 64 + 24"):
        assert word in frames, word
    # the encode side points the way back here, and keeps its words
    for name in ("HapGpuCompressNV12", "HapGpuEncodeFramesNV12"):
        comment = comment_before(text, name)
        assert "way back" in comment and "HapGpuDecodeFramesNV12" in comment, name


GUARD = 0x5A


class Call:
    """The arguments of one HapGpuDecodeFramesNV12 call of two 16 x 16 frames at half size, all in order, with guards
    behind every array"""

    def __init__(self):
        self.planes = (C.c_ubyte * 4096)(*([GUARD] * 4096))
        self.frames = (C.c_ubyte * 256)(*([GUARD] * 256))
        base = C.addressof(self.planes)
        self.inputs = (C.c_void_p * 3)(C.addressof(self.frames), C.addressof(self.frames) + 128, 0x5A5A)
        self.lens = (C.c_ulong * 3)(128, 128, 0x5A5A)
        self.luma = (C.c_void_p * 3)(base, base + 1024, 0x5A5A)
        self.chroma = (C.c_void_p * 3)(base + 2048, base + 3072, 0x5A5A)
        self.res = (C.c_uint * 3)(77, 78, 79)
        self.a = dict(frameCount=2, inputBuffers=self.inputs, inputBuffersBytes=self.lens, textureCount=1,
                      lumaPlanes=self.luma, lumaRowBytes=16, chromaPlanes=self.chroma, chromaRowBytes=12, matrix=P.BT709,
                      range=P.LIMITED, width=16, height=16, scaleLog2=1, results=self.res, flags=0)

    ORDER = ["frameCount", "inputBuffers", "inputBuffersBytes", "textureCount", "lumaPlanes", "lumaRowBytes", "chromaPlanes",
             "chromaRowBytes", "matrix", "range", "width", "height", "scaleLog2", "results", "flags"]

    def args(self, **change):
        a = dict(self.a, **change)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        base = C.addressof(self.planes)
        assert bytes(self.frames) == bytes([GUARD]) * 256 and bytes(self.planes) == bytes([GUARD]) * 4096
        assert list(self.lens) == [128, 128, 0x5A5A]
        assert list(self.inputs) == [C.addressof(self.frames), C.addressof(self.frames) + 128, 0x5A5A]
        assert list(self.luma) == [base, base + 1024, 0x5A5A] and list(self.chroma) == [base + 2048, base + 3072, 0x5A5A]
        # results[f] of the call's frames may have been set (to Bad_Arguments); the entry behind them never
        assert self.res[2] == 79


# every whole-call mistake the header names: what to change in a call that is otherwise in order
WHOLE_CALL = {
    "inputBuffers NULL": dict(inputBuffers=None), "inputBuffersBytes NULL": dict(inputBuffersBytes=None),
    "lumaPlanes NULL": dict(lumaPlanes=None), "chromaPlanes NULL": dict(chromaPlanes=None),
    "scaleLog2 3": dict(scaleLog2=3), "scaleLog2 -1": dict(scaleLog2=0xFFFFFFFF),
    "width 12 at half size": dict(width=12), "height 12 at half size": dict(height=12),
    "width 24 at quarter size": dict(width=24, scaleLog2=2), "height 8 at quarter size": dict(height=8, scaleLog2=2),
    "width 6": dict(width=6, scaleLog2=0), "width 0": dict(width=0), "height 0": dict(height=0),
    "matrix 2": dict(matrix=2), "matrix -1": dict(matrix=0xFFFFFFFF), "range 2": dict(range=2), "range -1": dict(range=0xFFFFFFFF),
    "lumaRowBytes short": dict(lumaRowBytes=4), "lumaRowBytes no multiple of 4": dict(lumaRowBytes=18),
    "lumaRowBytes 0": dict(lumaRowBytes=0), "lumaRowBytes of the output at full size": dict(scaleLog2=0, lumaRowBytes=8),
    "chromaRowBytes short": dict(chromaRowBytes=4), "chromaRowBytes no multiple of 4": dict(chromaRowBytes=10),
    "chromaRowBytes of W / 2": dict(width=32, lumaRowBytes=16, chromaRowBytes=8),
    "more than 65535 output block rows": dict(height=8 * 65536),
    "more than 65535 block rows at full size": dict(height=4 * 65536, scaleLog2=0),
    "textureCount 0": dict(textureCount=0), "textureCount 3": dict(textureCount=3),
}


@pytest.mark.parametrize("case", list(WHOLE_CALL))
def test_whole_call_mistakes_are_refused_without_a_context(hap, case):
    fn = hap._lib.lib.HapGpuDecodeFramesNV12
    bad = hap.HapResult.Bad_Arguments
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
    fn = hap._lib.lib.HapGpuDecodeFramesNV12
    bad = hap.HapResult.Bad_Arguments
    c = Call()
    assert fn(None, *c.args()) == bad
    c.untouched()
    assert list(c.res) == [77, 78, 79]
    # every row of the table, every scale, both texture counts and pitches of exactly W are in order too
    for matrix, range_ in P.ROWS:
        assert fn(None, *c.args(matrix=matrix, range=range_, textureCount=2)) == bad
    for s in (0, 1, 2):
        assert fn(None, *c.args(scaleLog2=s, lumaRowBytes=16 >> s, chromaRowBytes=16 >> s)) == bad
    assert fn(None, *c.args(height=8 * 65535, flags=0x10)) == bad
    assert list(c.res) == [77, 78, 79]


TEXTURE_MISTAKES = {
    "luma NULL": dict(luma=None), "chroma NULL": dict(chroma=None), "scaleLog2 3": dict(scaleLog2=3),
    "width 12": dict(width=12), "height 12": dict(height=12), "width 0": dict(width=0), "height 0": dict(height=0),
    "matrix 2": dict(matrix=2), "range 2": dict(range=2),
    "lumaRowBytes short": dict(lumaRowBytes=4), "lumaRowBytes no multiple of 4": dict(lumaRowBytes=18),
    "chromaRowBytes short": dict(chromaRowBytes=4), "chromaRowBytes no multiple of 4": dict(chromaRowBytes=10),
    "more than 65535 output block rows": dict(height=8 * 65536), "in order": dict(),
}


@pytest.mark.parametrize("case", list(TEXTURE_MISTAKES))
def test_decompress_nv12_refuses_without_a_context(hap, case):
    lib = hap._lib.lib
    c = Call()
    base = C.addressof(c.planes)
    a = dict(texture=c.frames, textureBytes=256, textureFormat=L.FMT_YCOCG, width=16, height=16, scaleLog2=1, matrix=P.BT601,
             range=P.FULL, luma=base, lumaRowBytes=16, chroma=base + 2048, chromaRowBytes=12)
    a.update(TEXTURE_MISTAKES[case])
    order = ["texture", "textureBytes", "textureFormat", "width", "height", "scaleLog2", "matrix", "range", "luma",
             "lumaRowBytes", "chroma", "chromaRowBytes"]
    assert lib.HapGpuDecompressNV12(None, *[a[k] for k in order]) == hap.HapResult.Bad_Arguments, case
    c.untouched()
    assert list(c.res) == [77, 78, 79]


def test_the_python_methods_exist(hap):
    tail = ["scale_log2", "matrix", "range", "luma_row_bytes", "chroma_row_bytes"]
    want = {"decompress_nv12": ["texture", "texture_format", "width", "height", "luma", "chroma"] + tail,
            "decode_frames_nv12": ["frames", "frame_bytes", "texture_count", "luma_planes", "chroma_planes", "width", "height"]
            + tail + ["flags"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["matrix"].default == hap.YCBCR_BT709 and sig.parameters["range"].default == hap.YCBCR_LIMITED
        assert sig.parameters["scale_log2"].default == 0


def test_the_python_methods_refuse_planes_they_cannot_take(hap):
    torch = pytest.importorskip("torch")
    frame = bytes(64)
    y, uv = torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 2, 4), dtype=torch.uint8)
    method = hap.Context.decode_frames_nv12
    # (no context is needed: the planes are looked at before anything else; unbound: self is never looked at)
    with pytest.raises(ValueError, match="dtype"):
        method(None, [frame], [64], 1, y.to(torch.float16), uv, 4, 4)
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, y, uv, 8, 8)                        # planes of the frames' size at full size ...
    with pytest.raises(ValueError, match="device memory"):
        method(None, [frame], [64], 1, y, uv, 8, 8, scale_log2=1)          # ... but of the output's at half size
    with pytest.raises(ValueError, match="per frame"):
        method(None, [frame], [64], 1, y, uv, 4, 4, scale_log2=1)
    with pytest.raises(ValueError, match="one chroma plane"):
        method(None, [frame], [64], 1, [0x1000], [0x2000, 0x3000], 4, 4, luma_row_bytes=4, chroma_row_bytes=4)
    with pytest.raises(ValueError, match="one chroma plane"):
        method(None, [frame, frame], [64, 64], 1, [0x1000], [0x2000], 4, 4, luma_row_bytes=4, chroma_row_bytes=4)
    with pytest.raises(ValueError, match="stride"):
        method(None, [frame], [64], 1, torch.zeros((1, 4, 8), dtype=torch.uint8)[..., ::2], uv, 4, 4)
    with pytest.raises(ValueError, match="row_bytes"):
        method(None, [frame], [64], 1, [0x1000], [0x2000], 4, 4)
    for bad in (torch.zeros((4, 4), dtype=torch.float32), torch.zeros((4, 8), dtype=torch.uint8)[:, ::2],
                torch.zeros((8, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            hap.Context.decompress_nv12(None, frame, L.FMT_DXT1, 4, 4, bad, uv[0])

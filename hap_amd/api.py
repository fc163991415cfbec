"""Python mirror of include/hap.h and include/hap_gpu.h (same names, argument
meaning and result codes as /root/reference/source/hap.h:40-152).

Buffers may be bytes / bytearray / numpy arrays (host) or objects exposing
`data_ptr()` + `numel()`/`nbytes` (torch CUDA tensors -> used in place)."""
import ctypes as C
import os

from ._lib import CALLBACK, WORK_FN, HapGpuPictureError, HapGpuPlacement, lib


class HapTextureFormat:
    RGB_DXT1 = 0x83F0
    RGBA_DXT5 = 0x83F3
    YCoCg_DXT5 = 0x01
    A_RGTC1 = 0x8DBB
    RGBA_BPTC_UNORM = 0x8E8C
    RGB_BPTC_UNSIGNED_FLOAT = 0x8E8F
    RGB_BPTC_SIGNED_FLOAT = 0x8E8E


HapCompressorNone, HapCompressorSnappy = 0, 1


class HapResult:
    No_Error, Bad_Arguments, Buffer_Too_Small, Bad_Frame, Internal_Error = range(5)


ENCODE_FRAGMENT_INDEX = 0x1
ENCODE_COARSE_MATCHES = 0x2
ENCODE_SMALLER_FILES = 0x4
ENCODE_FINE_CHUNKS = 0x8
ENCODE_BPTC_BLOCKS = 0x10
ENCODE_REFINE_ENDPOINTS = 0x20     # HAPGPU_ENCODE_REFINE_ENDPOINTS: refined end points for RGB_DXT1 / RGBA_DXT5 colour blocks
DECODE_IGNORE_FRAGMENT_INDEX = 0x1
DECODE_IGNORE_HALF_TILES = 0x2
DECODE_NO_BLOCK_SCAN = 0x4
DECODE_NO_FIELD_GUESS = 0x8
DECODE_GUESS_FIELDS = 0x10
DECODE_BPTC_PICTURES = 0x20
COMPOSITE_MAX_LAYERS = 16          # HAPGPU_COMPOSITE_MAX_LAYERS
KERNEL_CLASSES = ["block_encode", "snappy_compress", "frame_pack", "frame_gather", "decode_plan", "snappy_decode",
                  "block_decode", "block_scan", "encode_fused"]


PLANE_ELEMENTS = {"torch.float16": 0, "torch.bfloat16": 1, "torch.float32": 2}     # HapGpuPlaneElement by dtype


def _plane_tensors(out, single, width, height, scale_log2):
    """The tensors of a planar call and what they share: ([3-D tensors], channels, element, planeBytes, rowBytes).
    `out`: one (C, H >> s, W >> s) tensor (single), or one (N, C, H >> s, W >> s) tensor or a list of N 3-D ones."""
    if single:
        tensors = [out]
    elif hasattr(out, "dim"):
        if out.dim() != 4:
            raise ValueError("out: one (N, C, H >> s, W >> s) tensor or a list of (C, H >> s, W >> s) tensors")
        tensors = [out[i] for i in range(out.shape[0])]
    else:
        tensors = list(out)
    if not tensors:
        raise ValueError("out: no tensors")
    shift = scale_log2 if 0 <= scale_log2 < 3 else 0          # (a refused scale: nothing is written)
    shape = None
    for t in tensors:
        if t is None:                                          # (a frame without a tensor: Bad_Arguments for it alone)
            continue
        if not (hasattr(t, "dim") and hasattr(t, "stride") and hasattr(t, "data_ptr")):
            raise ValueError("out: torch tensors")
        if str(t.dtype) not in PLANE_ELEMENTS:
            raise ValueError("out: dtype float16, bfloat16 or float32, not %s" % t.dtype)
        if t.dim() != 3 or t.shape[0] not in (3, 4) or tuple(t.shape[1:]) != (height >> shift, width >> shift):
            raise ValueError("out: (3 or 4, %d, %d) per frame, not %s" % (height >> shift, width >> shift, tuple(t.shape)))
        if t.stride(2) != 1:
            raise ValueError("out: stride(-1) must be 1")
        if t.device.type != "cuda":
            raise ValueError("out: tensors in device memory")
        this = (t.shape[0], str(t.dtype), t.stride(0), t.stride(1))
        if shape is not None and this != shape:
            raise ValueError("out: the tensors of a call share channels, dtype and strides")
        shape = this
    if shape is None:
        raise ValueError("out: no tensors")
    e = 4 if shape[1] == "torch.float32" else 2
    return tensors, shape[0], PLANE_ELEMENTS[shape[1]], shape[2] * e, shape[3] * e


def _plane_constants(scale, bias, channels, default_scale=1.0 / 255.0):
    """scale (default 1/255 -- decoding -- or 255 -- encoding) and bias (default 0) per channel, through numpy.float32:
    two C float arrays"""
    import numpy as np
    scale = [default_scale] * channels if scale is None else list(scale)
    bias = [0.0] * channels if bias is None else list(bias)
    if len(scale) != channels or len(bias) != channels:
        raise ValueError("scale and bias: one value per channel")
    return ((C.c_float * channels)(*[float(np.float32(v)) for v in scale]),
            (C.c_float * channels)(*[float(np.float32(v)) for v in bias]))


YCBCR_BT601, YCBCR_BT709 = 0, 1    # HapGpuYCbCrMatrix
YCBCR_LIMITED, YCBCR_FULL = 0, 1   # HapGpuYCbCrRange


def _video_planes(planes, single, rows, row_len, row_bytes, what):
    """The Y or CbCr planes of a video call: ([addresses], rowBytes, keepalive).  `planes`: one plane (single), or one
    batch tensor or a list of planes; a plane is a torch uint8 tensor on the device of (rows, row_len) bytes -- CbCr
    planes also as (rows, row_len / 2, 2) pairs -- with stride(-1) 1, whose pitch is read from it, or an integer address
    (then row_bytes says the pitch), or None (no plane for that frame)."""
    if single:
        planes = [planes]
    elif hasattr(planes, "dim"):
        planes = [planes[i] for i in range(planes.shape[0])]
    else:
        planes = list(planes)
    addresses, pitch = [], row_bytes
    for t in planes:
        if t is None or isinstance(t, int):
            addresses.append(t)
            continue
        if not (hasattr(t, "dim") and hasattr(t, "stride") and hasattr(t, "data_ptr")):
            raise ValueError("%s: torch tensors or addresses" % what)
        if str(t.dtype) != "torch.uint8":
            raise ValueError("%s: dtype uint8, not %s" % (what, t.dtype))
        if t.dim() == 3 and t.shape[2] == 2:
            shape, unit = (t.shape[0], 2 * t.shape[1]), t.stride(1) == 2 and t.stride(2) == 1
        else:
            shape, unit = tuple(t.shape), t.dim() == 2 and t.stride(1) == 1
        if shape != (rows, row_len):
            raise ValueError("%s: (%d, %d) bytes per frame, not %s" % (what, rows, row_len, tuple(t.shape)))
        if not unit:
            raise ValueError("%s: stride(-1) must be 1" % what)
        if t.device.type != "cuda":
            raise ValueError("%s: planes in device memory" % what)
        if pitch is not None and t.stride(0) != pitch:
            raise ValueError("%s: the planes of a call share their pitch" % what)
        pitch = t.stride(0)
        addresses.append(t.data_ptr())
    if pitch is None:
        raise ValueError("%s: addresses need row_bytes" % what)
    return addresses, pitch, planes


def _video_frames(luma_planes, chroma_planes, width, height, luma_row_bytes, chroma_row_bytes, outputs):
    """The planes of a video frames call: _video_planes of both, ([Y addresses], lumaRowBytes, keepalive, [CbCr addresses],
    chromaRowBytes, keepalive), one pair per output"""
    y = _video_planes(luma_planes, False, height, width, luma_row_bytes, "luma_planes")
    c = _video_planes(chroma_planes, False, height // 2, width, chroma_row_bytes, "chroma_planes")
    if len(c[0]) != len(y[0]) or outputs != len(y[0]):
        raise ValueError("one chroma plane and one output per luma plane")
    return y + c


class PictureError:
    """A HapGpuPictureError: sse and sad per channel (R, G, B, A) as tuples of ints, and texels (0: not measured)"""
    __slots__ = ("sse", "sad", "texels")

    def __init__(self, sse=(0, 0, 0, 0), sad=(0, 0, 0, 0), texels=0):
        self.sse, self.sad, self.texels = tuple(int(v) for v in sse), tuple(int(v) for v in sad), int(texels)

    def __eq__(self, other):
        return isinstance(other, PictureError) and (self.sse, self.sad, self.texels) == (other.sse, other.sad, other.texels)

    def __repr__(self):
        return "PictureError(sse=%r, sad=%r, texels=%r)" % (self.sse, self.sad, self.texels)

    def psnr(self, channels=(0, 1, 2), peak=255.0):
        """PSNR in dB over `channels` together (hap_amd.psnr)"""
        from . import psnr
        return psnr(sum(self.sse[c] for c in channels), self.texels * len(channels), peak)


def _picture_error(raw):
    return PictureError(raw.sse, raw.sad, raw.texels)


def _picture_address(picture, keep):
    """the address of a reference picture: a tensor or another buffer (kept alive in `keep`), an integer address, or None"""
    if picture is None or isinstance(picture, int):
        return picture
    address, _n, alive = _addr_len(picture)
    keep.append(alive)
    return address


def _placement_array(placements, count):
    """`count` 6-tuples (srcX, srcY, width, height, dstX, dstY) as a HapGpuPlacement array; None stays None"""
    if placements is None:
        return None
    placements = [tuple(p) for p in placements]
    if len(placements) != count or any(len(p) != 6 for p in placements):
        raise ValueError("one placement of six numbers per layer")
    return (HapGpuPlacement * max(1, count))(*[HapGpuPlacement(*p) for p in placements])


def _addr_len(buf):
    """(address, nbytes, keepalive) of a host or device buffer."""
    if buf is None:
        return None, 0, None
    if hasattr(buf, "data_ptr"):                      # torch tensor (host or device)
        return buf.data_ptr(), buf.numel() * buf.element_size(), buf
    if hasattr(buf, "ctypes") and hasattr(buf, "nbytes"):   # numpy
        return buf.ctypes.data, buf.nbytes, buf
    if isinstance(buf, (bytes, bytearray, memoryview)):
        raw = (C.c_ubyte * max(1, len(buf))).from_buffer_copy(bytes(buf) or b"\0")
        return C.addressof(raw), len(buf), raw
    if isinstance(buf, C.Array):
        return C.addressof(buf), C.sizeof(buf), buf
    raise TypeError("unsupported buffer type %r" % type(buf))


def HapMaxEncodedLength(lengths, textureFormats, chunkCounts):
    n = len(lengths)
    return lib.HapMaxEncodedLength(n, (C.c_ulong * n)(*lengths), (C.c_uint * n)(*textureFormats),
                                   (C.c_uint * n)(*chunkCounts))


def HapEncode(inputBuffers, textureFormats, compressors, chunkCounts, outputBuffer=None, outputBufferBytes=None):
    """Returns (result, frame bytes | used). With outputBuffer=None a host buffer of
    HapMaxEncodedLength() is allocated and the frame returned as bytes."""
    n = len(inputBuffers)
    infos = [_addr_len(b) for b in inputBuffers]
    ptrs = (C.c_void_p * n)(*[i[0] for i in infos])
    lens = (C.c_ulong * n)(*[i[1] for i in infos])
    own = outputBuffer is None
    if own:
        if outputBufferBytes is None:
            outputBufferBytes = HapMaxEncodedLength([i[1] for i in infos], textureFormats, chunkCounts)
        outputBuffer = (C.c_ubyte * max(1, outputBufferBytes))()
    oaddr, olen, _keep = _addr_len(outputBuffer)
    if outputBufferBytes is None:
        outputBufferBytes = olen
    used = C.c_ulong(0)
    r = lib.HapEncode(n, ptrs, lens, (C.c_uint * n)(*textureFormats), (C.c_uint * n)(*compressors),
                      (C.c_uint * n)(*chunkCounts), oaddr, outputBufferBytes, C.byref(used))
    if own:
        return r, (C.string_at(outputBuffer, used.value) if r == 0 else None)
    return r, used.value


def _serial_callback():
    def cb(fn, p, count, info):
        for i in range(count):
            fn(p, i)
    return CALLBACK(cb)


def HapDecode(inputBuffer, index=0, callback=None, outputBuffer=None, outputBufferBytes=1 << 20):
    """Returns (result, decoded bytes | used, textureFormat)."""
    iaddr, ilen, _k = _addr_len(inputBuffer)
    own = outputBuffer is None
    if own:
        outputBuffer = (C.c_ubyte * max(1, outputBufferBytes))()
    oaddr, olen, _k2 = _addr_len(outputBuffer)
    if not own:
        outputBufferBytes = olen
    used = C.c_ulong(0)
    fmt = C.c_uint(0)
    cb = callback if callback is not None else _serial_callback()
    r = lib.HapDecode(iaddr, ilen, index, cb, None, oaddr, outputBufferBytes, C.byref(used), C.byref(fmt))
    if own:
        return r, (C.string_at(outputBuffer, used.value) if r == 0 else None), fmt.value
    return r, used.value, fmt.value


def HapGetFrameTextureCount(frame):
    a, n, _k = _addr_len(frame)
    out = C.c_uint(0)
    return lib.HapGetFrameTextureCount(a, n, C.byref(out)), out.value


def HapGetFrameTextureFormat(frame, index):
    a, n, _k = _addr_len(frame)
    out = C.c_uint(0)
    return lib.HapGetFrameTextureFormat(a, n, index, C.byref(out)), out.value


def HapGetFrameTextureChunkCount(frame, index):
    a, n, _k = _addr_len(frame)
    out = C.c_int(-1)
    return lib.HapGetFrameTextureChunkCount(a, n, index, C.byref(out)), out.value


def HapGpuGetFrameTextureChunkLayout(frame, index):
    """Returns (result, [decoded offset of every chunk ..., decoded size of the texture])."""
    a, n, _k = _addr_len(frame)
    r, count = HapGetFrameTextureChunkCount(frame, index)
    cap = max(1, count) + 1 if r == 0 else 2
    offs = (C.c_ulong * cap)()
    got = C.c_uint(0)
    r = lib.HapGpuGetFrameTextureChunkLayout(a, n, index, cap, offs, C.byref(got))
    return r, (list(offs[: got.value + 1]) if r == 0 else None)


def region_needs_bytes(width, block_bytes, region, first_byte, byte_count):
    """True if bytes [first_byte, first_byte + byte_count) of a `width`-wide texture of `block_bytes`-byte blocks hold a
    byte of a block of region = (x, y, w, h) (HapGpuRegionNeedsBytes: needs no GPU)."""
    x, y, w, h = region
    return bool(lib.HapGpuRegionNeedsBytes(width, block_bytes, x, y, w, h, first_byte, byte_count))


def HapGpuJoinChunkGroups(groupFrames, outputBufferBytes=None):
    """Joins frames holding consecutive chunk groups (host buffers). Returns (result, frame bytes | None)."""
    infos = [_addr_len(f) for f in groupFrames]
    n = len(infos)
    if outputBufferBytes is None:
        outputBufferBytes = sum(i[1] for i in infos) + 64
    out = (C.c_ubyte * max(1, outputBufferBytes))()
    used = C.c_ulong(0)
    r = lib.HapGpuJoinChunkGroups(n, (C.c_void_p * max(1, n))(*[i[0] for i in infos]),
                                  (C.c_ulong * max(1, n))(*[i[1] for i in infos]), out, outputBufferBytes, C.byref(used))
    return r, (C.string_at(out, used.value) if r == 0 else None)


class SequenceWriter:
    """include/hap_sequence.h: append complete Hap frames to a sequence file."""

    def __init__(self, path, width=0, height=0, rate=(60, 1)):
        h = C.c_void_p()
        r = lib.HapSequenceWriterOpen(os.fsencode(path), width, height, rate[0], rate[1], C.byref(h))
        if r != 0:
            raise OSError("HapSequenceWriterOpen(%r) failed with HapResult %d" % (path, r))
        self.handle = h

    def append(self, frame):
        a, n, _k = _addr_len(frame)
        return lib.HapSequenceWriterAppend(self.handle, a, n)

    def close(self):
        r = 0
        if self.handle:
            r = lib.HapSequenceWriterClose(self.handle)
            self.handle = None
        return r

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SequenceReader:
    """include/hap_sequence.h: random access to the frames of a sequence file."""

    def __init__(self, path):
        h = C.c_void_p()
        r = lib.HapSequenceReaderOpen(os.fsencode(path), C.byref(h))
        if r != 0:
            raise OSError("HapSequenceReaderOpen(%r) failed with HapResult %d" % (path, r))
        self.handle = h
        v = [C.c_uint(0) for _ in range(5)]
        lib.HapSequenceReaderInfo(h, *[C.byref(x) for x in v])
        self.width, self.height, self.rate, self.frame_count = v[0].value, v[1].value, (v[2].value, v[3].value), v[4].value

    def frame_bytes(self, i):
        return lib.HapSequenceReaderFrameBytes(self.handle, i)

    def read(self, first, count=1):
        """Returns (result, [frame bytes, ...])."""
        total = sum(self.frame_bytes(first + i) for i in range(count)) if first + count <= self.frame_count else 0
        buf = (C.c_ubyte * max(1, total))()
        offs = (C.c_ulong * (count + 1))()
        r = lib.HapSequenceReaderRead(self.handle, first, count, buf, total, offs)
        if r != 0:
            return r, None
        raw = C.string_at(buf, total)
        return 0, [raw[offs[i]:offs[i + 1]] for i in range(count)]

    def close(self):
        if self.handle:
            lib.HapSequenceReaderClose(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BufferList:
    """A list of buffers whose addresses and sizes are looked up once: pass it wherever the batched calls take
    a list of buffers that stay in place from call to call (a C client simply keeps its pointer array)."""

    def __init__(self, buffers):
        self.buffers = list(buffers)
        self.infos = [_addr_len(b) for b in self.buffers]
        self.pointers = (C.c_void_p * len(self.buffers))(*[i[0] for i in self.infos])

    def __len__(self):
        return len(self.buffers)

    def __getitem__(self, i):
        return self.buffers[i]


class Context:
    """HapGpuContext: device + stream + scratch (include/hap_gpu.h)."""

    def __init__(self, device=-1):
        h = C.c_void_p()
        r = lib.HapGpuCreate(device, C.byref(h))
        if r != 0:
            raise RuntimeError("HapGpuCreate failed with HapResult %d (no usable HIP device?)" % r)
        self.handle = h

    def close(self):
        if self.handle:
            lib.HapGpuDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_fragment_log2(self, v):
        return lib.HapGpuSetFragmentLog2(self.handle, v)

    def synchronize(self):
        return lib.HapGpuSynchronize(self.handle)

    def resolved_blocks(self):
        """64 KiB blocks of other encoders' streams decoded by a workgroup each (HapGpuResolvedBlockCount)"""
        return int(lib.HapGpuResolvedBlockCount(self.handle))

    def skipped_texture_bytes(self):
        """decoded bytes of the pieces this context's region calls left undecoded (HapGpuSkippedTextureBytes)"""
        return int(lib.HapGpuSkippedTextureBytes(self.handle))

    def placement_retries(self):
        """frames encoded a second time because one of their chunks did not shrink (HapGpuPlacementRetryCount)"""
        return int(lib.HapGpuPlacementRetryCount(self.handle))

    def placement_timeouts(self):
        """... of which because a wavefront gave up waiting for its predecessors' sizes (HapGpuPlacementTimeoutCount)"""
        return int(lib.HapGpuPlacementTimeoutCount(self.handle))

    def table_fallbacks(self):
        """frames decoded a second time because their fragment table did not describe their streams"""
        return int(lib.HapGpuTableFallbackCount(self.handle))

    def compress_rgba(self, rgba, width, height, row_bytes, texture_format, output=None, flags=0):
        """RGBA8 -> one block texture (HapGpuCompressRGBA; with nonzero flags HapGpuCompressRGBAFlags, where
        ENCODE_BPTC_BLOCKS admits RGBA_BPTC_UNORM and ENCODE_REFINE_ENDPOINTS makes the colour blocks of RGB_DXT1 and
        RGBA_DXT5 with least-squares refined end points: slower, never a larger error in any block, the other formats
        unchanged).  Returns (result, bytes | None), or (result, bytes used) into `output`."""
        block = 8 if texture_format in (HapTextureFormat.RGB_DXT1, HapTextureFormat.A_RGTC1) else 16
        need = (width // 4) * (height // 4) * block
        a, _n, _k = _addr_len(rgba)
        own = output is None
        if own:
            output = (C.c_ubyte * max(1, need))()
        oa, on, _k2 = _addr_len(output)
        used = C.c_ulong(0)
        if flags:
            r = lib.HapGpuCompressRGBAFlags(self.handle, a, width, height, row_bytes, texture_format, flags, oa, on, C.byref(used))
        else:
            r = lib.HapGpuCompressRGBA(self.handle, a, width, height, row_bytes, texture_format, oa, on, C.byref(used))
        if own:
            return r, (C.string_at(output, used.value) if r == 0 else None)
        return r, used.value

    def compress_rgba_half(self, rgba_half, width, height, row_bytes, texture_format, output=None):
        """RGBA16F picture (numpy uint16 / float16, bytes-like or torch, host or device) -> one BC6H texture
        (HapGpuCompressRGBAHalf; texture_format RGB_BPTC_UNSIGNED_FLOAT or RGB_BPTC_SIGNED_FLOAT).  Returns
        (result, bytes | None), or (result, bytes used) into `output`."""
        need = (width // 4) * (height // 4) * 16
        a, _n, _k = _addr_len(rgba_half)
        own = output is None
        if own:
            output = (C.c_ubyte * max(1, need))()
        oa, on, _k2 = _addr_len(output)
        used = C.c_ulong(0)
        r = lib.HapGpuCompressRGBAHalf(self.handle, a, width, height, row_bytes, texture_format, oa, on, C.byref(used))
        if own:
            return r, (C.string_at(output, used.value) if r == 0 else None)
        return r, used.value

    def compress_alpha(self, alpha, width, height, row_bytes, output=None):
        """A8 picture (one byte a texel; numpy uint8, bytes-like or torch, host or device) -> one A_RGTC1 texture
        (HapGpuCompressAlpha).  Returns (result, bytes | None), or (result, bytes used) into `output`."""
        need = (width // 4) * (height // 4) * 8
        a, _n, _k = _addr_len(alpha)
        own = output is None
        if own:
            output = (C.c_ubyte * max(1, need))()
        oa, on, _k2 = _addr_len(output)
        used = C.c_ulong(0)
        r = lib.HapGpuCompressAlpha(self.handle, a, width, height, row_bytes, oa, on, C.byref(used))
        if own:
            return r, (C.string_at(output, used.value) if r == 0 else None)
        return r, used.value

    def decompress_rgba(self, texture, texture_format, width, height, rgba=None, alpha=None, row_bytes=None):
        """Texture (+ optional RGTC1 alpha plane) -> RGBA8. Returns (result, bytes | None)."""
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        row_bytes = row_bytes or width * 4
        own = rgba is None
        if own:
            rgba = (C.c_ubyte * (row_bytes * height + 16))()
            base = C.addressof(rgba)
            pad = (-base) % 16
            oa = base + pad
        else:
            oa, _on, _k3 = _addr_len(rgba)
        r = lib.HapGpuDecompressRGBA(self.handle, ta, tn, texture_format, aa, an, width, height, oa, row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * height) if r == 0 else None)
        return r, None

    def measure_texture(self, texture, texture_format, width, height, picture, alpha=None, row_bytes=None):
        """Texture (+ optional RGTC1 alpha plane) against `picture`, an RGBA8 picture in device memory (a tensor or an
        address): per channel the exact sums of (d - p)^2 and |d - p|, d being decompress_rgba's byte
        (HapGpuMeasureTexture).  Returns (result, PictureError | None)."""
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        keep = []
        raw = HapGpuPictureError()
        r = lib.HapGpuMeasureTexture(self.handle, ta, tn, texture_format, aa, an, width, height,
                                     _picture_address(picture, keep), width * 4 if row_bytes is None else row_bytes,
                                     C.byref(raw))
        return r, (_picture_error(raw) if r == 0 else None)

    def decompress_rgba_scaled(self, texture, texture_format, width, height, scale_log2, rgba=None, alpha=None,
                               row_bytes=None):
        """Texture (+ optional RGTC1 alpha plane) -> the half- (scale_log2 1) or quarter-size (2) RGBA8 picture of
        (width >> scale_log2) x (height >> scale_log2): the rounded-up box mean of decompress_rgba's texels
        (HapGpuDecompressRGBAScaled).  Returns (result, bytes | None)."""
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        shift = scale_log2 if 0 < scale_log2 < 3 else 0          # (a refused scale: nothing is written)
        row_bytes = row_bytes or (width >> shift) * 4
        rows = height >> shift
        own = rgba is None
        if own:
            rgba = (C.c_ubyte * (row_bytes * rows + 16))()
            base = C.addressof(rgba)
            oa = base + (-base) % 16
        else:
            oa, _on, _k3 = _addr_len(rgba)
        r = lib.HapGpuDecompressRGBAScaled(self.handle, ta, tn, texture_format, aa, an, width, height, scale_log2, oa,
                                           row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * rows) if r == 0 else None)
        return r, None

    def decompress_planes(self, texture, texture_format, width, height, out, scale_log2=0, scale=None, bias=None,
                          alpha=None):
        """Texture (+ optional RGTC1 alpha plane) -> `out`, a (C, height >> scale_log2, width >> scale_log2) float16,
        bfloat16 or float32 torch tensor on the device, C 3 or 4: element = float32(byte) * scale[c] + bias[c] (two
        roundings), the byte being decompress_rgba[_scaled]'s (HapGpuDecompressPlanes).  channels, element, planeBytes and
        rowBytes are read from the tensor, so a slice with longer rows or planes is accepted; stride(-1) must be 1.
        scale defaults to 1/255 per channel, bias to 0.  Returns the result."""
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, True, width, height, scale_log2)
        sc, bi = _plane_constants(scale, bias, channels)
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        return lib.HapGpuDecompressPlanes(self.handle, ta, tn, texture_format, aa, an, width, height, scale_log2, channels,
                                          element, tensors[0].data_ptr(), plane_bytes, row_bytes, sc, bi)

    def decompress_planes_region(self, texture, texture_format, width, height, region, out, scale_log2=0, scale=None,
                                 bias=None, alpha=None):
        """Texture (+ optional RGTC1 alpha plane) -> `out`, the (C, h >> scale_log2, w >> scale_log2) tensor of region =
        (x, y, w, h), a block-aligned rectangle of the texture: bit for bit that crop of decompress_planes' tensor, from
        the rectangle's blocks alone (HapGpuDecompressPlanesRegion).  `out`, scale and bias as for decompress_planes.
        Returns the result."""
        x, y, w, h = region
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, True, w, h, scale_log2)
        sc, bi = _plane_constants(scale, bias, channels)
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        return lib.HapGpuDecompressPlanesRegion(self.handle, ta, tn, texture_format, aa, an, width, height, x, y, w, h,
                                                scale_log2, channels, element, tensors[0].data_ptr(), plane_bytes,
                                                row_bytes, sc, bi)

    def decompress_planes_resized(self, texture, texture_format, width, height, crop, out, scale_log2=0, scale=None,
                                  bias=None, alpha=None):
        """Texture (+ optional RGTC1 alpha plane) -> `out`, a (C, out_h, out_w) tensor: crop = (x, y, w, h), at any texel
        position and size of the (width >> scale_log2) x (height >> scale_log2) picture, resized to the tensor's size by
        the integer bilinear filter of HapGpuDecodeFramesPlanesResized (HapGpuDecompressPlanesResized).  channels, element,
        strides and the output size are read from the tensor; scale and bias as for decompress_planes.  Returns the
        result."""
        x, y, w, h = crop
        if not hasattr(out, "shape") or len(out.shape) != 3:
            raise ValueError("out: one (C, out_h, out_w) tensor")
        out_h, out_w = int(out.shape[1]), int(out.shape[2])
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, True, out_w, out_h, 0)
        sc, bi = _plane_constants(scale, bias, channels)
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        return lib.HapGpuDecompressPlanesResized(self.handle, ta, tn, texture_format, aa, an, width, height, scale_log2,
                                                 x, y, w, h, out_w, out_h, channels, element, tensors[0].data_ptr(),
                                                 plane_bytes, row_bytes, sc, bi)

    def compress_planes(self, planes, width, height, texture_format, scale=None, bias=None, output=None):
        """`planes`, a (C, height, width) float16, bfloat16 or float32 torch tensor on the device, C 3 or 4 -> one block
        texture (HapGpuCompressPlanes): byte = float32(element) * scale[c] + bias[c] (two roundings), NaN and anything
        not above 0 to 0, 255 and above to 255, else to nearest with halves to even; compress_rgba's texture of the
        picture of those bytes (A 255 with C 3).  texture_format RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 or A_RGTC1.  channels,
        element, planeBytes and rowBytes are read from the tensor, so a slice with longer rows or planes is accepted;
        stride(-1) must be 1.  scale defaults to 255 per channel, bias to 0.  Returns (result, bytes | None), or
        (result, bytes used) into `output`."""
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(planes, True, width, height, 0)
        sc, bi = _plane_constants(scale, bias, channels, 255.0)
        block = 8 if texture_format in (HapTextureFormat.RGB_DXT1, HapTextureFormat.A_RGTC1) else 16
        need = (width // 4) * (height // 4) * block
        own = output is None
        if own:
            output = (C.c_ubyte * max(1, need))()
        oa, on, _k = _addr_len(output)
        used = C.c_ulong(0)
        r = lib.HapGpuCompressPlanes(self.handle, tensors[0].data_ptr(), plane_bytes, row_bytes, channels, element, sc, bi,
                                     width, height, texture_format, oa, on, C.byref(used))
        if own:
            return r, (C.string_at(output, used.value) if r == 0 else None)
        return r, used.value

    def decompress_rgba_region(self, texture, texture_format, width, height, region, rgba=None, alpha=None,
                               row_bytes=None):
        """Texture (+ optional RGTC1 alpha plane) -> the RGBA8 picture of region = (x, y, w, h), a block-aligned rectangle
        of it: the crop of decompress_rgba's picture (HapGpuDecompressRGBARegion).  Returns (result, bytes | None)."""
        x, y, w, h = region
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        row_bytes = w * 4 if row_bytes is None else row_bytes
        own = rgba is None
        if own:
            rgba = (C.c_ubyte * (row_bytes * max(h, 1) + 16))()
            base = C.addressof(rgba)
            oa = base + (-base) % 16
        else:
            oa, _on, _k3 = _addr_len(rgba)
        r = lib.HapGpuDecompressRGBARegion(self.handle, ta, tn, texture_format, aa, an, width, height, x, y, w, h, oa,
                                           row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * h) if r == 0 else None)
        return r, None

    def decompress_rgba_half(self, texture, texture_format, width, height, out=None, row_bytes=None):
        """BC6H texture -> RGBA16F (four half bit patterns per texel, alpha 1.0). Returns (result, bytes | None):
        the picture's bytes when `out` is None, else None (the picture is in `out`: numpy or torch, host or device,
        e.g. a torch.float16 (H, W, 4) CUDA tensor)."""
        ta, tn, _k = _addr_len(texture)
        row_bytes = row_bytes or width * 8
        own = out is None
        if own:
            out = (C.c_ubyte * (row_bytes * height + 16))()
            base = C.addressof(out)
            oa = base + (-base) % 16
        else:
            oa, _on, _k2 = _addr_len(out)
        r = lib.HapGpuDecompressRGBAHalf(self.handle, ta, tn, texture_format, width, height, oa, row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * height) if r == 0 else None)
        return r, None

    def decompress_alpha(self, texture, width, height, out=None, row_bytes=None):
        """A_RGTC1 texture -> A8 picture (HapGpuDecompressAlpha). Returns (result, bytes | None): the picture's bytes
        (rows row_bytes apart) when `out` is None, else None (the picture is in `out`: numpy or torch, host or
        device)."""
        ta, tn, _k = _addr_len(texture)
        row_bytes = row_bytes or width
        own = out is None
        if own:
            out = (C.c_ubyte * (row_bytes * height + 16))()
            base = C.addressof(out)
            oa = base + (-base) % 16
        else:
            oa, _on, _k2 = _addr_len(out)
        r = lib.HapGpuDecompressAlpha(self.handle, ta, tn, width, height, oa, row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * height) if r == 0 else None)
        return r, None

    def decode_chunk_group(self, frame, index, first_chunk, chunk_count, output):
        """Decodes chunks [first_chunk, first_chunk + chunk_count) into their place in `output`
        (laid out as the whole texture). Returns (result, texture bytes, format)."""
        ia, il, _k = _addr_len(frame)
        oa, ol, _k2 = _addr_len(output)
        used = C.c_ulong(0)
        fmt = C.c_uint(0)
        r = lib.HapGpuDecodeChunkGroup(self.handle, ia, il, index, first_chunk, chunk_count, oa, ol,
                                       C.byref(used), C.byref(fmt))
        return r, used.value, fmt.value

    @staticmethod
    def _ptr_array(bufs):
        if isinstance(bufs, BufferList):          # addresses resolved once, reused call after call
            return bufs.pointers, bufs.infos
        infos = [_addr_len(b) for b in bufs]
        return (C.c_void_p * len(bufs))(*[i[0] for i in infos]), infos

    def encode_frames(self, textures, formats, compressors, chunk_counts, outputs, flags=0):
        """textures: list (frames) of lists (count) of buffers; outputs: list of buffers.
        Returns (result, used[], results[])."""
        nf, count = len(textures), len(formats)
        flat = [t for fr in textures for t in fr]
        ptrs, infos = self._ptr_array(flat)
        lens = (C.c_ulong * count)(*[infos[i][1] for i in range(count)])
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuEncodeFrames(self.handle, nf, count, ptrs, lens, (C.c_uint * count)(*formats),
                                   (C.c_uint * count)(*compressors), (C.c_uint * count)(*chunk_counts),
                                   optrs, olens, used, results, flags)
        return r, list(used), list(results)

    def encode_frames_rgba(self, rgba_frames, width, height, row_bytes, formats, compressors, chunk_counts,
                           outputs, flags=0):
        """RGBA8 pictures -> frames in one call (HapGpuEncodeFramesRGBA).  flags: the ENCODE_* bits; with
        ENCODE_REFINE_ENDPOINTS the textures of [RGB_DXT1] and [RGBA_DXT5] frames are compress_rgba's with that flag (the
        quality tier of Hap and Hap Alpha; every other format, and frames of two textures, as without it).  Returns
        (result, used[], results[])."""
        nf, count = len(rgba_frames), len(formats)
        ptrs, _infos = self._ptr_array(rgba_frames)
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuEncodeFramesRGBA(self.handle, nf, ptrs, width, height, row_bytes, count,
                                       (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors),
                                       (C.c_uint * count)(*chunk_counts), optrs, olens, used, results, flags)
        return r, list(used), list(results)

    def encode_frames_rgba_begin(self, rgba_frames, width, height, row_bytes, formats, compressors, chunk_counts,
                                 outputs, flags=0):
        """First half of encode_frames_rgba (HapGpuEncodeFramesRGBABegin): everything launched, nothing waited for.
        The context takes no other call until encode_finish(), which returns what encode_frames_rgba returns."""
        nf, count = len(rgba_frames), len(formats)
        ptrs, _infos = self._ptr_array(rgba_frames)
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuEncodeFramesRGBABegin(self.handle, nf, ptrs, width, height, row_bytes, count,
                                            (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors),
                                            (C.c_uint * count)(*chunk_counts), optrs, olens, used, results, flags)
        self._pending = (used, results, ptrs, optrs, olens, rgba_frames, outputs)     # alive until the second half
        return r

    def _encode_planes(self, fn, described, width, height, formats, compressors, chunk_counts, outputs, scale, bias, flags):
        tensors, channels, element, plane_bytes, row_bytes = described
        nf, count = len(tensors), len(formats)
        if len(outputs) != nf:
            raise ValueError("one output per tensor")
        sc, bi = _plane_constants(scale, bias, channels, 255.0)
        ptrs = (C.c_void_p * nf)(*[None if t is None else t.data_ptr() for t in tensors])
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = fn(self.handle, nf, ptrs, channels, element, plane_bytes, row_bytes, sc, bi, width, height, count,
               (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors), (C.c_uint * count)(*chunk_counts),
               optrs, olens, used, results, flags)
        return r, used, results, (ptrs, optrs, olens, tensors, outputs)

    def encode_frames_planes(self, planes, width, height, formats, compressors, chunk_counts, outputs, scale=None,
                             bias=None, flags=0):
        """Planar tensors -> frames in one call, without RGBA8 pictures in between (HapGpuEncodeFramesPlanes).  `planes`:
        one (N, C, height, width) torch tensor on the device or a list of N (C, H, W) ones that share their strides
        (None: no tensor for that frame), float16, bfloat16 or float32, C 3 or 4; channels, element, planeBytes and
        rowBytes are read from it, stride(-1) must be 1.  byte = float32(element) * scale[c] + bias[c] (two roundings),
        NaN and anything not above 0 to 0, 255 and above to 255, else to nearest with halves to even; the frames are
        encode_frames_rgba's of the pictures of those bytes.  formats: [RGB_DXT1], [RGBA_DXT5], [YCoCg_DXT5], [A_RGTC1]
        or [YCoCg_DXT5, A_RGTC1].  scale defaults to 255 per channel, bias to 0.  flags: encode_frames_rgba's,
        ENCODE_REFINE_ENDPOINTS included (ENCODE_BPTC_BLOCKS is ignored).  Returns (result, used[], results[])."""
        described = _plane_tensors(planes, False, width, height, 0)               # (refusals first: no context needed)
        r, used, results, _keep = self._encode_planes(lib.HapGpuEncodeFramesPlanes, described, width, height, formats,
                                                      compressors, chunk_counts, outputs, scale, bias, flags)
        return r, list(used), list(results)

    def encode_frames_planes_begin(self, planes, width, height, formats, compressors, chunk_counts, outputs, scale=None,
                                   bias=None, flags=0):
        """First half of encode_frames_planes (HapGpuEncodeFramesPlanesBegin); encode_finish() is the second."""
        described = _plane_tensors(planes, False, width, height, 0)
        r, used, results, keep = self._encode_planes(lib.HapGpuEncodeFramesPlanesBegin, described, width, height, formats,
                                                     compressors, chunk_counts, outputs, scale, bias, flags)
        self._pending = (used, results) + keep                                      # alive until the second half
        return r

    def compress_nv12(self, luma, chroma, width, height, texture_format, matrix=YCBCR_BT709, range=YCBCR_LIMITED,
                      luma_row_bytes=None, chroma_row_bytes=None, output=None):
        """One NV12 video picture on the device -> one block texture (HapGpuCompressNV12).  `luma`: a (height, width)
        torch uint8 tensor, `chroma`: a (height / 2, width) one or (height / 2, width / 2, 2) Cb, Cr pairs; stride(-1)
        must be 1 and the pitches are read from the tensors (a slice with longer rows is accepted), or integer addresses
        with luma_row_bytes / chroma_row_bytes.  Texel (x, y) is the integer conversion of Y[y][x] and the pair at
        [y >> 1][x >> 1] under matrix (YCBCR_BT601, YCBCR_BT709) and range (YCBCR_LIMITED, YCBCR_FULL), A 255; the
        texture is compress_rgba's of that picture.  texture_format RGB_DXT1 or YCoCg_DXT5.  Returns
        (result, bytes | None), or (result, bytes used) into `output`."""
        ya, luma_row_bytes, _k1 = _video_planes(luma, True, height, width, luma_row_bytes, "luma")
        ca, chroma_row_bytes, _k2 = _video_planes(chroma, True, height // 2, width, chroma_row_bytes, "chroma")
        need = (width // 4) * (height // 4) * (8 if texture_format == HapTextureFormat.RGB_DXT1 else 16)
        own = output is None
        if own:
            output = (C.c_ubyte * max(1, need))()
        oa, on, _k = _addr_len(output)
        used = C.c_ulong(0)
        r = lib.HapGpuCompressNV12(self.handle, ya[0], luma_row_bytes, ca[0], chroma_row_bytes, matrix, range, width,
                                   height, texture_format, oa, on, C.byref(used))
        if own:
            return r, (C.string_at(output, used.value) if r == 0 else None)
        return r, used.value

    def _encode_nv12(self, fn, described, width, height, formats, compressors, chunk_counts, outputs, matrix, range, flags):
        ya, luma_row_bytes, keep_y, ca, chroma_row_bytes, keep_c = described
        nf, count = len(ya), len(formats)
        yptrs, cptrs = (C.c_void_p * nf)(*ya), (C.c_void_p * nf)(*ca)
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = fn(self.handle, nf, yptrs, luma_row_bytes, cptrs, chroma_row_bytes, matrix, range, width, height, count,
               (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors), (C.c_uint * count)(*chunk_counts),
               optrs, olens, used, results, flags)
        return r, used, results, (yptrs, cptrs, optrs, olens, keep_y, keep_c, outputs)

    def encode_frames_nv12(self, luma_planes, chroma_planes, width, height, formats, compressors, chunk_counts, outputs,
                           matrix=YCBCR_BT709, range=YCBCR_LIMITED, luma_row_bytes=None, chroma_row_bytes=None, flags=0):
        """NV12 video pictures on the device -> frames in one call, without RGBA8 pictures in between
        (HapGpuEncodeFramesNV12).  luma_planes / chroma_planes: one (N, height, width) / (N, height / 2, width) torch
        uint8 tensor each, or lists of N planes as compress_nv12 takes them that share their pitch (None: no plane for
        that frame; integer addresses with luma_row_bytes / chroma_row_bytes).  The frames are encode_frames_rgba's of
        the converted pictures.  formats: [RGB_DXT1] or [YCoCg_DXT5].  flags: encode_frames_rgba's,
        ENCODE_REFINE_ENDPOINTS included (ENCODE_BPTC_BLOCKS is ignored).  Returns (result, used[], results[])."""
        described = _video_frames(luma_planes, chroma_planes, width, height, luma_row_bytes, chroma_row_bytes,
                                  len(outputs))                                     # (refusals first: no context needed)
        r, used, results, _keep = self._encode_nv12(lib.HapGpuEncodeFramesNV12, described, width, height, formats,
                                                    compressors, chunk_counts, outputs, matrix, range, flags)
        return r, list(used), list(results)

    def encode_frames_nv12_begin(self, luma_planes, chroma_planes, width, height, formats, compressors, chunk_counts,
                                 outputs, matrix=YCBCR_BT709, range=YCBCR_LIMITED, luma_row_bytes=None,
                                 chroma_row_bytes=None, flags=0):
        """First half of encode_frames_nv12 (HapGpuEncodeFramesNV12Begin); encode_finish() is the second."""
        described = _video_frames(luma_planes, chroma_planes, width, height, luma_row_bytes, chroma_row_bytes,
                                  len(outputs))
        r, used, results, keep = self._encode_nv12(lib.HapGpuEncodeFramesNV12Begin, described, width, height, formats,
                                                   compressors, chunk_counts, outputs, matrix, range, flags)
        self._pending = (used, results) + keep                                      # alive until the second half
        return r

    def _encode_half(self, fn, rgba_half_frames, width, height, row_bytes, texture_format, compressor, chunk_count,
                     outputs, flags):
        nf = len(rgba_half_frames)
        ptrs, infos = self._ptr_array(rgba_half_frames)
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = fn(self.handle, nf, ptrs, width, height, row_bytes, texture_format, compressor, chunk_count, optrs, olens,
               used, results, flags)
        return r, used, results, (ptrs, optrs, olens, infos, oinfos)

    def encode_frames_rgba_half(self, rgba_half_frames, width, height, row_bytes, texture_format, compressor,
                                chunk_count, outputs, flags=0):
        """RGBA16F pictures -> Hap HDR frames of one BC6H texture (HapGpuEncodeFramesRGBAHalf).  Returns
        (result, used[], results[])."""
        r, used, results, _keep = self._encode_half(lib.HapGpuEncodeFramesRGBAHalf, rgba_half_frames, width, height,
                                                    row_bytes, texture_format, compressor, chunk_count, outputs, flags)
        return r, list(used), list(results)

    def encode_frames_rgba_half_begin(self, rgba_half_frames, width, height, row_bytes, texture_format, compressor,
                                      chunk_count, outputs, flags=0):
        """First half of encode_frames_rgba_half (HapGpuEncodeFramesRGBAHalfBegin); encode_finish() is the second."""
        r, used, results, keep = self._encode_half(lib.HapGpuEncodeFramesRGBAHalfBegin, rgba_half_frames, width, height,
                                                   row_bytes, texture_format, compressor, chunk_count, outputs, flags)
        self._pending = (used, results) + keep                                      # alive until the second half
        return r

    def _encode_alpha(self, fn, alpha_frames, width, height, row_bytes, compressor, chunk_count, outputs, flags):
        nf = len(alpha_frames)
        ptrs, infos = self._ptr_array(alpha_frames)
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = fn(self.handle, nf, ptrs, width, height, row_bytes, compressor, chunk_count, optrs, olens, used, results, flags)
        return r, used, results, (ptrs, optrs, olens, infos, oinfos)

    def encode_frames_alpha(self, alpha_frames, width, height, row_bytes, compressor, chunk_count, outputs, flags=0):
        """A8 pictures -> Hap Alpha-Only frames of one A_RGTC1 texture (HapGpuEncodeFramesAlpha).  Returns
        (result, used[], results[])."""
        r, used, results, _keep = self._encode_alpha(lib.HapGpuEncodeFramesAlpha, alpha_frames, width, height, row_bytes,
                                                     compressor, chunk_count, outputs, flags)
        return r, list(used), list(results)

    def encode_frames_alpha_begin(self, alpha_frames, width, height, row_bytes, compressor, chunk_count, outputs, flags=0):
        """First half of encode_frames_alpha (HapGpuEncodeFramesAlphaBegin); encode_finish() is the second."""
        r, used, results, keep = self._encode_alpha(lib.HapGpuEncodeFramesAlphaBegin, alpha_frames, width, height,
                                                    row_bytes, compressor, chunk_count, outputs, flags)
        self._pending = (used, results) + keep                                      # alive until the second half
        return r

    def encode_finish(self):
        r = lib.HapGpuEncodeFramesFinish(self.handle)
        pending, self._pending = getattr(self, "_pending", None), None
        if pending is None:
            return r, [], []
        return r, list(pending[0]), list(pending[1])

    def decode_frames(self, frames, frame_bytes, index, outputs, flags=0):
        nf = len(frames)
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        fmts = (C.c_uint * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFrames(self.handle, nf, ptrs, lens, index, optrs, olens, used, fmts, results, flags)
        return r, list(used), list(fmts), list(results)

    def decode_frame_textures(self, frames, frame_bytes, texture_count, outputs, flags=0):
        """All textures of every frame in one batch (HapGpuDecodeFrameTextures).  outputs[f * texture_count + t].
        Returns (result, used[], formats[], results[]), one entry per frame and texture."""
        nf = len(frames)
        n = nf * texture_count
        if len(outputs) != n:
            raise ValueError("outputs must hold frames x textures buffers")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * n)(*[i[1] for i in oinfos])
        used = (C.c_ulong * n)()
        fmts = (C.c_uint * n)()
        results = (C.c_uint * n)()
        r = lib.HapGpuDecodeFrameTextures(self.handle, nf, ptrs, lens, texture_count, optrs, olens, used, fmts, results, flags)
        return r, list(used), list(fmts), list(results)

    def decode_frames_rgba(self, frames, frame_bytes, texture_count, rgba_frames, width, height, row_bytes=None, flags=0):
        """Frames -> RGBA8 pictures in one call (HapGpuDecodeFramesRGBA).  Returns (result, results[])."""
        nf = len(frames)
        if len(rgba_frames) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, _oinfos = self._ptr_array(rgba_frames)
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesRGBA(self.handle, nf, ptrs, lens, texture_count, optrs, width, height,
                                       row_bytes or width * 4, results, flags)
        return r, list(results)

    def composite_textures(self, layers, width, height, opacities=None, background=None, rgba=None, row_bytes=None):
        """Layers of textures "over" a background colour -> one RGBA8 picture (HapGpuCompositeTextures).  layers: a list,
        bottom to top, of (texture, format, alpha plane or None); opacities: a byte per layer (None: all 255); background:
        (R, G, B, A) bytes (None: 0, 0, 0, 255).  Per texel, with the layer's decompress_rgba bytes (Rs, Gs, Bs, As):
        a = rdiv255(As * o), Cd = rdiv255(Cs * a + Cd * (255 - a)), Ad = a + rdiv255(Ad * (255 - a)), in integers.
        Returns (result, bytes | None), or (result, None) into `rgba`."""
        n = len(layers)
        infos = [_addr_len(t) for t, _f, _a in layers]
        ainfos = [_addr_len(a) for _t, _f, a in layers]
        ptrs = (C.c_void_p * n)(*[i[0] for i in infos])
        lens = (C.c_ulong * n)(*[i[1] for i in infos])
        fmts = (C.c_uint * n)(*[f for _t, f, _a in layers])
        aptrs = (C.c_void_p * n)(*[i[0] for i in ainfos])
        alens = (C.c_ulong * n)(*[i[1] for i in ainfos])
        ops = (C.c_ubyte * n)(*opacities) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        row_bytes = row_bytes or width * 4
        own = rgba is None
        if own:
            rgba = (C.c_ubyte * (row_bytes * height + 16))()
            base = C.addressof(rgba)
            oa = base + (-base) % 16
        else:
            oa, _on, _k = _addr_len(rgba)
        r = lib.HapGpuCompositeTextures(self.handle, n, ptrs, lens, fmts, aptrs, alens, ops, bg, width, height, oa, row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * height) if r == 0 else None)
        return r, None

    def composite_frames(self, frames, frame_bytes, texture_counts, rgba_frames, width, height, opacities=None,
                         background=None, row_bytes=None, flags=0):
        """Layers of Hap frames "over" a background colour -> one RGBA8 picture per output frame in one call
        (HapGpuCompositeFrames).  frames: a list (output frames) of lists (layers, bottom to top) of buffers; frame_bytes
        likewise (None entries, or None for all: the buffers' sizes); texture_counts: 1 or 2 per layer (None: all 1);
        opacities: a list per output frame of a byte per layer (None: all 255); background: (R, G, B, A) (None:
        0, 0, 0, 255).  The definition is composite_textures' with decode_frames_rgba's bytes.
        Returns (result, results[]): one entry per output frame and layer, entry f * layers + l."""
        nf = len(frames)
        nl = len(frames[0]) if nf else 0
        if len(rgba_frames) != nf:
            raise ValueError("one picture per output frame")
        if any(len(fr) != nl for fr in frames):
            raise ValueError("every output frame has the same number of layers")
        flat = [b for fr in frames for b in fr]
        ptrs, infos = self._ptr_array(flat)
        given = [None] * len(flat) if frame_bytes is None else [b for fr in frame_bytes for b in fr]
        lens = (C.c_ulong * len(flat))(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(given)])
        counts = (C.c_uint * nl)(*texture_counts) if texture_counts is not None else None
        ops = (C.c_ubyte * len(flat))(*[o for fr in opacities for o in fr]) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        optrs, _oinfos = self._ptr_array(rgba_frames)
        results = (C.c_uint * max(1, len(flat)))()
        r = lib.HapGpuCompositeFrames(self.handle, nf, nl, ptrs, lens, counts, ops, bg, optrs, width, height,
                                      row_bytes or width * 4, results, flags)
        return r, list(results)[: len(flat)]

    def composite_textures_placed(self, layers, layer_sizes, width, height, placements=None, opacities=None, background=None,
                                  rgba=None, row_bytes=None):
        """composite_textures for layers of sizes of their own, each placed and clipped on the width x height canvas
        (HapGpuCompositeTexturesPlaced).  layer_sizes: (width, height) per layer; placements: per layer a 6-tuple
        (srcX, srcY, width, height, dstX, dstY), all multiples of 4 -- the rectangle of the layer's picture and where its
        top-left texel lands on the canvas (None: every layer whole at (0, 0)).  A canvas texel a rectangle does not
        cover keeps what it has; what falls outside the canvas is clipped.
        Returns (result, bytes | None), or (result, None) into `rgba`."""
        n = len(layers)
        if len(layer_sizes) != n:
            raise ValueError("one size per layer")
        infos = [_addr_len(t) for t, _f, _a in layers]
        ainfos = [_addr_len(a) for _t, _f, a in layers]
        ptrs = (C.c_void_p * n)(*[i[0] for i in infos])
        lens = (C.c_ulong * n)(*[i[1] for i in infos])
        fmts = (C.c_uint * n)(*[f for _t, f, _a in layers])
        aptrs = (C.c_void_p * n)(*[i[0] for i in ainfos])
        alens = (C.c_ulong * n)(*[i[1] for i in ainfos])
        lws = (C.c_uint * n)(*[w for w, _h in layer_sizes])
        lhs = (C.c_uint * n)(*[h for _w, h in layer_sizes])
        places = _placement_array(placements, n)
        ops = (C.c_ubyte * n)(*opacities) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        row_bytes = row_bytes or width * 4
        own = rgba is None
        if own:
            rgba = (C.c_ubyte * (row_bytes * height + 16))()
            base = C.addressof(rgba)
            oa = base + (-base) % 16
        else:
            oa, _on, _k = _addr_len(rgba)
        r = lib.HapGpuCompositeTexturesPlaced(self.handle, n, ptrs, lens, fmts, aptrs, alens, lws, lhs, places, ops, bg, width,
                                              height, oa, row_bytes)
        if own:
            return r, (C.string_at(oa, row_bytes * height) if r == 0 else None)
        return r, None

    def composite_frames_placed(self, frames, frame_bytes, texture_counts, layer_sizes, rgba_frames, width, height,
                                placements=None, opacities=None, background=None, row_bytes=None, flags=0):
        """composite_frames for layers of sizes of their own, each placed and clipped on the width x height canvas
        (HapGpuCompositeFramesPlaced).  layer_sizes: (width, height) per layer, the same in every output frame;
        placements: a list per output frame of a 6-tuple (srcX, srcY, width, height, dstX, dstY) per layer (None: every
        layer whole at (0, 0)).  The definition is composite_textures_placed's with decode_frames_rgba's bytes.
        Returns (result, results[]): one entry per output frame and layer, entry f * layers + l."""
        nf = len(frames)
        nl = len(frames[0]) if nf else len(layer_sizes)
        if len(rgba_frames) != nf:
            raise ValueError("one picture per output frame")
        if any(len(fr) != nl for fr in frames):
            raise ValueError("every output frame has the same number of layers")
        if len(layer_sizes) != nl:
            raise ValueError("one size per layer")
        if placements is not None and (len(placements) != nf or any(len(fr) != nl for fr in placements)):
            raise ValueError("one placement per output frame and layer")
        flat = [b for fr in frames for b in fr]
        ptrs, infos = self._ptr_array(flat)
        given = [None] * len(flat) if frame_bytes is None else [b for fr in frame_bytes for b in fr]
        lens = (C.c_ulong * len(flat))(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(given)])
        counts = (C.c_uint * nl)(*texture_counts) if texture_counts is not None else None
        lws = (C.c_uint * max(1, nl))(*[w for w, _h in layer_sizes])
        lhs = (C.c_uint * max(1, nl))(*[h for _w, h in layer_sizes])
        places = _placement_array(None if placements is None else [p for fr in placements for p in fr], len(flat))
        ops = (C.c_ubyte * len(flat))(*[o for fr in opacities for o in fr]) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        optrs, _oinfos = self._ptr_array(rgba_frames)
        results = (C.c_uint * max(1, len(flat)))()
        r = lib.HapGpuCompositeFramesPlaced(self.handle, nf, nl, ptrs, lens, counts, lws, lhs, places, ops, bg, optrs, width,
                                            height, row_bytes or width * 4, results, flags)
        return r, list(results)[: len(flat)]

    def composite_textures_encoded(self, layers, layer_sizes, width, height, output_formats, placements=None, opacities=None,
                                   background=None, outputs=None):
        """composite_textures_placed with the canvas going out as textures of output_formats instead of a picture: as
        compress_rgba would make them of composite_textures_placed's picture, without that picture
        (HapGpuCompositeTexturesEncoded).  The canvas bytes are encoded as they are, premultiplied.
        Returns (result, [bytes] | None), or (result, [bytes used]) into `outputs`."""
        n = len(layers)
        if len(layer_sizes) != n:
            raise ValueError("one size per layer")
        infos = [_addr_len(t) for t, _f, _a in layers]
        ainfos = [_addr_len(a) for _t, _f, a in layers]
        ptrs = (C.c_void_p * n)(*[i[0] for i in infos])
        lens = (C.c_ulong * n)(*[i[1] for i in infos])
        fmts = (C.c_uint * n)(*[f for _t, f, _a in layers])
        aptrs = (C.c_void_p * n)(*[i[0] for i in ainfos])
        alens = (C.c_ulong * n)(*[i[1] for i in ainfos])
        lws = (C.c_uint * n)(*[w for w, _h in layer_sizes])
        lhs = (C.c_uint * n)(*[h for _w, h in layer_sizes])
        places = _placement_array(placements, n)
        ops = (C.c_ubyte * n)(*opacities) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        count = len(output_formats)
        own = outputs is None
        if own:
            blocks = (width // 4) * (height // 4)
            outputs = [(C.c_ubyte * max(1, blocks * (8 if f in (HapTextureFormat.RGB_DXT1, HapTextureFormat.A_RGTC1) else 16)))()
                       for f in output_formats]
        if len(outputs) != count:
            raise ValueError("one output per format")
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * max(1, count))(*[i[1] for i in oinfos])
        used = (C.c_ulong * max(1, count))()
        r = lib.HapGpuCompositeTexturesEncoded(self.handle, n, ptrs, lens, fmts, aptrs, alens, lws, lhs, places, ops, bg, width,
                                               height, count, (C.c_uint * max(1, count))(*output_formats), optrs, olens, used)
        if own:
            return r, ([C.string_at(o, used[i]) for i, o in enumerate(outputs)] if r == 0 else None)
        return r, list(used)[:count]

    def composite_frames_encoded(self, frames, frame_bytes, texture_counts, layer_sizes, width, height, formats, compressors,
                                 chunk_counts, outputs, placements=None, opacities=None, background=None, decode_flags=0,
                                 encode_flags=0):
        """composite_frames_placed whose canvases go on to the encoder: one Hap frame of `formats` per output frame, byte
        for byte what encode_frames_rgba makes of composite_frames_placed's pictures, without those pictures
        (HapGpuCompositeFramesEncoded).  frames, frame_bytes, texture_counts, layer_sizes, placements, opacities and
        background as for composite_frames_placed; formats, compressors, chunk_counts and outputs as for
        transcode_frames.  Returns (result, used[], results[], layer_results[]): results has an entry per output frame,
        layer_results one per output frame and layer, entry f * layers + l."""
        nf, count = len(frames), len(formats)
        nl = len(frames[0]) if nf else len(layer_sizes)
        if len(outputs) != nf:
            raise ValueError("one output per output frame")
        if any(len(fr) != nl for fr in frames):
            raise ValueError("every output frame has the same number of layers")
        if len(layer_sizes) != nl:
            raise ValueError("one size per layer")
        if placements is not None and (len(placements) != nf or any(len(fr) != nl for fr in placements)):
            raise ValueError("one placement per output frame and layer")
        flat = [b for fr in frames for b in fr]
        ptrs, infos = self._ptr_array(flat)
        given = [None] * len(flat) if frame_bytes is None else [b for fr in frame_bytes for b in fr]
        lens = (C.c_ulong * len(flat))(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(given)])
        counts = (C.c_uint * nl)(*texture_counts) if texture_counts is not None else None
        lws = (C.c_uint * max(1, nl))(*[w for w, _h in layer_sizes])
        lhs = (C.c_uint * max(1, nl))(*[h for _w, h in layer_sizes])
        places = _placement_array(None if placements is None else [p for fr in placements for p in fr], len(flat))
        ops = (C.c_ubyte * len(flat))(*[o for fr in opacities for o in fr]) if opacities is not None else None
        bg = (C.c_ubyte * 4)(*background) if background is not None else None
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * max(1, nf))(*[i[1] for i in oinfos])
        used = (C.c_ulong * max(1, nf))()
        results = (C.c_uint * max(1, nf))()
        layer_results = (C.c_uint * max(1, len(flat)))()
        r = lib.HapGpuCompositeFramesEncoded(self.handle, nf, nl, ptrs, lens, counts, lws, lhs, places, ops, bg, width, height,
                                             count, (C.c_uint * max(1, count))(*formats),
                                             (C.c_uint * max(1, count))(*compressors),
                                             (C.c_uint * max(1, count))(*chunk_counts), optrs, olens, used, layer_results,
                                             results, decode_flags, encode_flags)
        return r, list(used)[:nf], list(results)[:nf], list(layer_results)[: len(flat)]

    def measure_frames(self, frames, frame_bytes, texture_count, pictures, width, height, row_bytes=None, flags=0):
        """Frames against their RGBA8 reference pictures in device memory (tensors or addresses; None: no picture for that
        frame) in one call, without decoded pictures: per frame and channel the exact sums of (d - p)^2 and |d - p|, d
        being decode_frames_rgba's byte (HapGpuMeasureFrames).  Returns (result, results[], errors[]): PictureError
        objects, all zero for a frame that failed."""
        nf = len(frames)
        if len(pictures) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        keep = []
        pptrs = (C.c_void_p * nf)(*[_picture_address(p, keep) for p in pictures])
        results = (C.c_uint * nf)()
        raw = (HapGpuPictureError * nf)()
        r = lib.HapGpuMeasureFrames(self.handle, nf, ptrs, lens, texture_count, pptrs, width, height,
                                    width * 4 if row_bytes is None else row_bytes, raw, results, flags)
        return r, list(results), [_picture_error(e) for e in raw]

    def decode_frames_rgba_scaled(self, frames, frame_bytes, texture_count, rgba_frames, width, height, scale_log2,
                                  row_bytes=None, flags=0):
        """Frames -> half- (scale_log2 1) or quarter-size (2) RGBA8 pictures in one call (HapGpuDecodeFramesRGBAScaled);
        width and height are the frames'.  Returns (result, results[])."""
        nf = len(frames)
        if len(rgba_frames) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, _oinfos = self._ptr_array(rgba_frames)
        results = (C.c_uint * nf)()
        shift = scale_log2 if 0 < scale_log2 < 3 else 0
        r = lib.HapGpuDecodeFramesRGBAScaled(self.handle, nf, ptrs, lens, texture_count, optrs, width, height, scale_log2,
                                             row_bytes or (width >> shift) * 4, results, flags)
        return r, list(results)

    def decompress_nv12(self, texture, texture_format, width, height, luma, chroma, scale_log2=0, matrix=YCBCR_BT709,
                        range=YCBCR_LIMITED, luma_row_bytes=None, chroma_row_bytes=None):
        """One block texture -> one NV12 video picture on the device (HapGpuDecompressNV12), of W x H =
        (width >> scale_log2) x (height >> scale_log2).  `luma`: a (H, W) torch uint8 tensor, `chroma`: a (H / 2, W) one
        or (H / 2, W / 2, 2) Cb, Cr pairs; stride(-1) must be 1 and the pitches are read from the tensors (a slice with
        longer rows is accepted), or integer addresses with luma_row_bytes / chroma_row_bytes.  Y[y][x] is the integer
        luma of decompress_rgba[_scaled]'s texel (x, y), pair [j][i] the integer chroma of the mean of its 2 x 2 texels,
        under matrix (YCBCR_BT601, YCBCR_BT709) and range (YCBCR_LIMITED, YCBCR_FULL); alpha is ignored.  texture_format
        RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5.  Returns the result."""
        shift = scale_log2 if 0 <= scale_log2 < 3 else 0            # (a refused scale: nothing is written)
        ya, luma_row_bytes, _k1 = _video_planes(luma, True, height >> shift, width >> shift, luma_row_bytes, "luma")
        ca, chroma_row_bytes, _k2 = _video_planes(chroma, True, (height >> shift) // 2, width >> shift, chroma_row_bytes,
                                                  "chroma")
        ta, tn, _k = _addr_len(texture)
        return lib.HapGpuDecompressNV12(self.handle, ta, tn, texture_format, width, height, scale_log2, matrix, range,
                                        ya[0], luma_row_bytes, ca[0], chroma_row_bytes)

    def decode_frames_nv12(self, frames, frame_bytes, texture_count, luma_planes, chroma_planes, width, height,
                           scale_log2=0, matrix=YCBCR_BT709, range=YCBCR_LIMITED, luma_row_bytes=None,
                           chroma_row_bytes=None, flags=0):
        """Frames -> NV12 video pictures on the device in one call, without RGBA8 pictures in between
        (HapGpuDecodeFramesNV12); width and height are the frames', the pictures W x H = (width >> scale_log2) x
        (height >> scale_log2).  luma_planes / chroma_planes: one (N, H, W) / (N, H / 2, W) torch uint8 tensor each, or
        lists of N planes as decompress_nv12 takes them that share their pitch (None: no plane for that frame; integer
        addresses with luma_row_bytes / chroma_row_bytes).  The samples are decompress_nv12's of
        decode_frames_rgba[_scaled]'s pictures.  Returns (result, results[])."""
        nf = len(frames)
        shift = scale_log2 if 0 <= scale_log2 < 3 else 0
        ya, luma_row_bytes, _ky, ca, chroma_row_bytes, _kc = _video_frames(
            luma_planes, chroma_planes, width >> shift, height >> shift, luma_row_bytes, chroma_row_bytes, nf)
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        yptrs, cptrs = (C.c_void_p * nf)(*ya), (C.c_void_p * nf)(*ca)
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesNV12(self.handle, nf, ptrs, lens, texture_count, yptrs, luma_row_bytes, cptrs,
                                       chroma_row_bytes, matrix, range, width, height, scale_log2, results, flags)
        return r, list(results)

    def decode_frames_planes(self, frames, frame_bytes, texture_count, out, width, height, scale_log2=0, scale=None,
                             bias=None, flags=0):
        """Frames -> normalised planar tensors in one call, without RGBA8 pictures in between (HapGpuDecodeFramesPlanes).
        `out`: one (N, C, height >> scale_log2, width >> scale_log2) torch tensor on the device or a list of N
        (C, H, W) ones that share their strides (None: no tensor for that frame), float16, bfloat16 or float32, C 3 or 4;
        channels, element, planeBytes and rowBytes are read from it, stride(-1) must be 1.  element = float32(byte) *
        scale[c] + bias[c] (two roundings), the byte being decode_frames_rgba[_scaled]'s; scale defaults to 1/255 per
        channel, bias to 0.  Returns (result, results[])."""
        nf = len(frames)
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, False, width, height, scale_log2)
        if len(tensors) != nf:
            raise ValueError("one tensor per frame")
        sc, bi = _plane_constants(scale, bias, channels)
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs = (C.c_void_p * nf)(*[None if t is None else t.data_ptr() for t in tensors])
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesPlanes(self.handle, nf, ptrs, lens, texture_count, optrs, width, height, scale_log2,
                                         channels, element, plane_bytes, row_bytes, sc, bi, results, flags)
        return r, list(results)

    def decode_frames_planes_region(self, frames, frame_bytes, texture_count, out, width, height, origins, region_size,
                                    scale_log2=0, scale=None, bias=None, flags=0):
        """Frames -> normalised planar tensors of a crop per frame in one call (HapGpuDecodeFramesPlanesRegion): frame f's
        tensor is, bit for bit, the crop of decode_frames_planes' at origins[f] = (x, y), of region_size = (w, h) texels
        of the frames' width x height, all multiples of 4.  `out`: as for decode_frames_planes, but of the rectangle's
        scaled size, (N, C, h >> scale_log2, w >> scale_log2); scale and bias likewise.  Pieces of a frame that hold none
        of its rectangle's blocks stay undecoded (skipped_texture_bytes).  Returns (result, results[])."""
        nf = len(frames)
        w, h = region_size
        origins = [tuple(o) for o in origins]
        if len(origins) != nf or any(len(o) != 2 for o in origins):
            raise ValueError("one origin per frame")
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, False, w, h, scale_log2)
        if len(tensors) != nf:
            raise ValueError("one tensor per frame")
        sc, bi = _plane_constants(scale, bias, channels)
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs = (C.c_void_p * nf)(*[None if t is None else t.data_ptr() for t in tensors])
        xs = (C.c_uint * nf)(*[o[0] for o in origins])
        ys = (C.c_uint * nf)(*[o[1] for o in origins])
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesPlanesRegion(self.handle, nf, ptrs, lens, texture_count, optrs, width, height, xs, ys,
                                               w, h, scale_log2, channels, element, plane_bytes, row_bytes, sc, bi,
                                               results, flags)
        return r, list(results)

    def decode_frames_planes_resized(self, frames, frame_bytes, texture_count, out, width, height, crops, out_size,
                                     scale_log2=0, scale=None, bias=None, flags=0):
        """Frames -> normalised planar tensors of a resized crop per frame in one call (HapGpuDecodeFramesPlanesResized):
        crops[f] = (x, y, w, h), at any texel position and size of frame f's (width >> scale_log2) x
        (height >> scale_log2) picture, comes out as out_size = (out_w, out_h) elements by the call's integer bilinear
        filter; w <= 4 * out_w and h <= 4 * out_h.  `out`: as for decode_frames_planes, but (N, C, out_h, out_w); scale and
        bias likewise.  Pieces of a frame that hold none of the blocks under its crop stay undecoded
        (skipped_texture_bytes).  Returns (result, results[])."""
        nf = len(frames)
        out_w, out_h = out_size
        crops = [tuple(c) for c in crops]
        if len(crops) != nf or any(len(c) != 4 for c in crops):
            raise ValueError("one crop (x, y, w, h) per frame")
        tensors, channels, element, plane_bytes, row_bytes = _plane_tensors(out, False, out_w, out_h, 0)
        if len(tensors) != nf:
            raise ValueError("one tensor per frame")
        sc, bi = _plane_constants(scale, bias, channels)
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs = (C.c_void_p * nf)(*[None if t is None else t.data_ptr() for t in tensors])
        xs, ys, ws, hs = [(C.c_uint * nf)(*[c[k] for c in crops]) for k in range(4)]
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesPlanesResized(self.handle, nf, ptrs, lens, texture_count, optrs, width, height, scale_log2,
                                                xs, ys, ws, hs, out_w, out_h, channels, element, plane_bytes, row_bytes, sc,
                                                bi, results, flags)
        return r, list(results)

    def transcode_texture(self, texture, texture_format, width, height, scale_log2, output_formats, alpha=None,
                          outputs=None):
        """Texture (+ optional RGTC1 alpha plane) -> textures of output_formats at (width >> scale_log2) x
        (height >> scale_log2), as compress_rgba would make them of decompress_rgba[_scaled]'s picture, without that
        picture (HapGpuTranscodeTexture).  Returns (result, [bytes] | None), or (result, [bytes used]) into `outputs`."""
        ta, tn, _k = _addr_len(texture)
        aa, an, _k2 = _addr_len(alpha) if alpha is not None else (None, 0, None)
        count = len(output_formats)
        own = outputs is None
        if own:
            shift = scale_log2 if 0 <= scale_log2 < 3 else 0
            blocks = ((width >> shift) // 4) * ((height >> shift) // 4)
            outputs = [(C.c_ubyte * max(1, blocks * (8 if f in (HapTextureFormat.RGB_DXT1, HapTextureFormat.A_RGTC1) else 16)))()
                       for f in output_formats]
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * max(1, count))(*[i[1] for i in oinfos])
        used = (C.c_ulong * max(1, count))()
        r = lib.HapGpuTranscodeTexture(self.handle, ta, tn, texture_format, aa, an, width, height, scale_log2, count,
                                       (C.c_uint * max(1, count))(*output_formats), optrs, olens, used)
        if own:
            return r, ([C.string_at(o, used[i]) for i, o in enumerate(outputs)] if r == 0 else None)
        return r, list(used)[:count]

    def transcode_frames(self, frames, frame_bytes, source_texture_count, width, height, scale_log2, formats, compressors,
                         chunk_counts, outputs, decode_flags=0, encode_flags=0):
        """Frames -> frames of the texture formats `formats` at (width >> scale_log2) x (height >> scale_log2) in one call,
        without a picture in between (HapGpuTranscodeFrames); width and height are the source frames'.  Returns
        (result, used[], results[])."""
        nf, count = len(frames), len(formats)
        if len(outputs) != nf:
            raise ValueError("one output per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
        used = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuTranscodeFrames(self.handle, nf, ptrs, lens, source_texture_count, width, height, scale_log2, count,
                                      (C.c_uint * max(1, count))(*formats), (C.c_uint * max(1, count))(*compressors),
                                      (C.c_uint * max(1, count))(*chunk_counts), optrs, olens, used, results,
                                      decode_flags, encode_flags)
        return r, list(used), list(results)

    def decode_frames_rgba_region(self, frames, frame_bytes, texture_count, rgba_frames, width, height, region,
                                  row_bytes=None, flags=0):
        """Frames -> RGBA8 pictures of region = (x, y, w, h), a block-aligned rectangle of every frame, in one call
        (HapGpuDecodeFramesRGBARegion); width and height are the frames'.  Returns (result, results[])."""
        x, y, w, h = region
        nf = len(frames)
        if len(rgba_frames) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, _oinfos = self._ptr_array(rgba_frames)
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesRGBARegion(self.handle, nf, ptrs, lens, texture_count, optrs, width, height, x, y, w, h,
                                             w * 4 if row_bytes is None else row_bytes, results, flags)
        return r, list(results)

    def decode_frames_rgba_half(self, frames, frame_bytes, pictures, width, height, row_bytes=None, flags=0):
        """Hap HDR frames -> RGBA16F pictures in one call (HapGpuDecodeFramesRGBAHalf).  Returns (result, results[])."""
        nf = len(frames)
        if len(pictures) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, _oinfos = self._ptr_array(pictures)
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesRGBAHalf(self.handle, nf, ptrs, lens, optrs, width, height, row_bytes or width * 8,
                                           results, flags)
        return r, list(results)

    def decode_frames_alpha(self, frames, frame_bytes, pictures, width, height, row_bytes=None, flags=0):
        """Hap Alpha-Only frames -> A8 pictures in one call (HapGpuDecodeFramesAlpha).  Returns (result, results[])."""
        nf = len(frames)
        if len(pictures) != nf:
            raise ValueError("one picture per frame")
        ptrs, infos = self._ptr_array(frames)
        lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
        optrs, _oinfos = self._ptr_array(pictures)
        results = (C.c_uint * nf)()
        r = lib.HapGpuDecodeFramesAlpha(self.handle, nf, ptrs, lens, optrs, width, height, row_bytes or width, results, flags)
        return r, list(results)

    def decode_sequence(self, reader, first, count, index, outputs, batch=0):
        """Disk -> pinned double buffer -> GPU (HapGpuDecodeSequence). Returns (result, used[], formats[], results[])."""
        optrs, oinfos = self._ptr_array(outputs)
        olens = (C.c_ulong * count)(*[i[1] for i in oinfos])
        used = (C.c_ulong * count)()
        fmts = (C.c_uint * count)()
        results = (C.c_uint * count)()
        r = lib.HapGpuDecodeSequence(self.handle, reader.handle, first, count, index, batch, optrs, olens, used, fmts, results)
        return r, list(used), list(fmts), list(results)

    def join_chunk_groups(self, group_frames, group_bytes, output):
        """HapGpuJoinChunkGroupsDevice: group frames and output in device memory. Returns (result, used)."""
        n = len(group_frames)
        ptrs, _infos = self._ptr_array(group_frames)
        oaddr, olen, _keep = _addr_len(output)
        used = C.c_ulong(0)
        r = lib.HapGpuJoinChunkGroupsDevice(self.handle, n, ptrs, (C.c_ulong * max(1, n))(*group_bytes), oaddr, olen, C.byref(used))
        return r, used.value

    def encode_sequence(self, writer, rgba_frames, width, height, row_bytes, formats, compressors, chunk_counts,
                        flags=0, batch=0):
        """RGBA pictures -> GPU -> pinned double buffer -> file (HapGpuEncodeSequence). Returns (result, frame bytes[], results[])."""
        nf, count = len(rgba_frames), len(formats)
        ptrs, _infos = self._ptr_array(rgba_frames)
        sizes = (C.c_ulong * nf)()
        results = (C.c_uint * nf)()
        r = lib.HapGpuEncodeSequence(self.handle, writer.handle, nf, ptrs, width, height, row_bytes, count,
                                     (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors),
                                     (C.c_uint * count)(*chunk_counts), flags, batch, sizes, results)
        return r, list(sizes), list(results)

    def set_profiling(self, on):
        return lib.HapGpuSetProfiling(self.handle, 1 if on else 0)

    def collect_profile(self):
        n = len(KERNEL_CLASSES)
        launches = (C.c_ulong * n)()
        ms = (C.c_double * n)()
        lib.HapGpuCollectProfileN(self.handle, n, launches, ms)
        return {k: (launches[i], ms[i]) for i, k in enumerate(KERNEL_CLASSES)}

    def timer_start(self):
        return lib.HapGpuTimerStart(self.handle)

    def timer_stop(self):
        ms = C.c_double(0)
        lib.HapGpuTimerStop(self.handle, C.byref(ms))
        return ms.value


def _handles(contexts):
    return (C.c_void_p * len(contexts))(*[c.handle for c in contexts])


def encode_frames_rgba_on_devices(contexts, rgba_frames, width, height, row_bytes, formats, compressors, chunk_counts, outputs, flags=0):
    """HapGpuEncodeFramesRGBAOnDevices: frame f -> contexts[f mod N], one host thread per context, no collective."""
    nf, count = len(rgba_frames), len(formats)
    ptrs, _infos = contexts[0]._ptr_array(rgba_frames)
    optrs, oinfos = contexts[0]._ptr_array(outputs)
    olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
    used = (C.c_ulong * nf)()
    results = (C.c_uint * nf)()
    r = lib.HapGpuEncodeFramesRGBAOnDevices(_handles(contexts), len(contexts), nf, ptrs, width, height, row_bytes, count,
                                            (C.c_uint * count)(*formats), (C.c_uint * count)(*compressors),
                                            (C.c_uint * count)(*chunk_counts), optrs, olens, used, results, flags)
    return r, list(used), list(results)


def decode_frames_on_devices(contexts, frames, frame_bytes, index, outputs, flags=0):
    """HapGpuDecodeFramesOnDevices: frame f -> contexts[f mod N]."""
    nf = len(frames)
    ptrs, infos = contexts[0]._ptr_array(frames)
    lens = (C.c_ulong * nf)(*[fb if fb is not None else infos[i][1] for i, fb in enumerate(frame_bytes)])
    optrs, oinfos = contexts[0]._ptr_array(outputs)
    olens = (C.c_ulong * nf)(*[i[1] for i in oinfos])
    used = (C.c_ulong * nf)()
    fmts = (C.c_uint * nf)()
    results = (C.c_uint * nf)()
    r = lib.HapGpuDecodeFramesOnDevices(_handles(contexts), len(contexts), nf, ptrs, lens, index, optrs, olens, used, fmts, results, flags)
    return r, list(used), list(fmts), list(results)


def fine_chunk_count(texture_bytes, texture_format):
    """HapGpuFineChunkCount: the chunk count ENCODE_FINE_CHUNKS gives a texture (size buffers with it)."""
    return int(lib.HapGpuFineChunkCount(texture_bytes, texture_format))

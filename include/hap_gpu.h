/*
 * hap_gpu.h -- device-resident, batched and RGBA entry points of hap_amd.
 *
 * hap.h (the reference API) takes one frame of already block-compressed
 * texture bytes at a time and has no RGBA input (reference hap.h:82-104).
 * The functions here cover what a GPU pipeline needs on top of that, without
 * touching hap.h:
 *
 *   - RGBA -> DXT1 / DXT5 / scaled YCoCg-DXT5 / RGTC1 block compression
 *     (the "external squish/DXT encoder" stage that reference clients run
 *     before HapEncode; absent from the reference tree),
 *   - whole batches of frames per call, all work enqueued on one HIP stream
 *     with a single host synchronisation at the end,
 *   - explicit contexts (device, stream, scratch) instead of the implicit
 *     per-process context hap.h uses.
 *
 * Plain C ABI: no HIP or C++ types appear in any signature.  Every pointer
 * argument documented as "host or device" is classified at run time
 * (hipPointerGetAttributes); device pointers are used in place, host pointers
 * are staged through pinned memory.
 *
 * Frames produced here are ordinary Hap frames: the reference decoder
 * (hap.c:993-1040) decodes them byte-identically.  With
 * HAPGPU_ENCODE_FRAGMENT_INDEX the Decode Instructions Container additionally
 * carries a private section (type 0x46) listing the compressed size of every
 * independently compressed Snappy fragment; decoders that do not know it skip
 * it (reference hap.c:701-703, HapVideoDRAFT.md:34), hap_amd's decoder uses it
 * to decode one chunk with many wavefronts.  The table also records the
 * granularity (1, 2 or 4 bytes) that every element of the streams honours.
 * The flag is off unless asked for -- also for plain hap.h HapEncode, where the
 * environment variable HAP_AMD_FRAGMENT_INDEX=1 stands in for it: whether every
 * OTHER parser of a frame skips unknown sections is not something this library
 * can know ("The private section").  Frames written without it
 * still consist of independent 8 KiB Snappy fragments; hap_amd's decoder finds
 * them with a scan (an element boundary at every 8 KiB of a chunk's output) and
 * decodes them one wavefront per fragment -- about a fifth of the speed the
 * table gives.
 *
 * Section 0x46, version 1:  [1][log2 F][granularity log2][match window / 256 B][LE32 compressed size x fragments]
 *               version 4:  [4][13][granularity log2 | fields per block << 4][window][LE32 size x fragments]
 *                           [196-byte group table x fragments]
 * Version 1 promises, of every fragment: it is Snappy elements of any form (literals with up to four length bytes,
 * copy-1, copy-2, copy-4) that make exactly F bytes (the last fragment of a chunk: the rest); no copy reaches before
 * the fragment's first byte; every length and every copy offset is a multiple of the granularity; and, where the
 * window byte is 1..12 and F is 8 KiB, no copy offset exceeds 3072.  The entries of a chunk add up to the chunk less
 * its length prefix.
 * Version 4 ("field streams": block textures, 8 KiB fragments) adds, per fragment, a table of 64 groups of its
 * elements -- the elements in stream order, ceil(N / 64) to a group, the last groups shorter or empty: 24 bits per
 * group, little endian, the group's compressed bytes | the bytes it produces << 12; then N (LE16) and two zero bytes --
 * and promises that no element crosses a 128-byte half-tile of output,
 * that every element starts and ends on a block field boundary (2 + 6 + 4 + 4, 4 + 4, 2 + 6, or -- layout 8, opaque
 * 16-byte blocks -- 4 + 4 + 4 + 4 bytes) and that every
 * copy offset is a whole number of blocks: the decoder's 64 lanes then each walk one group -- the same number of
 * elements, from a known input position to a known output position -- and produce one block per lane.  Every promise
 * is checked while decoding; a frame whose table lies is decoded again without it.  (Earlier builds wrote version 2,
 * one size byte per half-tile -- ignored: such frames decode like any other encoder's -- and version 3, 96-byte group
 * tables without the groups' output bytes: its fragment sizes are still used, one wavefront per fragment.)
 */
#ifndef HAP_AMD_HAP_GPU_H
#define HAP_AMD_HAP_GPU_H

#include "hap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct HapGpuContext HapGpuContext;

/* Encode flags */
#define HAPGPU_ENCODE_FRAGMENT_INDEX 0x1u   /* emit the private fragment-size section (type 0x46): for frames that only
                                               this library or hap.c-based readers will parse */
#define HAPGPU_ENCODE_COARSE_MATCHES 0x2u   /* size for speed, for the formats without a field layout of their own: BC7 /
                                               BC6H textures (opaque 16-byte blocks) go through the block kernels as four
                                               dwords per block, copy distances in whole blocks (table layout 8): about
                                               3.5x the encode and 3.8x the decode rate of the default position-per-lane
                                               streams for 0.41 instead of 0.38 of the texture size (8K, r04).  Other
                                               formats: Snappy elements on 32-bit boundaries (DXT1's are anyway; for
                                               DXT5 / YCoCg-DXT5 / RGTC1 the default field streams are both smaller
                                               and faster) */

#define HAPGPU_ENCODE_SMALLER_FILES 0x4u    /* smaller frames, slower: Snappy fragments of 64 KiB (matches up to 64 KiB back,
                                               as in libsnappy's blocks) with elements at any 16-bit position, and no
                                               private section.  8K YCoCg-DXT5: 0.360 of the texture size against 0.395
                                               (libsnappy: 0.336), compressing at a fifth of the default rate; such frames
                                               decode like another encoder's (block scan, about 300 GB/s of texture) */

#define HAPGPU_ENCODE_FINE_CHUNKS 0x8u      /* one second-stage chunk per Snappy fragment: the chunk counts of the call are
                                               replaced by HapGpuFineChunkCount() -- 8 KiB of texture per chunk where the
                                               texture divides that way (8K Hap Q: 4050 chunks).  The chunk tables every Hap
                                               parser reads (hap.c:265-300; 5 bytes per chunk) then list every independently
                                               compressed piece: nothing private in the frame, no scan when decoding.
                                               Size the output buffers with HapMaxEncodedLength() for THAT chunk count.
                                               8K Hap Q: +20 KB per frame (the private table: +810 KB); decoded one
                                               wavefront per chunk by the generic kernel ("Frames without a
                                               table").  May be combined with HAPGPU_ENCODE_FRAGMENT_INDEX. */

#define HAPGPU_ENCODE_BPTC_BLOCKS 0x10u     /* the calls that start from RGBA pictures (HapGpuCompressRGBAFlags,
                                               HapGpuEncodeFramesRGBA and its ...Begin / ...OnDevices forms) accept
                                               HapTextureFormat_RGBA_BPTC_UNORM: the pictures are BC7-encoded on the GPU
                                               (Hap R; bptc_encode.hip: modes 6 and 1 for opaque blocks, 6 and 5 for
                                               blocks with alpha).  One texture per frame.  Without the flag they refuse
                                               that format with Bad_Arguments, as before; BC6H formats are refused
                                               either way: they are made from half-float pictures, by
                                               HapGpuCompressRGBAHalf and HapGpuEncodeFramesRGBAHalf.  Ignored by the
                                               calls that take finished textures. */

#define HAPGPU_ENCODE_REFINE_ENDPOINTS 0x20u /* a quality tier for Hap and Hap Alpha: better colour blocks, slower, the same
                                               sizes and layouts.  The calls that make blocks from pictures or planes
                                               (HapGpuCompressRGBAFlags; HapGpuEncodeFramesRGBA and its ...Begin and
                                               ...OnDevices forms; HapGpuEncodeFramesPlanes[Begin]; HapGpuEncodeSequence)
                                               replace the colour block of RGB_DXT1, and of the colour half of RGBA_DXT5,
                                               by the following.  px: the block's 16 RGB pixels; all numbers integers.
                                               1. Start: best = (c0, c1, idx), exactly the default block.
                                               2. err(best) = sum_i sum_c (px[i][c] - pal[idx_i][c])^2, pal the palette a
                                                  decoder builds with c0 > c1: the two expanded 5:6:5 words,
                                                  (2 p0 + p1) / 3, (p0 + 2 p1) / 3, floor.
                                               3. Two rounds, each from the current best.  w_i = {3, 0, 2, 1}[idx_i] (the
                                                  thirds of pal[0] in entry idx_i), v_i = 3 - w_i; A = sum w^2,
                                                  B = sum w v, C = sum v^2, det = A C - B^2; per channel P = sum w x,
                                                  Q = sum v x.  det == 0 (every pixel on one entry): no candidate.  Else
                                                  per channel a = clamp((2 * 3 (C P - B Q) + det) div (2 det), 0, 255) and
                                                  b the same from A Q - B P (div: floor) -- the least-squares end points
                                                  rounded to nearest; qa = quant5(a_r) << 11 | quant6(a_g) << 5 |
                                                  quant5(a_b) with the default's quantisers, qb likewise;
                                                  c0' = max(qa, qb), c1' = min(qa, qb); idx' from the default's index
                                                  selection on the new palette, 0 if c0' == c1'.  The candidate replaces
                                                  best only if err(candidate) < err(best), strictly.
                                               4. The block is best.
                                               So per block the error never grows, a block no round improves keeps the
                                               default's bytes, and the DXT5 alpha half is untouched.  RGBA_DXT5 frames
                                               of a flagged call do not go through the fused block compressor.
                                               Ignored, with the default's bytes: every other texture format, frames of
                                               two textures, the calls that take finished textures, HapGpuCompressPlanes
                                               (which has no flags) and HapGpuTranscodeFrames' encodeFlags.
                                               (tests/_refined_endpoints.py states the definition in numpy.) */

/* Decode flags */
#define HAPGPU_DECODE_IGNORE_FRAGMENT_INDEX 0x1u /* decode as a decoder unaware of section 0x46 would */
#define HAPGPU_DECODE_IGNORE_HALF_TILES 0x2u     /* use a version-4 table's fragment sizes only (the generic
                                                    fragment decoder), not its group tables: for A/B measurements */
#define HAPGPU_DECODE_NO_FIELD_GUESS 0x8u        /* frames whose chunks are each as short as one fragment (HAPGPU_ENCODE_FINE_CHUNKS)
                                                    and carry no private table: do not look for the block-per-lane decoder's
                                                    starting points (one lane per chunk walks its tags, then the chunk
                                                    decodes like a fragment with a table), decode every chunk with the
                                                    generic kernel -- what calls of fewer than 4096 such chunks do anyway.
                                                    The same for table-less frames whose chunks are many fragments long
                                                    (plain hap.h frames of this library): calls with 32768 or more 8 KiB
                                                    pieces found by the block scan run the pre-pass over the pieces */
#define HAPGPU_DECODE_GUESS_FIELDS 0x10u         /* ... do it however few the chunks / pieces are (tests) */
#define HAPGPU_DECODE_NO_BLOCK_SCAN 0x4u         /* decode other encoders' Snappy streams with one wavefront per
                                                    stream instead of looking for their 64 KiB blocks first: for A/B
                                                    measurements (environment HAP_AMD_NO_BLOCK_SCAN does the same) */
#define HAPGPU_DECODE_BPTC_PICTURES 0x20u        /* HapGpuDecodeFramesRGBA only: Hap R frames (one BC7 texture) become
                                                    pictures too.  Without it they are Bad_Arguments, as they were before
                                                    BC7 could be expanded here -- clients that send Hap R down a path of
                                                    their own on that result keep working; pass the flag to get the
                                                    pixels instead.  Ignored by the other decode calls. */

/* Creates a context on HIP device `device` (-1: the current device) with its
 * own non-blocking stream and growable scratch.  Returns a HapResult. */
unsigned int HapGpuCreate(int device, HapGpuContext **context);
void HapGpuDestroy(HapGpuContext *context);

/* The process-wide context used by the hap.h functions (created on first
 * use on the current device; HAP_AMD_DEVICE overrides). NULL if no GPU. */
HapGpuContext *HapGpuDefaultContext(void);

/* Log2 of the Snappy fragment size used by the compressor (10..16, default
 * 13 = 8 KiB).  Fragments are compressed independently of each other. */
unsigned int HapGpuSetFragmentLog2(HapGpuContext *context, unsigned int log2_bytes);

/* The chunk count HAPGPU_ENCODE_FINE_CHUNKS gives a texture: the smallest divisor of its block count (hap.c:277-300: every
 * chunk count must be one) that is at least bytes / 8 KiB rounded up -- chunks of at most 8 KiB, one Snappy fragment each;
 * where the block count has no divisor up to four times that number, the largest one below it (chunks of two fragments
 * and more: such frames decode like plain ones).  0 for arguments HapEncode would refuse.  Needs no GPU. */
unsigned int HapGpuFineChunkCount(unsigned long textureBytes, unsigned int textureFormat);

/* Blocks until everything enqueued on the context's stream has finished. */
unsigned int HapGpuSynchronize(HapGpuContext *context);

/* Number of frames this context has decoded a second time because their fragment table (section 0x46) did not
 * describe their streams, or because a stream split into 64 KiB blocks by the block scan turned out to copy across a
 * block start: table and scan are only ever hints, results are the same either way.  For tests and tools. */
unsigned long HapGpuTableFallbackCount(HapGpuContext *context);

/* Number of frames this context has encoded a second time: the block compressor writes a frame's compressed fragments
 * straight to their final places on the assumption that every chunk shrinks; a frame with a chunk that did not (stored
 * uncompressed, reference hap.c:460-466) is encoded again with the fragments gathered afterwards.  Same bytes either
 * way.  For tests and tools. */
unsigned long HapGpuPlacementRetryCount(HapGpuContext *context);

/* ... and how many of those were retried because a wavefront waited longer than its bound (about two milliseconds)
 * for the sizes of the fragments in front of its own: placing relies on the workgroups of a grid starting in index
 * order, which gfx950 does but HIP does not promise.  Such a frame switches placing off for the context's next 64 encode
 * calls, which gather (r06; until r05 for the rest of its life: one late neighbour under a profiler or on a shared GPU was a
 * permanent, nearly invisible change); 0 in every run so far.  For tests and tools. */
unsigned long HapGpuPlacementTimeoutCount(HapGpuContext *context);

/* Number of 64 KiB blocks of OTHER encoders' Snappy streams (frames without this library's private table, e.g. what the
 * reference's HapEncode writes: hap.c:448-476) that this context decoded with a whole workgroup each -- sixteen wavefronts
 * resolving the block's copies by pointer jumping -- instead of one wavefront walking its elements.  Which of the two
 * decodes a block changes nothing but the time it takes.  Waits for the context's stream.  For tests and tools. */
unsigned long HapGpuResolvedBlockCount(HapGpuContext *context);

/* RGBA8 (row-major, rowBytes stride, width/height multiples of 4) -> block
 * compressed texture.  textureFormat is one of RGB_DXT1, RGBA_DXT5,
 * YCoCg_DXT5, A_RGTC1 (A_RGTC1 compresses the alpha channel; a plane that is
 * not part of an RGBA8 picture goes through HapGpuCompressAlpha).  rgba and
 * output: host or device.  *outputBytesUsed = width/4 * height/4 * 8 or 16. */
unsigned int HapGpuCompressRGBA(HapGpuContext *context,
                                const void *rgba, unsigned int width, unsigned int height,
                                unsigned long rowBytes, unsigned int textureFormat,
                                void *output, unsigned long outputBytes,
                                unsigned long *outputBytesUsed);

/* HapGpuCompressRGBA with encode flags: flags == 0 is exactly HapGpuCompressRGBA.  With HAPGPU_ENCODE_BPTC_BLOCKS it
 * also takes textureFormat RGBA_BPTC_UNORM: 16 bytes per block, a device output must be 16-byte aligned.  With
 * HAPGPU_ENCODE_REFINE_ENDPOINTS the colour blocks of RGB_DXT1 and RGBA_DXT5 have refined end points (every other format:
 * the same bytes as without).  Other bits are ignored. */
unsigned int HapGpuCompressRGBAFlags(HapGpuContext *context,
                                     const void *rgba, unsigned int width, unsigned int height,
                                     unsigned long rowBytes, unsigned int textureFormat,
                                     unsigned int flags,
                                     void *output, unsigned long outputBytes,
                                     unsigned long *outputBytesUsed);

/* Block-compressed texture -> RGBA8 (the stage a GPU's texture unit performs for the reference's
 * clients; CDNA has none).  textureFormat: RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 (converted back to
 * RGB) or RGBA_BPTC_UNORM (BC7, Hap R: all eight modes; reserved blocks give (0, 0, 0, 0));
 * alphaTexture: optional A_RGTC1 plane that supplies A (Hap Q Alpha), else NULL / 0 -- Bad_Arguments
 * with BC7.  Device textures of 16-byte blocks must be 16-byte aligned, DXT1 ones 8-byte aligned.
 * rgba must be 16-byte aligned with rowBytes a multiple of 16.  Host or device pointers.  Only the
 * picture's bytes of each row are written, host or device.  BC6H textures are Bad_Arguments here:
 * HapGpuDecompressRGBAHalf expands them.  So is a lone A_RGTC1 texture: HapGpuDecompressAlpha expands it to
 * an A8 picture. */
unsigned int HapGpuDecompressRGBA(HapGpuContext *context,
                                  const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                  const void *alphaTexture, unsigned long alphaBytes,
                                  unsigned int width, unsigned int height,
                                  void *rgba, unsigned long rowBytes);

/* The same texture -> the half- (scaleLog2 1) or quarter-size (scaleLog2 2) RGBA8 picture of
 * (width >> scaleLog2) x (height >> scaleLog2), without the full-size one in between: a thumbnail, a scrub preview, a
 * monitor output.  Every output texel is the box mean of the 2^scaleLog2 x 2^scaleLog2 texels HapGpuDecompressRGBA
 * writes there, per channel (R, G, B and A alike, colour not weighted by alpha), halves rounded up:
 * (sum + (1 << (2 * scaleLog2 - 1))) >> (2 * scaleLog2), exact, on texels that are bit for bit HapGpuDecompressRGBA's.
 * width and height are the TEXTURE's (multiples of 4, so no output texel spans two blocks); textures, formats and the
 * alpha plane as for HapGpuDecompressRGBA.  rowBytes at least (width >> scaleLog2) * 4 and, like a device picture's
 * address, a multiple of the 16 >> scaleLog2 bytes a lane stores per row: 8 at half, 4 at quarter size (the natural
 * pitch always qualifies).  Host or device pointers; only the picture's bytes of each row are written.  scaleLog2 0 or
 * above 2 is Bad_Arguments (the full-size call is HapGpuDecompressRGBA, with its own alignment rules).  Out of scope:
 * RGBA16F pictures (a float mean needs a summation order defined first) and A8 pictures -- BC6H and lone A_RGTC1
 * textures are Bad_Arguments here as there. */
unsigned int HapGpuDecompressRGBAScaled(HapGpuContext *context,
                                        const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                        const void *alphaTexture, unsigned long alphaTextureBytes,
                                        unsigned int width, unsigned int height, unsigned int scaleLog2,
                                        void *rgba, unsigned long rowBytes);

/* What the elements of a planar tensor are (HapGpuDecompressPlanes, HapGpuDecodeFramesPlanes, HapGpuCompressPlanes,
 * HapGpuEncodeFramesPlanes): 2, 2 and 4 bytes */
enum HapGpuPlaneElement { HapGpuPlaneElement_F16 = 0, HapGpuPlaneElement_BF16 = 1, HapGpuPlaneElement_F32 = 2 };

/* The same texture -> one planar float tensor in DEVICE memory, for a consumer that is a model, a filter or an analysis
 * pass: `channels` planes (3: R, G, B; 4: R, G, B, A) of (width >> scaleLog2) x (height >> scaleLog2) elements, planes
 * planeBytes apart, rows rowBytes apart, scaled and shifted per channel -- made by the block decoder itself, no RGBA8
 * picture is written or read back.
 * The definition.  Let v be the byte that HapGpuDecompressRGBA (scaleLog2 0) or HapGpuDecompressRGBAScaled (1, 2) writes
 * for a texel and channel c.  The element is
 *     t = (float)v * scale[c]     one IEEE binary32 multiply, round to nearest even
 *     r = t + bias[c]             one IEEE binary32 add, round to nearest even: NOT a fused multiply-add
 * and then r itself (F32), r rounded to nearest even to half (F16; subnormal halves are kept, not flushed) or to
 * bfloat16 (BF16): numpy's v.astype(float32) * float32(s) + float32(b), then .astype(float16).  scale and bias point to
 * `channels` finite floats each, which the call does not check.  With channels 3 alpha is not written and the alpha
 * plane, if given, is not read.
 * width and height are the TEXTURE's, multiples of 4; scaleLog2 0 to 2; textures (host or device), formats and the alpha
 * plane as for HapGpuDecompressRGBA, without BC7.  Alignment: with n = 4 >> scaleLog2 elements a lane stores per row and
 * e the element's size, rowBytes, planeBytes and the tensor's address are multiples of n * e; rowBytes is at least
 * (width >> scaleLog2) * e and planeBytes at least rowBytes * ((height >> scaleLog2) - 1) + (width >> scaleLog2) * e (a
 * slice of a larger tensor, with longer rows and planes, qualifies).  Only the elements are written, nothing between
 * rows or planes.  Bad_Arguments, and nothing written, for anything else: a NULL, host or misaligned tensor, channels
 * other than 3 or 4, an element or scaleLog2 outside the above, a NULL scale or bias.
 * Out of scope: RGBA_BPTC_UNORM (BC7), the BC6H formats and a lone A_RGTC1 as sources (Bad_Arguments), and host tensors;
 * rectangles: HapGpuDecompressPlanesRegion.  The way back, from a planar float tensor to a texture, is
 * HapGpuCompressPlanes. */
unsigned int HapGpuDecompressPlanes(HapGpuContext *context,
                                    const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                    const void *alphaTexture, unsigned long alphaTextureBytes,
                                    unsigned int width, unsigned int height, unsigned int scaleLog2,
                                    unsigned int channels, unsigned int element,
                                    void *planes, unsigned long planeBytes, unsigned long rowBytes,
                                    const float *scale, const float *bias);

/* The way back: one planar float tensor in DEVICE memory -> one block-compressed texture, for a producer that is a model,
 * a filter or a colour pass -- `channels` planes (3: R, G, B; 4: R, G, B, A) of width x height elements, planes planeBytes
 * apart, rows rowBytes apart, scaled and shifted per channel and quantised by the block encoder itself as it loads them:
 * no RGBA8 picture is written or read back.
 * The definition.  For an element of plane c at a texel, with x its value as binary32 (the conversion from half or
 * bfloat16 is exact; subnormal inputs are kept, not flushed):
 *     t = x * scale[c]      one IEEE binary32 multiply, round to nearest even
 *     r = t + bias[c]       one IEEE binary32 add, round to nearest even: NOT a fused multiply-add (two roundings, not fused)
 *     v = 0                 if not (r > 0): NaN -> 0, and so -0, everything negative and -Inf
 *         255               if r >= 255: +Inf too
 *         rint(r)           otherwise: to nearest, halves to even (0.5 -> 0, 1.5 -> 2, 254.5 -> 254)
 * numpy's r = x.astype(float32) * float32(s) + float32(b); v = where(isnan(r), 0, clip(rint(r), 0, 255)).  scale and bias
 * point to `channels` finite floats each, which the call does not check.  With channels 3, A is 255 wherever a format
 * wants alpha (what HapGpuTranscodeTexture does for a source without alpha).  The picture of a tensor is the RGBA8
 * picture of these bytes, and the texture is byte for byte what HapGpuCompressRGBA makes of that picture.  It is the
 * inverse of HapGpuDecompressPlanes: a byte decoded with scale 1/255, bias 0 and quantised with scale 255, bias 0 comes
 * back, through F16, BF16 and F32 alike.
 * textureFormat: RGB_DXT1, RGBA_DXT5, YCoCg_DXT5 or A_RGTC1 (the fourth plane, or the constant 255 with three); only the
 * planes the format looks at are read.  output is host or device, under HapGpuCompressRGBA's rules (a device output
 * aligned to its blocks; too small: Buffer_Too_Small).  width and height multiples of 4, at most 65535 block rows.
 * Alignment: with e the element's size, the tensor's address, rowBytes and planeBytes are multiples of 4 * e, what a lane
 * loads per row; rowBytes is at least width * e and planeBytes at least rowBytes * (height - 1) + width * e (a slice of a
 * larger tensor, with longer rows and planes, qualifies).  Only the elements are read.  Bad_Arguments, and nothing
 * written, for anything else: a NULL, host or misaligned tensor, channels other than 3 or 4, an element outside the
 * enum, a NULL scale or bias, another format.
 * Out of scope: RGBA_BPTC_UNORM (BC7) and the BC6H formats as destinations (HAPGPU_ENCODE_BPTC_BLOCKS has no form
 * here), a one-plane tensor as a Hap Alpha-Only source (HapGpuCompressAlpha takes A8), host tensors, and scaled or
 * rectangular sources. */
unsigned int HapGpuCompressPlanes(HapGpuContext *context,
                                  const void *planes, unsigned long planeBytes, unsigned long rowBytes,
                                  unsigned int channels, unsigned int element,
                                  const float *scale, const float *bias,
                                  unsigned int width, unsigned int height, unsigned int textureFormat,
                                  void *output, unsigned long outputBytes,
                                  unsigned long *outputBytesUsed);

/* The same texture -> the RGBA8 picture of one block-aligned rectangle of it, regionWidth x regionHeight: byte for byte
 * the crop of what HapGpuDecompressRGBA writes, from the rectangle's blocks alone (no other block of the texture or of
 * the alpha plane is read).  width and height are the TEXTURE's.  regionX, regionY, regionWidth and regionHeight are
 * multiples of 4, the last two non-zero, regionX + regionWidth <= width and regionY + regionHeight <= height: anything
 * else is Bad_Arguments and nothing is written.  rowBytes a multiple of 16 and at least regionWidth * 4, a device picture
 * 16-byte aligned; host or device pointers; only the picture's bytes of each row are written.  Textures, formats and the
 * alpha plane as for HapGpuDecompressRGBA.  Out of scope: RGBA16F and A8 pictures, and scaled rectangles. */
unsigned int HapGpuDecompressRGBARegion(HapGpuContext *context,
                                        const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                        const void *alphaTexture, unsigned long alphaTextureBytes,
                                        unsigned int width, unsigned int height,
                                        unsigned int regionX, unsigned int regionY,
                                        unsigned int regionWidth, unsigned int regionHeight,
                                        void *rgba, unsigned long rowBytes);

/* The same texture -> the planar float tensor of one block-aligned rectangle of it, in DEVICE memory: HapGpuDecompressPlanes
 * and HapGpuDecompressRGBARegion joined, the single-texture form of HapGpuDecodeFramesPlanesRegion.
 * The definition, and the only one.  With s = scaleLog2, the tensor is `channels` planes of (regionWidth >> s) x
 * (regionHeight >> s) elements, and it equals, bit for bit, rows [regionY >> s, (regionY + regionHeight) >> s) and columns
 * [regionX >> s, (regionX + regionWidth) >> s) of every plane of the tensor HapGpuDecompressPlanes writes for the same
 * texture, alpha plane, scaleLog2, channels, element, scale and bias.  A box mean never spans two blocks, so a block-aligned
 * rectangle is enough at every scale.  The two roundings -- one binary32 multiply by scale[c], then one binary32 add of
 * bias[c], not fused --, the conversion to the element (subnormal halves kept) and the handling of alpha (with channels 3
 * it is not written and the alpha plane not read) are HapGpuDecompressPlanes'.  Only the rectangle's blocks are read.
 * Geometry: width and height are the TEXTURE's; regionX, regionY, regionWidth and regionHeight are multiples of 4, the last
 * two non-zero, regionX + regionWidth <= width and regionY + regionHeight <= height.  Tensor: HapGpuDecompressPlanes' rules
 * at the rectangle's size -- device memory only; with n = 4 >> scaleLog2 and e the element's size the address, rowBytes
 * and planeBytes are multiples of n * e, rowBytes at least (regionWidth >> s) * e and planeBytes at least
 * rowBytes * ((regionHeight >> s) - 1) + (regionWidth >> s) * e; a slice of a larger tensor qualifies; nothing is written
 * between rows or planes.  Bad_Arguments, and nothing written, for anything else.
 * Out of scope: RGBA_BPTC_UNORM (BC7), the BC6H formats and a lone A_RGTC1 as sources (Bad_Arguments), host tensors, and
 * rectangles off the block grid. */
unsigned int HapGpuDecompressPlanesRegion(HapGpuContext *context,
                                          const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                          const void *alphaTexture, unsigned long alphaTextureBytes,
                                          unsigned int width, unsigned int height,
                                          unsigned int regionX, unsigned int regionY,
                                          unsigned int regionWidth, unsigned int regionHeight,
                                          unsigned int scaleLog2, unsigned int channels, unsigned int element,
                                          void *planes, unsigned long planeBytes, unsigned long rowBytes,
                                          const float *scale, const float *bias);

/* The same texture -> the planar float tensor, in DEVICE memory, of one crop of it at any texel position and size,
 * resized to outWidth x outHeight: the single-texture form of HapGpuDecodeFramesPlanesResized, which has the definition
 * -- P is here what HapGpuDecompressRGBA (scaleLog2 0) or HapGpuDecompressRGBAScaled (1, 2) writes, (cropX, cropY,
 * cropWidth, cropHeight) the crop in texels of P, and the taps, the blend, the two roundings (one binary32 multiply, one
 * binary32 add, not fused) and the limits are that call's.  Only the blocks that hold texels of the crop are read.
 * width and height are the TEXTURE's, multiples of 4; textures (host or device), formats and the alpha plane as for
 * HapGpuDecompressPlanes.  Tensor: device memory only; with e the element's size the address, rowBytes and planeBytes are
 * multiples of e, rowBytes at least outWidth * e and planeBytes at least rowBytes * (outHeight - 1) + outWidth * e; a
 * slice of a larger tensor qualifies; nothing is written between rows or planes.  Bad_Arguments, and nothing written, for
 * anything else: a crop that is empty, past an edge of P or more than 4 x the output in either axis, an output size of 0
 * or above 16384, and what HapGpuDecompressPlanes refuses.
 * Out of scope: RGBA_BPTC_UNORM (BC7), the BC6H formats and a lone A_RGTC1 as sources (Bad_Arguments), host tensors,
 * other filters, RGBA8 output. */
unsigned int HapGpuDecompressPlanesResized(HapGpuContext *context,
                                           const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                           const void *alphaTexture, unsigned long alphaTextureBytes,
                                           unsigned int width, unsigned int height, unsigned int scaleLog2,
                                           unsigned int cropX, unsigned int cropY,
                                           unsigned int cropWidth, unsigned int cropHeight,
                                           unsigned int outWidth, unsigned int outHeight,
                                           unsigned int channels, unsigned int element,
                                           void *planes, unsigned long planeBytes, unsigned long rowBytes,
                                           const float *scale, const float *bias);

/* BC6H texture (Hap HDR) -> RGBA16F: four IEEE half bit patterns per texel, 8 bytes, rows rowBytes apart.
 * textureFormat: RGB_BPTC_UNSIGNED_FLOAT or RGB_BPTC_SIGNED_FLOAT (anything else is Bad_Arguments).  RGB is
 * the BPTC definition's result bit for bit (signed textures may give -0, 0x8000, which is kept); alpha is
 * 1.0 (0x3C00); reserved modes give RGB 0.  width and height multiples of 4; rowBytes at least width * 8
 * and a multiple of 16.  Host or device pointers; a device texture and a device picture must each be
 * 16-byte aligned.  Only the picture's bytes of each row are written, host or device. */
unsigned int HapGpuDecompressRGBAHalf(HapGpuContext *context,
                                      const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                      unsigned int width, unsigned int height,
                                      void *rgbaHalf, unsigned long rowBytes);

/* RGBA16F picture -> BC6H texture (Hap HDR), the other way.  rgbaHalf: four IEEE half bit patterns per texel, 8 bytes,
 * rows rowBytes apart; alpha is ignored.  textureFormat: RGB_BPTC_UNSIGNED_FLOAT or RGB_BPTC_SIGNED_FLOAT (anything
 * else is Bad_Arguments).  Unsigned: negative values, -0 and NaN encode as 0, +Inf as the largest finite half; signed:
 * NaN as 0, +-Inf as the largest finite half of their sign.  The encoder is bc6h_encode.hip (modes 0x03, 0x07, 0x0B,
 * 0x0F of one region, 0x1E, 0x01, 0x00 of two; tests/_bc6h_encode.py defines it bit for bit).  width and height
 * multiples of 4; rowBytes at least width * 8 and a multiple of 16.  Host or device pointers; a device picture and a
 * device output must each be 16-byte aligned.  16 bytes per block. */
unsigned int HapGpuCompressRGBAHalf(HapGpuContext *context,
                                    const void *rgbaHalf, unsigned int width, unsigned int height,
                                    unsigned long rowBytes, unsigned int textureFormat,
                                    void *output, unsigned long outputBytes,
                                    unsigned long *outputBytesUsed);

/* --- alpha-only pictures (Hap Alpha-Only: mattes and masks) -----------------------------------
 * An A8 picture is one byte per texel, row-major, rows rowBytes apart.  The rules of every ...Alpha call:
 *   - width and height are multiples of 4 (height at most 262140);
 *   - rowBytes is at least width and a multiple of 4;
 *   - pointers are host or device; a device picture is 4-byte aligned, a device texture 8-byte aligned;
 *   - only the picture's own bytes of each row are written: host pictures with longer rows are written row by row,
 *     and the kernels never store between width and rowBytes.
 * A picture whose address (in device memory) and rowBytes are both 16-byte aligned is read and written 16 bytes at a
 * time by lanes that take four blocks each (alpha_plane.hip); any other by the one-block-per-lane form.  The bytes
 * are the same. */

/* A8 picture -> A_RGTC1 texture, 8 bytes a block: byte for byte the texture HapGpuCompressRGBA(..., A_RGTC1) makes
 * of an RGBA8 picture that carries the plane in its alpha channel, from a quarter of the bytes.
 * *outputBytesUsed = width/4 * height/4 * 8; a smaller output is Buffer_Too_Small. */
unsigned int HapGpuCompressAlpha(HapGpuContext *context,
                                 const void *alpha, unsigned int width, unsigned int height,
                                 unsigned long rowBytes,
                                 void *output, unsigned long outputBytes,
                                 unsigned long *outputBytesUsed);

/* A_RGTC1 texture -> A8 picture (the RGTC definition's values, bit for bit).  textureBytes below
 * width/4 * height/4 * 8 is Bad_Arguments. */
unsigned int HapGpuDecompressAlpha(HapGpuContext *context,
                                   const void *texture, unsigned long textureBytes,
                                   unsigned int width, unsigned int height,
                                   void *alpha, unsigned long rowBytes);

/* Batched HapEncode: frame f is made of `count` textures
 * inputBuffers[f*count + i] of inputBuffersBytes[i] bytes each (every frame of
 * a batch has the same geometry).  Semantics, frame layout, chunk-count
 * limiting, store-raw decisions and result codes per frame follow HapEncode.
 * outputBuffers[f] must hold HapMaxEncodedLength() bytes.
 * results[f] receives the HapResult of frame f; the function result is the
 * first non-zero of them. */
unsigned int HapGpuEncodeFrames(HapGpuContext *context, unsigned int frameCount,
                                unsigned int count,
                                const void *const *inputBuffers,
                                const unsigned long *inputBuffersBytes,
                                const unsigned int *textureFormats,
                                const unsigned int *compressors,
                                const unsigned int *chunkCounts,
                                void *const *outputBuffers,
                                const unsigned long *outputBuffersBytes,
                                unsigned long *outputBuffersBytesUsed,
                                unsigned int *results,
                                unsigned int flags);

/* Batched RGBA -> Hap frame: block-compresses every frame into `count`
 * textures of textureFormats[] (e.g. {YCoCg_DXT5} for Hap Q, {YCoCg_DXT5,
 * A_RGTC1} for Hap Q Alpha, {RGB_DXT1} for Hap, {RGBA_DXT5} for Hap Alpha,
 * {RGBA_BPTC_UNORM} for Hap R with HAPGPU_ENCODE_BPTC_BLOCKS in flags and
 * count 1) and packs them exactly as HapGpuEncodeFrames does; the
 * intermediate textures never leave HBM.  rgbaFrames[f]: host or device. */
unsigned int HapGpuEncodeFramesRGBA(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *rgbaFrames,
                                    unsigned int width, unsigned int height,
                                    unsigned long rowBytes,
                                    unsigned int count,
                                    const unsigned int *textureFormats,
                                    const unsigned int *compressors,
                                    const unsigned int *chunkCounts,
                                    void *const *outputBuffers,
                                    const unsigned long *outputBuffersBytes,
                                    unsigned long *outputBuffersBytesUsed,
                                    unsigned int *results,
                                    unsigned int flags);

/* The same two calls in two halves, for pipelines: ...Begin checks the arguments, enqueues every launch of the call on
 * the context's stream and returns WITHOUT waiting for the GPU; HapGpuEncodeFramesFinish waits, fills
 * outputBuffersBytesUsed[] and results[] (the two arrays must live until then; every other argument array may go
 * once Begin has returned; the buffers themselves must of course stay) and encodes again whatever the first pass
 * could not place.  Between the halves the context takes no other call (Internal_Error) -- the client meanwhile
 * decodes the previous batch on ANOTHER context, parses, reads the next pictures: the encode kernels run under it
 * and the GPU never idles between calls (bench.py's step, DESIGN.md "Pipelined step").  Begin returns errors that are
 * known at once (then nothing is pending and Finish has nothing to do); Finish returns what the one-call form
 * returns.  At most 32768 frames per Begin.  A context destroyed between the halves waits for the launches and writes
 * no results.  The reference has no counterpart: HapEncode returns when its frame is
 * written (hap.h:98-104). */
unsigned int HapGpuEncodeFramesRGBABegin(HapGpuContext *context, unsigned int frameCount,
                                         const void *const *rgbaFrames,
                                         unsigned int width, unsigned int height,
                                         unsigned long rowBytes,
                                         unsigned int count,
                                         const unsigned int *textureFormats,
                                         const unsigned int *compressors,
                                         const unsigned int *chunkCounts,
                                         void *const *outputBuffers,
                                         const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed,
                                         unsigned int *results,
                                         unsigned int flags);
unsigned int HapGpuEncodeFramesBegin(HapGpuContext *context, unsigned int frameCount,
                                     unsigned int count,
                                     const void *const *inputBuffers,
                                     const unsigned long *inputBuffersBytes,
                                     const unsigned int *textureFormats,
                                     const unsigned int *compressors,
                                     const unsigned int *chunkCounts,
                                     void *const *outputBuffers,
                                     const unsigned long *outputBuffersBytes,
                                     unsigned long *outputBuffersBytesUsed,
                                     unsigned int *results,
                                     unsigned int flags);
unsigned int HapGpuEncodeFramesFinish(HapGpuContext *context);

/* Batched RGBA16F -> Hap HDR frame: HapGpuEncodeFramesRGBA for half-float pictures (HapGpuCompressRGBAHalf's rules
 * for them; a misaligned device picture makes its frame Bad_Arguments) and one BC6H texture per frame, packed exactly
 * as HapGpuEncodeFrames packs a BC6H texture; the flags mean what they mean there.  textureFormat:
 * RGB_BPTC_UNSIGNED_FLOAT or RGB_BPTC_SIGNED_FLOAT, else Bad_Arguments.  ...Begin is the first half of the call as
 * HapGpuEncodeFramesRGBABegin is; HapGpuEncodeFramesFinish finishes it. */
unsigned int HapGpuEncodeFramesRGBAHalf(HapGpuContext *context, unsigned int frameCount,
                                        const void *const *rgbaHalfFrames,
                                        unsigned int width, unsigned int height,
                                        unsigned long rowBytes,
                                        unsigned int textureFormat,
                                        unsigned int compressor,
                                        unsigned int chunkCount,
                                        void *const *outputBuffers,
                                        const unsigned long *outputBuffersBytes,
                                        unsigned long *outputBuffersBytesUsed,
                                        unsigned int *results,
                                        unsigned int flags);
unsigned int HapGpuEncodeFramesRGBAHalfBegin(HapGpuContext *context, unsigned int frameCount,
                                             const void *const *rgbaHalfFrames,
                                             unsigned int width, unsigned int height,
                                             unsigned long rowBytes,
                                             unsigned int textureFormat,
                                             unsigned int compressor,
                                             unsigned int chunkCount,
                                             void *const *outputBuffers,
                                             const unsigned long *outputBuffersBytes,
                                             unsigned long *outputBuffersBytesUsed,
                                             unsigned int *results,
                                             unsigned int flags);

/* Batched A8 -> Hap Alpha-Only frame: HapGpuEncodeFramesRGBA for A8 pictures (the rules above; a misaligned device
 * picture makes its frame Bad_Arguments) and one A_RGTC1 texture per frame.  A frame is byte for byte the one
 * HapGpuEncodeFramesRGBA makes with the same flags and {A_RGTC1} of an RGBA8 picture that carries the plane in its
 * alpha channel; the flags mean what they mean there.  ...Begin is the first half of the call as
 * HapGpuEncodeFramesRGBABegin is; HapGpuEncodeFramesFinish finishes it. */
unsigned int HapGpuEncodeFramesAlpha(HapGpuContext *context, unsigned int frameCount,
                                     const void *const *alphaFrames,
                                     unsigned int width, unsigned int height,
                                     unsigned long rowBytes,
                                     unsigned int compressor,
                                     unsigned int chunkCount,
                                     void *const *outputBuffers,
                                     const unsigned long *outputBuffersBytes,
                                     unsigned long *outputBuffersBytesUsed,
                                     unsigned int *results,
                                     unsigned int flags);
unsigned int HapGpuEncodeFramesAlphaBegin(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *alphaFrames,
                                          unsigned int width, unsigned int height,
                                          unsigned long rowBytes,
                                          unsigned int compressor,
                                          unsigned int chunkCount,
                                          void *const *outputBuffers,
                                          const unsigned long *outputBuffersBytes,
                                          unsigned long *outputBuffersBytesUsed,
                                          unsigned int *results,
                                          unsigned int flags);

/* Batched HapDecode of texture `index` of every frame.  No callback: all
 * chunks of all frames are decoded by the GPU.  Per-frame result codes,
 * bytes used and texture formats follow HapDecode (including the hardening
 * noted in INTEGRATION.md: out-of-range chunk tables are Bad_Frame instead of
 * an out-of-bounds read).  outputBytesUsed / outputTextureFormats may be NULL. */
unsigned int HapGpuDecodeFrames(HapGpuContext *context, unsigned int frameCount,
                                const void *const *inputBuffers,
                                const unsigned long *inputBuffersBytes,
                                unsigned int index,
                                void *const *outputBuffers,
                                const unsigned long *outputBuffersBytes,
                                unsigned long *outputBuffersBytesUsed,
                                unsigned int *outputTextureFormats,
                                unsigned int *results,
                                unsigned int flags);

/* The same for textures 0 .. textureCount-1 (1 or 2) of every frame in ONE batch: the arrays outputBuffers,
 * outputBuffersBytes, outputBuffersBytesUsed, outputTextureFormats and results have frameCount * textureCount
 * entries, entry f * textureCount + t belonging to texture t of frame f (what HapDecode(..., index = t, ...) would
 * be handed for that frame, reference hap.h:132-140).  A Hap Q Alpha stream decoded this way pays the per-call
 * costs (header read-back, launches, completion) once instead of once per texture. */
unsigned int HapGpuDecodeFrameTextures(HapGpuContext *context, unsigned int frameCount,
                                       const void *const *inputBuffers,
                                       const unsigned long *inputBuffersBytes,
                                       unsigned int textureCount,
                                       void *const *outputBuffers,
                                       const unsigned long *outputBuffersBytes,
                                       unsigned long *outputBuffersBytesUsed,
                                       unsigned int *outputTextureFormats,
                                       unsigned int *results,
                                       unsigned int flags);

/* Frames in, pixels out: every frame's second stage is undone (as HapGpuDecodeFrameTextures does, in one batch) and
 * its block texture expanded to an RGBA8 picture of width x height in rgbaFrames[f] (rowBytes: a multiple of 16,
 * at least width * 4; device pictures 16-byte aligned; host or device).  textureCount 1: the frames hold one
 * DXT1 / DXT5 / scaled-YCoCg-DXT5 texture (Hap, Hap Alpha, Hap Q; YCoCg is converted back to RGB the way the
 * reference's consumers do in their shader); textureCount 2: Hap Q Alpha frames, whose RGTC1
 * plane becomes the pictures' alpha.  The block textures live in the context's scratch only (at most 4 GiB of them at a
 * time: longer batches are worked through in slices).  results[f]:
 * HapDecode's code for the frame; Bad_Arguments for a frame whose texture is of another format or geometry than the
 * call says (lone RGTC1 textures, Hap Alpha-Only, go to HapGpuDecodeFramesAlpha; BC6H ones go to
 * HapGpuDecodeFramesRGBAHalf, flag or not).
 * Hap R frames (one BC7 texture) are
 * Bad_Arguments unless flags has HAPGPU_DECODE_BPTC_PICTURES: then, with textureCount 1, they decode to pictures like
 * the others (textureCount 2 stays Bad_Arguments for them).  A batch may mix Hap, Hap Alpha, Hap Q and Hap R frames:
 * one block-decode launch per texture format present.  The reference has no counterpart: it stops at the texture
 * (hap.h:132-140) and leaves the pixels to the consumer's GPU. */
unsigned int HapGpuDecodeFramesRGBA(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *inputBuffers,
                                    const unsigned long *inputBuffersBytes,
                                    unsigned int textureCount,
                                    void *const *rgbaFrames,
                                    unsigned int width, unsigned int height, unsigned long rowBytes,
                                    unsigned int *results,
                                    unsigned int flags);

/* Frames in, the pixels of one rectangle out: HapGpuDecodeFramesRGBA for clients that show a tile of a large canvas (one
 * output of a video wall, one projector of a blend, one GPU's band).  The rectangle (regionX, regionY, regionWidth,
 * regionHeight, in texels of the FRAMES' width x height) is block-aligned: all four are multiples of 4, width and height
 * of it are non-zero, regionX + regionWidth <= width and regionY + regionHeight <= height; anything else is Bad_Arguments
 * for the whole call, every results[f] set to it and nothing written.  Pictures are regionWidth x regionHeight RGBA8,
 * host or device, rowBytes a multiple of 16 and at least regionWidth * 4, device pictures 16-byte aligned, host pictures
 * with longer rows written row by row: HapGpuDecodeFramesRGBA's rules at the rectangle's size.  Every picture is byte for
 * byte the crop of what HapGpuDecodeFramesRGBA writes for the same frame; bytes outside a picture's own rows are never
 * written.  The block decoder reads the rectangle's blocks only, and the second stage leaves undecoded every
 * independently decodable piece -- a chunk, a fragment of this library's table, a block found by the scan of a
 * table-less stream, a 64 KiB piece of an uncompressed chunk -- that holds no byte of them (HapGpuRegionNeedsBytes);
 * a rectangle that is the whole frame skips nothing.  textureCount, the formats, flags (HAPGPU_DECODE_BPTC_PICTURES
 * included), mixed batches and slicing are HapGpuDecodeFramesRGBA's.  results[f] too, with one difference: damage that
 * lies wholly inside skipped pieces is not seen (as HapDecode does not see a chunk its callback never runs); damage in
 * the container, the tables or a decoded piece gets the full call's code.  A frame of another format or geometry is
 * Bad_Arguments alone, its picture untouched.  Out of scope: RGBA16F and A8 pictures, a rectangle together with
 * scaleLog2, ...OnDevices / ...Sequence forms, rectangles off the block grid.  (Planar float tensors of a rectangle, at
 * any of the three sizes and with a rectangle per frame: HapGpuDecodeFramesPlanesRegion.) */
unsigned int HapGpuDecodeFramesRGBARegion(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *inputBuffers,
                                          const unsigned long *inputBuffersBytes,
                                          unsigned int textureCount,
                                          void *const *rgbaFrames,
                                          unsigned int width, unsigned int height,
                                          unsigned int regionX, unsigned int regionY,
                                          unsigned int regionWidth, unsigned int regionHeight,
                                          unsigned long rowBytes,
                                          unsigned int *results,
                                          unsigned int flags);

/* Which bytes of a texture a rectangle needs, without a GPU: 1 if and only if bytes [firstByte, firstByte + byteCount)
 * of a width-wide texture of blockBytes-byte blocks (8: DXT1, RGTC1; 16: the others) hold at least one byte of a block
 * of the rectangle; 0 for an empty range and for arguments the region rules refuse (Bad_Arguments above; the texture's
 * height is not known here).  The very predicate the decoder skips by.  With HapGpuGetFrameTextureChunkLayout's offsets
 * it tells a client which chunks of a frame it has to read from disk at all. */
unsigned int HapGpuRegionNeedsBytes(unsigned int width, unsigned int blockBytes,
                                    unsigned int regionX, unsigned int regionY,
                                    unsigned int regionWidth, unsigned int regionHeight,
                                    unsigned long firstByte, unsigned long byteCount);

/* Decoded bytes of all the pieces the region calls of this context left undecoded, summed over the context's life.
 * A frame counts once: one that is decoded a second time without its fragment table keeps the first pass's figure,
 * though the second pass skips whole chunks only.  Never more, per call, than the textures' bytes minus the bytes of
 * the rectangle's blocks (HapGpuDecodeFramesPlanesRegion: of the rectangles' blocks, frame by frame).  Waits for the stream: for tests and tools, like HapGpuResolvedBlockCount. */
unsigned long HapGpuSkippedTextureBytes(HapGpuContext *context);

/* Frames in, half- (scaleLog2 1) or quarter-size (scaleLog2 2) pixels out: HapGpuDecodeFramesRGBA with the pictures of
 * HapGpuDecompressRGBAScaled -- (width >> scaleLog2) x (height >> scaleLog2) RGBA8, every texel the rounded-up box mean
 * of the 2^scaleLog2 x 2^scaleLog2 texels HapGpuDecodeFramesRGBA writes there -- made by the block decoder itself: no
 * full-size picture is written or read back.  width and height are the FRAMES' geometry; rowBytes and device pictures
 * follow HapGpuDecompressRGBAScaled's rule (multiples of 8 at half, 4 at quarter size; at least
 * (width >> scaleLog2) * 4); host pictures with longer rows are written row by row.  textureCount, flags
 * (HAPGPU_DECODE_BPTC_PICTURES included), mixed batches and results[f] are HapGpuDecodeFramesRGBA's: a frame of another
 * format or geometry is Bad_Arguments alone and its picture untouched, a broken frame gets HapDecode's code.  scaleLog2
 * 0 or above 2 is Bad_Arguments for the whole call.  Out of scope: RGBA16F (Hap HDR) and A8 (Hap Alpha-Only) pictures,
 * and ...OnDevices / ...Sequence forms of this call. */
unsigned int HapGpuDecodeFramesRGBAScaled(HapGpuContext *context, unsigned int frameCount,
                                          const void *const *inputBuffers,
                                          const unsigned long *inputBuffersBytes,
                                          unsigned int textureCount,
                                          void *const *rgbaFrames,
                                          unsigned int width, unsigned int height, unsigned int scaleLog2,
                                          unsigned long rowBytes,
                                          unsigned int *results,
                                          unsigned int flags);

/* Frames in, normalised planar float tensors out: HapGpuDecodeFramesRGBA with the tensors of HapGpuDecompressPlanes in
 * place of pictures -- planeFrames[f] is frame f's tensor in DEVICE memory, `channels` planes of
 * (width >> scaleLog2) x (height >> scaleLog2) elements, planeBytes and rowBytes shared by all frames (one N x C x H x W
 * tensor: planeFrames[f] = base + f * channels * planeBytes).  The definition is HapGpuDecompressPlanes': for the byte v
 * that HapGpuDecodeFramesRGBA (scaleLog2 0) or HapGpuDecodeFramesRGBAScaled (1, 2) writes for the frame at that texel
 * and channel c, with the same textureCount and flags, one binary32 multiply by scale[c], then one binary32 add of
 * bias[c] (two roundings, not fused), then the rounding to the element.  No RGBA8 picture ever exists: per Hap Q block
 * 16 bytes are read and 96 written for three half planes, where decoding to RGBA8 and converting moves 16 + 64 + 64 + 96.
 * width and height are the FRAMES', multiples of 4; scaleLog2 0 to 2; channels 3 or 4 (with 3 alpha is not written, and a
 * Hap Q Alpha frame read with textureCount 1 is its colour texture alone); scale and bias point to `channels` floats;
 * alignment as for HapGpuDecompressPlanes.  textureCount, flags, mixed batches (one block-decode launch per texture
 * format present), slicing and results[f] are HapGpuDecodeFramesRGBA's: a broken frame gets HapDecode's code; a frame of
 * another format or geometry, or one whose tensor is NULL, in host memory or misaligned, is Bad_Arguments alone, its
 * memory untouched, and the other frames are decoded.  The function's result is the first failure.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written -- for a NULL array, a width or height that
 * is no multiple of 4, channels other than 3 or 4, an element or scaleLog2 outside the above, a rowBytes or planeBytes
 * that breaks the alignment rule or is too short.  A context between HapGpuEncodeFramesRGBABegin and
 * HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: Hap R (BC7), Hap HDR (BC6H) and Hap Alpha-Only (a lone A_RGTC1) frames -- Bad_Arguments alone, with or
 * without HAPGPU_DECODE_BPTC_PICTURES --, host tensors, ...OnDevices and ...Sequence forms of this call; rectangles:
 * HapGpuDecodeFramesPlanesRegion.  The way back, from planar float tensors to frames, is HapGpuEncodeFramesPlanes.  A crop
 * per frame at any texel position and size, every one resized to one output size: HapGpuDecodeFramesPlanesResized. */
unsigned int HapGpuDecodeFramesPlanes(HapGpuContext *context, unsigned int frameCount,
                                      const void *const *inputBuffers,
                                      const unsigned long *inputBuffersBytes,
                                      unsigned int textureCount,
                                      void *const *planeFrames,
                                      unsigned int width, unsigned int height, unsigned int scaleLog2,
                                      unsigned int channels, unsigned int element,
                                      unsigned long planeBytes, unsigned long rowBytes,
                                      const float *scale, const float *bias,
                                      unsigned int *results,
                                      unsigned int flags);

/* Frames in, normalised planar float tensors of a crop per frame out: HapGpuDecodeFramesPlanes and
 * HapGpuDecodeFramesRGBARegion joined, for an input pipeline that wants a (random, tracked, tiled) crop of every frame,
 * often at half or quarter size.  Frame f's rectangle is regionWidth x regionHeight texels at (regionXs[f], regionYs[f])
 * of the FRAMES' width x height; regionXs and regionYs have frameCount entries each; the size is shared.
 * The definition, and the only one.  With s = scaleLog2, planeFrames[f] is frame f's tensor in DEVICE memory: `channels`
 * planes of (regionWidth >> s) x (regionHeight >> s) elements, planeBytes and rowBytes shared by all frames.  It equals, bit
 * for bit, rows [regionYs[f] >> s, (regionYs[f] + regionHeight) >> s) and columns [regionXs[f] >> s,
 * (regionXs[f] + regionWidth) >> s) of every plane of the tensor HapGpuDecodeFramesPlanes writes for that frame with the
 * same textureCount, scaleLog2, channels, element, scale, bias and flags.  A box mean never spans two blocks, so a
 * block-aligned rectangle is enough at every scale.  The two roundings -- one binary32 multiply by scale[c], then one
 * binary32 add of bias[c], not fused --, the conversion to the element and the handling of alpha are that call's.
 * The block decoder reads every frame's own rectangle's blocks only, and the second stage leaves undecoded, frame by
 * frame, every independently decodable piece that holds no byte of them, as HapGpuDecodeFramesRGBARegion does for its one
 * rectangle (HapGpuRegionNeedsBytes; counted by HapGpuSkippedTextureBytes); a rectangle that is the whole frame skips
 * nothing.
 * Geometry (HapGpuDecodeFramesRGBARegion's rules): regionXs[f], regionYs[f], regionWidth and regionHeight are multiples
 * of 4, regionWidth and regionHeight non-zero, regionXs[f] + regionWidth <= width and regionYs[f] + regionHeight <= height.
 * Tensors (HapGpuDecodeFramesPlanes' rules at the rectangle's size): device memory only; with n = 4 >> scaleLog2 and e the
 * element's size the addresses, rowBytes and planeBytes are multiples of n * e, rowBytes at least (regionWidth >> s) * e
 * and planeBytes at least rowBytes * ((regionHeight >> s) - 1) + (regionWidth >> s) * e; a slice of a larger tensor
 * qualifies; nothing is written between rows or planes.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written -- for what HapGpuDecodeFramesPlanes refuses, a
 * NULL regionXs or regionYs, a regionWidth or regionHeight that is zero, off the grid or larger than the frame.  A frame
 * whose own origin puts the rectangle off the grid or past an edge is Bad_Arguments alone: its tensor is untouched,
 * nothing of it is handed to the second stage or the block decoder, and the other frames are decoded.  So is a frame of
 * another format or geometry, or one whose tensor is NULL, in host memory or misaligned.  A broken frame gets the full
 * call's code; damage wholly inside skipped pieces is not seen, as in HapGpuDecodeFramesRGBARegion.  A context between
 * HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.  Sources, textureCount, flags, mixed batches
 * (one block-decode launch per texture format present) and slicing are HapGpuDecodeFramesPlanes': Hap, Hap Alpha, Hap Q,
 * Hap Q Alpha.
 * Out of scope: Hap R (BC7), Hap HDR (BC6H) and Hap Alpha-Only (a lone A_RGTC1) frames as sources, host tensors,
 * rectangles off the block grid, rectangles of different sizes in one call, ...OnDevices and ...Sequence forms of this
 * call, and an RGBA8 "rectangle together with scaleLog2" call.  (Rectangles of a size of their own per frame, at any texel
 * position, resized to one output size: HapGpuDecodeFramesPlanesResized.) */
unsigned int HapGpuDecodeFramesPlanesRegion(HapGpuContext *context, unsigned int frameCount,
                                            const void *const *inputBuffers,
                                            const unsigned long *inputBuffersBytes,
                                            unsigned int textureCount,
                                            void *const *planeFrames,
                                            unsigned int width, unsigned int height,
                                            const unsigned int *regionXs, const unsigned int *regionYs,
                                            unsigned int regionWidth, unsigned int regionHeight,
                                            unsigned int scaleLog2, unsigned int channels, unsigned int element,
                                            unsigned long planeBytes, unsigned long rowBytes,
                                            const float *scale, const float *bias,
                                            unsigned int *results,
                                            unsigned int flags);

/* Frames in, normalised planar float tensors of a RESIZED crop per frame out: what a training or inference loader does
 * with video -- a random-resized crop, a tracked box, a tile -- in one call.  Every frame has a crop of its own, at any
 * texel position and of any size, and every crop comes out at one size, outWidth x outHeight (224 x 224, say):
 * planeFrames[f] is frame f's tensor in DEVICE memory, `channels` planes of outWidth x outHeight elements, planeBytes and
 * rowBytes shared by all frames.  cropXs, cropYs, cropWidths and cropHeights have frameCount entries each.
 * The definition, and the only one.  Let s = scaleLog2, 0 to 2, and P the picture that HapGpuDecodeFramesRGBA (s = 0) or
 * HapGpuDecodeFramesRGBAScaled (s = 1, 2) writes for the frame with the same textureCount and flags: (width >> s) x
 * (height >> s) texels.  Frame f's crop is (x, y, cw, ch) = (cropXs[f], cropYs[f], cropWidths[f], cropHeights[f]) in
 * texels of P: arbitrary integers -- no grid -- with cw, ch >= 1, x + cw <= width >> s and y + ch <= height >> s.
 * The taps of an output axis of o elements over a crop axis of c texels, in integers only (pixel centres, what torch
 * calls align_corners = false):
 *     num  = max((2 * i + 1) * c - o, 0)            i = 0 .. o - 1
 *     i0   = min(num / (2 * o), c - 1)      i1 = min(i0 + 1, c - 1)        taps never leave the crop: edge texels repeat
 *     frac = num % (2 * o)                  w  = (frac * 256 + o) / (2 * o)     0 .. 256: nearest, halves up
 * The byte of output texel (ox, oy), channel k, with x0, x1, wx from (outWidth, cw) at ox and y0, y1, wy from
 * (outHeight, ch) at oy:
 *     top = P[y + y0][x + x0][k] * (256 - wx) + P[y + y0][x + x1][k] * wx
 *     bot = P[y + y1][x + x0][k] * (256 - wx) + P[y + y1][x + x1][k] * wx
 *     v   = (top * (256 - wy) + bot * wy + 32768) >> 16                        0 .. 255
 * and the element is HapGpuDecodeFramesPlanes' conversion of v: one binary32 multiply by scale[k], then one binary32 add
 * of bias[k] (two roundings, not fused), then the rounding to the element.  All intermediates fit 32 bits.  With
 * outWidth == cw and outHeight == ch every weight is 0 and the call is an exact crop; on a block-aligned crop of that kind
 * it equals HapGpuDecodeFramesPlanesRegion bit for bit.  Bilinear filters of other libraries come close (within a byte
 * of torch's bilinear, antialias = False) but are not the definition.
 * Limits.  outWidth and outHeight are 1 to 16384.  Per frame cw <= 4 * outWidth and ch <= 4 * outHeight: the block decoder
 * stages the texels under a tile of the output in on-chip memory, and that bounds them.  With scaleLog2 that is 16 x in
 * all.  A bilinear filter aliases beyond a ratio of 2: a client that minds picks scaleLog2 so that the remaining ratio
 * is at most 2 -- the box mean of the level is the prefilter.
 * The block decoder reads only the blocks that hold texels of a frame's crop, and the second stage leaves undecoded, frame
 * by frame, every independently decodable piece that holds no byte of them (the crop taken back to full-size texels and
 * rounded outward to the block grid: HapGpuRegionNeedsBytes; counted by HapGpuSkippedTextureBytes), as
 * HapGpuDecodeFramesPlanesRegion does.
 * Tensors: device memory only.  A lane stores single elements, so the rule is the plain one: with e the element's size the
 * addresses, rowBytes and planeBytes are multiples of e, rowBytes at least outWidth * e and planeBytes at least
 * rowBytes * (outHeight - 1) + outWidth * e; a slice of a larger tensor qualifies; nothing is written between rows or
 * planes.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written -- for what HapGpuDecodeFramesPlanes refuses
 * (its tensor rule replaced by the one above), a NULL crop array, an outWidth or outHeight of 0 or above 16384.  A frame
 * whose crop is empty, past an edge of P or over the ratio cap is Bad_Arguments alone: its tensor is untouched, nothing
 * of it is handed to the second stage or the block decoder, and the other frames are decoded.  So is a frame of another
 * format or geometry, or one whose tensor is NULL, in host memory or misaligned.  A broken frame gets HapDecode's code;
 * damage wholly inside skipped pieces is not seen.  A context between HapGpuEncodeFramesRGBABegin and
 * HapGpuEncodeFramesFinish: Internal_Error.  Sources, textureCount, flags, mixed batches (one block-decode launch per
 * texture format present), slicing and result codes are HapGpuDecodeFramesPlanes': Hap, Hap Alpha, Hap Q, Hap Q Alpha.
 * Out of scope: Hap R (BC7), Hap HDR (BC6H) and Hap Alpha-Only (a lone A_RGTC1) frames as sources, host tensors, an
 * output size per frame, other filters (nearest, bicubic, antialiased), ...OnDevices and ...Sequence forms of this call,
 * and RGBA8 output. */
unsigned int HapGpuDecodeFramesPlanesResized(HapGpuContext *context, unsigned int frameCount,
                                             const void *const *inputBuffers,
                                             const unsigned long *inputBuffersBytes,
                                             unsigned int textureCount,
                                             void *const *planeFrames,
                                             unsigned int width, unsigned int height, unsigned int scaleLog2,
                                             const unsigned int *cropXs, const unsigned int *cropYs,
                                             const unsigned int *cropWidths, const unsigned int *cropHeights,
                                             unsigned int outWidth, unsigned int outHeight,
                                             unsigned int channels, unsigned int element,
                                             unsigned long planeBytes, unsigned long rowBytes,
                                             const float *scale, const float *bias,
                                             unsigned int *results,
                                             unsigned int flags);

/* How far a texture or a frame is from a picture (HapGpuMeasureTexture, HapGpuMeasureFrames): per channel the exact
 * integer sums over all width x height texels.  72 bytes. */
typedef struct HapGpuPictureError {
    unsigned long long sse[4];   /* R, G, B, A: sum over texels of (d - p)^2 */
    unsigned long long sad[4];   /* R, G, B, A: sum over texels of |d - p|   */
    unsigned long long texels;   /* width * height when measured, 0 when not */
} HapGpuPictureError;

/* One texture (+ optional RGTC1 alpha plane) against the RGBA8 picture it was made from, or any other of its size: how
 * close is the result to the source?  The block decoder adds up the errors from the texels it holds in registers; no
 * decoded picture is written.
 * The definition, and the only one.  d is the byte that HapGpuDecompressRGBA writes for a texel and channel; p is the
 * byte of the caller's picture `rgba` at that texel and channel.  error->sse[c] is the sum of (d - p)^2 and
 * error->sad[c] the sum of |d - p| over all width x height texels, c = R, G, B, A, as exact integers; error->texels is
 * width * height.  A source without alpha decodes to A = 255, as it does in that call, and is compared with the
 * picture's A like any other channel: the caller ignores sse[3] and sad[3] where they mean nothing.  The sums do not
 * depend on how the work is laid out on the device: two calls give the same struct.  PSNR of channel c is
 * 10 * log10(255^2 * texels / sse[c]), of R, G and B together 10 * log10(255^2 * 3 * texels / (sse[0] + sse[1] + sse[2])).
 * width and height are multiples of 4; textures (host or device), textureFormat -- RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5 --
 * and the alpha plane follow HapGpuDecompressRGBA's rules.  The reference picture is in DEVICE memory and 16-byte aligned;
 * rowBytes is a multiple of 16 and at least width * 4; only the picture's width * 4 bytes of each row are read, and
 * nothing is written to it.  `error` is in host memory and is written on No_Error only.
 * Bad_Arguments, and nothing written, for anything else: a host picture, a misaligned picture, a NULL error, any other
 * format.
 * Out of scope: RGBA_BPTC_UNORM (BC7) and the BC6H formats as sources, a lone A_RGTC1 against A8 pictures, RGBA16F
 * pictures, scaled or rectangular measurement, host pictures. */
unsigned int HapGpuMeasureTexture(HapGpuContext *context,
                                  const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                  const void *alphaTexture, unsigned long alphaTextureBytes,
                                  unsigned int width, unsigned int height,
                                  const void *rgba, unsigned long rowBytes, HapGpuPictureError *error);

/* Frames in, errors out: HapGpuDecodeFramesRGBA with reference pictures that are read in place of pictures that are
 * written -- rgbaFrames[f] is the RGBA8 picture in DEVICE memory that frame f is measured against (its source picture,
 * or the decoded picture of an earlier generation), and errors[f] gets the sums of HapGpuMeasureTexture for it.
 * The definition, and the only one.  d is the byte that HapGpuDecodeFramesRGBA writes for the frame at a texel and
 * channel with the same textureCount and flags; p is the byte of rgbaFrames[f] there.  errors[f].sse[c] is the sum of
 * (d - p)^2 and errors[f].sad[c] the sum of |d - p| over all width x height texels, exact integers; errors[f].texels
 * is width * height.  A frame without alpha gives A = 255, compared like any other channel.  Two calls give the same
 * structs.  No decoded picture ever exists: per Hap Q block 16 bytes of texture and 64 of the picture are read and
 * nothing is written but a few sums.
 * Frames, textureCount, formats (Hap, Hap Alpha, Hap Q, Hap Q Alpha), the flags of the second stage, mixed batches (one
 * block launch per texture format present), slicing and results[f] are HapGpuDecodeFramesRGBA's, without
 * HAPGPU_DECODE_BPTC_PICTURES, which is ignored.  A frame that fails -- a broken frame gets HapDecode's code; a frame of
 * another format or geometry, or one whose picture is NULL, in host memory or misaligned, Bad_Arguments -- fails alone:
 * its errors[f] is all zero and the other frames are measured.  The function's result is the first failure.  errors
 * and results are HOST arrays of frameCount entries.  Pictures are 16-byte aligned, rowBytes is a multiple of 16 and at
 * least width * 4, shared by all frames; only the pictures' bytes of each row are read.
 * Bad_Arguments for the whole call -- every results[f] set, nothing else written -- for a NULL array (errors among
 * them), a width or height that is no multiple of 4, a rowBytes that is too short or no multiple of 16.  A context
 * between HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: Hap R (BC7) and Hap HDR (BC6H) frames, Hap Alpha-Only frames (a lone A_RGTC1) against A8 pictures --
 * Bad_Arguments alone --, RGBA16F pictures, scaled or rectangular measurement, ...OnDevices and ...Sequence forms of
 * this call, host pictures. */
unsigned int HapGpuMeasureFrames(HapGpuContext *context, unsigned int frameCount,
                                 const void *const *inputBuffers,
                                 const unsigned long *inputBuffersBytes,
                                 unsigned int textureCount,
                                 const void *const *rgbaFrames,
                                 unsigned int width, unsigned int height, unsigned long rowBytes,
                                 HapGpuPictureError *errors,
                                 unsigned int *results,
                                 unsigned int flags);

/* The most layers one compositing call takes (HapGpuCompositeTextures, HapGpuCompositeFrames) */
#define HAPGPU_COMPOSITE_MAX_LAYERS 16u

/* Textures in, one picture out: layerCount textures (+ optional RGTC1 alpha planes) of one geometry go "over" a
 * background colour, bottom to top, and the result is one RGBA8 picture of width x height -- a matte, a keyed clip or a
 * title over a background; with two layers and an opacity, a cross-dissolve.  The block decoder blends the texels it
 * holds in registers into a canvas block it keeps there too: no layer's decoded picture is written or read.
 * The definition, and the only one; all of it is integer arithmetic on bytes.  The canvas is an RGBA8 picture whose
 * colour is premultiplied by its alpha (with an opaque background: the same as straight alpha); layers are straight
 * alpha, as HapGpuDecompressRGBA writes them.  rdiv255(x) is the integer nearest to x / 255 for 0 <= x <= 65025 (no x
 * lies on a tie: 255 is odd); it equals t = x + 128; (t + (t >> 8)) >> 8, and (2x + 255) / 510 rounded down.  Every
 * texel of the canvas starts as background[0 .. 3] = R, G, B, A, taken as they are (R, G, B <= A is not checked; NULL:
 * 0, 0, 0, 255).  Layers are applied in order l = 0 .. layerCount - 1.  For a texel, (Rs, Gs, Bs, As) are the bytes
 * HapGpuDecompressRGBA writes there for textures[l] with textureFormats[l] and alphaTextures[l] (a source without alpha:
 * As = 255), o = opacities[l] (NULL: all 255), (Rd, Gd, Bd, Ad) the canvas:
 *     a  = rdiv255(As * o)
 *     Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
 *     Ad = a + rdiv255(Ad * (255 - a))           (never above 255)
 * The picture written is the canvas after the last layer.  So a = 255 replaces the texel, a = 0 leaves it unchanged,
 * and a single RGB_DXT1 or YCoCg_DXT5 layer without a plane at opacity 255 gives HapGpuDecompressRGBA's picture byte for
 * byte, whatever the background.  Two calls give the same bytes.
 * Every layer has the canvas's width x height, both multiples of 4.  textures, texturesBytes and textureFormats have
 * layerCount entries; the formats are RGB_DXT1, RGBA_DXT5 and YCoCg_DXT5, and layers may differ in format.
 * alphaTextures (and alphaTexturesBytes) may be NULL, and so may any entry: a layer with an entry has that RGTC1 plane
 * for its alpha.  Textures and planes are in host or device memory and follow HapGpuDecompressRGBA's rules (device
 * textures aligned to their blocks, device planes to 8 bytes).  The picture follows them too: host or device, rowBytes a
 * multiple of 16 and at least width * 4, a device picture 16-byte aligned, a host picture with longer rows written row
 * by row; only the picture's own width * 4 bytes of each row are ever written.
 * Bad_Arguments, and nothing written, for a NULL required array or picture, a layerCount of 0 or above
 * HAPGPU_COMPOSITE_MAX_LAYERS, a width or height that is no multiple of 4, a rowBytes that is short or misaligned, a NULL
 * or short texture, any other format, a misaligned device address.  A context between HapGpuEncodeFramesRGBABegin and
 * HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: layers of other sizes or at an offset, scaled or rectangular canvases; blend modes other than "over"; an
 * existing picture as the bottom layer; RGBA_BPTC_UNORM (Hap R), BC6H (Hap HDR) and lone A_RGTC1 (Hap Alpha-Only) layers;
 * planar or RGBA16F output; skipping layers hidden under an opaque one. */
unsigned int HapGpuCompositeTextures(HapGpuContext *context, unsigned int layerCount,
                                     const void *const *textures, const unsigned long *texturesBytes,
                                     const unsigned int *textureFormats,
                                     const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                     const unsigned char *opacities,
                                     const unsigned char *background,
                                     unsigned int width, unsigned int height, void *rgba, unsigned long rowBytes);

/* Frames in, one picture per output frame out: HapGpuCompositeTextures for frameCount output frames of layerCount layers
 * each.  inputBuffers[f * layerCount + l] (inputBuffersBytes likewise) is the Hap frame of layer l of output frame f,
 * layer 0 at the bottom; rgbaFrames[f] is output frame f's RGBA8 picture.  All frameCount * layerCount frames of a slice
 * go through the second stage in one batch into the context's texture scratch (at most 4 GiB of block textures and
 * 32768 textures at a time: longer calls are worked through in slices of output frames), and one compositing launch per
 * slice follows.  A dissolve is two layers with opacities that change from output frame to output frame.
 * The definition, and the only one; all of it is integer arithmetic on bytes.  The canvas is an RGBA8 picture whose
 * colour is premultiplied by its alpha; layers are straight alpha.  rdiv255(x) is the integer nearest to x / 255 for
 * 0 <= x <= 65025: t = x + 128; (t + (t >> 8)) >> 8.  Every texel of output frame f's canvas starts as background[0 .. 3]
 * = R, G, B, A, taken as they are (NULL: 0, 0, 0, 255); then, for l = 0 .. layerCount - 1, with (Rs, Gs, Bs, As) the
 * bytes HapGpuDecodeFramesRGBA writes there for that layer's frame with textureCounts[l] and the call's flags (a source
 * without alpha: As = 255), o = opacities[f * layerCount + l] (NULL: all 255) and (Rd, Gd, Bd, Ad) the canvas:
 *     a  = rdiv255(As * o)
 *     Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
 *     Ad = a + rdiv255(Ad * (255 - a))           (never above 255)
 * The picture written is the canvas after the last layer: a = 255 replaces the texel, a = 0 leaves it unchanged, and a
 * single Hap or Hap Q layer at opacity 255 gives HapGpuDecodeFramesRGBA's picture byte for byte, whatever the background.
 * Two calls give the same bytes.
 * Every layer has the canvas's width x height, both multiples of 4.  textureCounts has layerCount entries (NULL: all 1):
 * with 2, layer l holds Hap Q Alpha frames; with 1, Hap, Hap Alpha or Hap Q frames, and a Hap Q Alpha frame read with 1
 * is its colour texture alone, as in HapGpuDecodeFramesRGBA.  A layer may hold different flavours in different output
 * frames.  Frames are in host or device memory, as for HapGpuDecodeFramesRGBA; flags are the decode flags of
 * HapGpuDecodeFrameTextures, and HAPGPU_DECODE_BPTC_PICTURES is ignored.  Pictures follow HapGpuDecodeFramesRGBA's
 * rules: host or device, rowBytes a multiple of 16 and at least width * 4, shared by all output frames, device pictures
 * 16-byte aligned, host pictures with longer rows written row by row; only a picture's own bytes of each row are ever
 * written.
 * results is a HOST array of frameCount * layerCount entries: results[f * layerCount + l] is HapDecode's code for that
 * layer's frame, and Bad_Arguments for a frame of another format or geometry than the call says.  Output picture f is
 * written if and only if all its layers are No_Error and its picture pointer is usable; otherwise it is untouched, and
 * the other output frames are still composited.  For a NULL or misaligned picture every entry of that output frame is
 * Bad_Arguments.  The function's result is the first failure.
 * Bad_Arguments for the whole call -- every result set, nothing written, no device touched -- for a NULL required
 * array (a NULL results: nothing to set), a layerCount of 0 or above HAPGPU_COMPOSITE_MAX_LAYERS, a width or height that
 * is no multiple of 4, a rowBytes that is short or misaligned, a textureCounts entry other than 1 or 2.  A context
 * between HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: layers of other sizes or at an offset, scaled or rectangular canvases; blend modes other than "over"; an
 * existing picture as the bottom layer; Hap R, Hap HDR and Hap Alpha-Only layers -- Bad_Arguments alone --; planar or
 * RGBA16F output; skipping layers hidden under an opaque one; ...OnDevices and ...Sequence forms of this call. */
unsigned int HapGpuCompositeFrames(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                   const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                   const unsigned int *textureCounts,
                                   const unsigned char *opacities,
                                   const unsigned char *background,
                                   void *const *rgbaFrames,
                                   unsigned int width, unsigned int height, unsigned long rowBytes,
                                   unsigned int *results,
                                   unsigned int flags);

/* A rectangle of a layer's picture and where it goes on the canvas of a placed compositing call
 * (HapGpuCompositeTexturesPlaced, HapGpuCompositeFramesPlaced).  All six fields are multiples of 4: placements stay on the
 * grid of 4 x 4 blocks. */
typedef struct HapGpuPlacement {
    unsigned int srcX, srcY, width, height;  /* a rectangle of the layer's picture, in texels */
    int dstX, dstY;                          /* where the rectangle's top-left texel lands on the canvas */
} HapGpuPlacement;

/* HapGpuCompositeTextures for layers of sizes of their own, each placed and clipped on the canvas: a picture-in-picture
 * inset, a lower third, a logo in a corner, a mosaic of clips, a window of a large clip on a smaller output.  The block
 * decoder still blends the texels it holds in registers into a canvas block it keeps there: no layer's decoded picture
 * is written or read, and a canvas block outside a layer's rectangle does not read that layer at all.
 * The definition, and the only one.  The canvas is width x height, both multiples of 4.  Layer l is
 * layerWidths[l] x layerHeights[l], both multiples of 4 and not 0; placements[l] is its placement.  A canvas texel (x, y)
 * is covered by the layer when dstX <= x < dstX + width and dstY <= y < dstY + height (the placement's).  For a covered
 * texel, (Rs, Gs, Bs, As) are the bytes HapGpuDecompressRGBA writes at (srcX + x - dstX, srcY + y - dstY) of the layer's
 * picture, and HapGpuCompositeTextures' three formulas apply unchanged, with its canvas, background, opacities and order
 * of layers:
 *     a  = rdiv255(As * o)
 *     Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
 *     Ad = a + rdiv255(Ad * (255 - a))           (never above 255)
 * A texel that is not covered is left as the canvas has it.  Whatever of the rectangle falls outside the canvas is
 * clipped; a rectangle wholly outside contributes nothing and is no error.  placements == NULL means every layer whole
 * at (0, 0): {0, 0, layerWidths[l], layerHeights[l], 0, 0}; with every layer of the canvas's size that is
 * HapGpuCompositeTextures' picture byte for byte.  Two calls give the same bytes.
 * textures, texturesBytes, textureFormats, alphaTextures, alphaTexturesBytes, opacities, background, rgba and rowBytes are
 * HapGpuCompositeTextures' and follow its rules, a texture and a plane having their own layer's blocks.
 * Bad_Arguments, and nothing written and no device touched, for any of the six placement fields not a multiple of 4, a
 * placement width or height of 0, a rectangle that leaves its layer (srcX + width above layerWidths[l], srcY + height
 * above layerHeights[l]), |dstX| or |dstY| above 1 << 20, a layer size that is 0 or no multiple of 4 (or of 2^32 blocks
 * and more), a NULL layerWidths or layerHeights, and everything HapGpuCompositeTextures refuses already.
 * Out of scope: placements off the block grid; scaled or rotated layers; blend modes other than "over"; an existing
 * picture as the bottom layer; Hap R, Hap HDR and Hap Alpha-Only layers; planar, NV12 or encoded output. */
unsigned int HapGpuCompositeTexturesPlaced(HapGpuContext *context, unsigned int layerCount,
                                           const void *const *textures, const unsigned long *texturesBytes,
                                           const unsigned int *textureFormats,
                                           const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                           const unsigned int *layerWidths, const unsigned int *layerHeights,
                                           const HapGpuPlacement *placements,
                                           const unsigned char *opacities,
                                           const unsigned char *background,
                                           unsigned int width, unsigned int height, void *rgba, unsigned long rowBytes);

/* HapGpuCompositeFrames for layers of sizes of their own, each placed and clipped on the canvas, with a placement per
 * layer and output frame: placements[f * layerCount + l] is layer l's in output frame f, so an inset may move from frame
 * to frame.  The canvas is width x height and layer l is layerWidths[l] x layerHeights[l], all multiples of 4 and not 0;
 * a layer's size is the same in every output frame.
 * The definition, and the only one, is HapGpuCompositeTexturesPlaced's with HapGpuDecodeFramesRGBA's bytes: a canvas
 * texel (x, y) of output frame f is covered by layer l when dstX <= x < dstX + width and dstY <= y < dstY + height; for a
 * covered texel, (Rs, Gs, Bs, As) are the bytes HapGpuDecodeFramesRGBA writes at (srcX + x - dstX, srcY + y - dstY) of
 * the picture of that layer's frame, read with textureCounts[l] and the call's flags, and HapGpuCompositeFrames' three
 * formulas apply unchanged:
 *     a  = rdiv255(As * o)
 *     Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
 *     Ad = a + rdiv255(Ad * (255 - a))           (never above 255)
 * A texel that is not covered is left as the canvas has it.  Whatever of the rectangle falls outside the canvas is
 * clipped; a rectangle wholly outside contributes nothing and is no error.  placements == NULL means every layer whole
 * at (0, 0) in every output frame: {0, 0, layerWidths[l], layerHeights[l], 0, 0}; with every layer of the canvas's size
 * that is HapGpuCompositeFrames' picture byte for byte.  Two calls give the same bytes.
 * A layer's frame must hold a colour texture of exactly layerWidths[l] x layerHeights[l], and with textureCounts[l] == 2
 * an RGTC1 plane of the same size: otherwise that entry of results is Bad_Arguments and that output frame is untouched.
 * The second stage decodes every layer's whole frame, whatever of it the clip hides.  results, and that output picture f
 * is written if and only if all its layers are No_Error and its picture pointer is usable; frames and pictures in host
 * or device memory and the staging of host pictures; slices of at most 4 GiB of block textures and 32768 textures: all
 * as HapGpuCompositeFrames has them.
 * Bad_Arguments for the whole call -- every result set, nothing written, no device touched -- for any of the six
 * placement fields of any placement not a multiple of 4, a placement width or height of 0, a rectangle that leaves its
 * layer, |dstX| or |dstY| above 1 << 20, a layer size that is 0 or no multiple of 4 (or of 2^32 blocks and more), a NULL
 * layerWidths or layerHeights, and everything HapGpuCompositeFrames refuses already.
 * Out of scope: placements off the block grid; scaled or rotated layers; skipping the second stage of what a clip
 * hides; blend modes other than "over"; an existing picture as the bottom layer; Hap R, Hap HDR and Hap Alpha-Only
 * layers; planar, NV12 or encoded output; ...OnDevices and ...Sequence forms of this call. */
unsigned int HapGpuCompositeFramesPlaced(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                         const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                         const unsigned int *textureCounts,
                                         const unsigned int *layerWidths, const unsigned int *layerHeights,
                                         const HapGpuPlacement *placements,
                                         const unsigned char *opacities,
                                         const unsigned char *background,
                                         void *const *rgbaFrames,
                                         unsigned int width, unsigned int height, unsigned long rowBytes,
                                         unsigned int *results,
                                         unsigned int flags);

/* HapGpuCompositeTexturesPlaced with the canvas going out as `count` block textures instead of an RGBA8 picture: the
 * compositing kernel hands the canvas block it holds in registers to the block encoder, as HapGpuTranscodeTexture's kernel
 * hands over a decoded block.  No picture of the canvas is written or read: per canvas block one block is stored, where
 * a compositing call followed by HapGpuCompressRGBA writes 64 bytes and reads them again.
 * The definition, and the only one: outputs[i] is byte for byte what HapGpuCompressRGBA(..., outputFormats[i], ...,
 * flags 0) makes of the picture HapGpuCompositeTexturesPlaced writes for the same layers, layerWidths, layerHeights,
 * placements, opacities, background, width and height, with rowBytes = width * 4.  The canvas bytes go to the encoder as
 * they are: the canvas is premultiplied by its alpha, so with an opaque background the result is opaque and the same
 * as straight alpha, and with any other background the textures hold premultiplied colour.  Two calls give the same
 * bytes.
 * Destination sets, the four HapGpuTranscodeTexture makes -- count 1: RGB_DXT1 (Hap), RGBA_DXT5 (Hap Alpha) or
 * YCoCg_DXT5 (Hap Q); count 2: YCoCg_DXT5 then A_RGTC1 (Hap Q Alpha, both textures in one pass).  Outputs are in host or
 * device memory, device outputs aligned to their blocks; outputsBytesUsed may be NULL.  The layer arguments are
 * HapGpuCompositeTexturesPlaced's and follow its rules.
 * Bad_Arguments, and nothing written and no device touched, for everything HapGpuCompositeTexturesPlaced refuses of its
 * layer sizes, placements, layerCount, width and height, a canvas of more than 65535 block rows, a count of 0 or above
 * 2, any other destination set, a NULL required array; Bad_Arguments, and nothing written, for a NULL or short texture,
 * another layer format, a NULL output, a misaligned device address; Buffer_Too_Small for an output shorter than its
 * texture.  A context between HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: scaled or rotated layers; RGBA_BPTC_UNORM (BC7), BC6H and Alpha-Only (lone A_RGTC1) layers or
 * destinations; refined end points; NV12 or planar output; un-premultiplying the canvas. */
unsigned int HapGpuCompositeTexturesEncoded(HapGpuContext *context, unsigned int layerCount,
                                            const void *const *textures, const unsigned long *texturesBytes,
                                            const unsigned int *textureFormats,
                                            const void *const *alphaTextures, const unsigned long *alphaTexturesBytes,
                                            const unsigned int *layerWidths, const unsigned int *layerHeights,
                                            const HapGpuPlacement *placements,
                                            const unsigned char *opacities,
                                            const unsigned char *background,
                                            unsigned int width, unsigned int height,
                                            unsigned int count, const unsigned int *outputFormats,
                                            void *const *outputs, const unsigned long *outputsBytes,
                                            unsigned long *outputsBytesUsed);

/* Layers of frames in, one Hap frame per output frame out: HapGpuCompositeFramesPlaced whose canvases go on to the encoder
 * as HapGpuTranscodeFrames' textures do -- a title or lower third baked into a master, a dissolve or a mosaic rendered
 * into one Hap movie, a programme output recorded.  The input side (inputBuffers, inputBuffersBytes, textureCounts,
 * layerWidths, layerHeights, placements, opacities, background, width, height, decodeFlags) is
 * HapGpuCompositeFramesPlaced's; the output side (count, textureFormats, compressors, chunkCounts, outputBuffers,
 * outputBuffersBytes, outputBuffersBytesUsed, results, encodeFlags) is HapGpuTranscodeFrames'.
 * The definition, and the only one: output frame f is byte for byte, and in outputBuffersBytesUsed, the frame
 * HapGpuEncodeFramesRGBA(..., width, height, width * 4, count, textureFormats, compressors, chunkCounts, ...,
 * encodeFlags) makes of the picture HapGpuCompositeFramesPlaced writes for the same layers, placements, opacities and
 * background -- encodeFlags without HAPGPU_ENCODE_BPTC_BLOCKS and HAPGPU_ENCODE_REFINE_ENDPOINTS, which are ignored as
 * in HapGpuTranscodeFrames.  The canvas bytes go to the encoder as they are: the canvas is premultiplied by its alpha,
 * so with an opaque background the result is opaque.  No such picture ever exists: the layers' textures go from the
 * decoder's second stage through HapGpuCompositeTexturesEncoded's kernel (one launch per slice) to the encoder's second
 * stage, and the host is waited for twice per slice.  Two calls give the same bytes.
 * Destination sets, the four of HapGpuCompositeTexturesEncoded -- count 1: RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; count 2:
 * YCoCg_DXT5 then A_RGTC1.  Buffers may be host or device.  Slices: at most 4 GiB of block textures, the canvases' among
 * them, and 32768 textures of the second stage at a time.
 * layerResults is a HOST array of frameCount * layerCount entries: layerResults[f * layerCount + l] is what
 * HapGpuCompositeFramesPlaced sets for that layer's frame -- HapDecode's code, Bad_Arguments for a frame of another
 * format or geometry than the call says.  results is a HOST array of frameCount entries.  Output frame f is encoded if
 * and only if all its layers are No_Error; otherwise results[f] is the first failing layer's code,
 * outputBuffersBytesUsed[f] is 0 and its output buffer is untouched.  Where the layers are in order results[f] is the
 * encode's code, as HapGpuEncodeFramesRGBA sets it (a NULL output: Bad_Arguments, a short one: Buffer_Too_Small), and
 * a failed frame does not disturb its neighbours.  The function's result is the first failure in results.
 * Bad_Arguments for the whole call -- every entry of results and of layerResults set, nothing written, no device
 * touched, before the context is looked at -- for everything HapGpuCompositeFramesPlaced refuses of its layer sizes,
 * placements, layerCount, textureCounts, width and height, a canvas of more than 65535 block rows, a count of 0 or
 * above 2, any other destination set, what HapGpuEncodeFrames refuses of textureFormats, compressors and chunkCounts,
 * and a NULL required array (a NULL results or layerResults: the other is still set).  A context between
 * HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: scaled or rotated layers; Hap R (BC7), Hap HDR (BC6H) and Hap Alpha-Only layers or destinations;
 * refined end points; NV12 or planar output; un-premultiplying the canvas; ...OnDevices, ...Sequence and ...Begin forms
 * of this call. */
unsigned int HapGpuCompositeFramesEncoded(HapGpuContext *context, unsigned int frameCount, unsigned int layerCount,
                                          const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                          const unsigned int *textureCounts,
                                          const unsigned int *layerWidths, const unsigned int *layerHeights,
                                          const HapGpuPlacement *placements,
                                          const unsigned char *opacities,
                                          const unsigned char *background,
                                          unsigned int width, unsigned int height,
                                          unsigned int count, const unsigned int *textureFormats,
                                          const unsigned int *compressors, const unsigned int *chunkCounts,
                                          void *const *outputBuffers, const unsigned long *outputBuffersBytes,
                                          unsigned long *outputBuffersBytesUsed,
                                          unsigned int *layerResults, unsigned int *results,
                                          unsigned int decodeFlags, unsigned int encodeFlags);

/* Planar float tensors in, frames out -- the way back of HapGpuDecodeFramesPlanes: HapGpuEncodeFramesRGBA with the tensors of
 * HapGpuCompressPlanes in place of pictures.  planeFrames[f] is frame f's tensor in DEVICE memory, `channels` planes of
 * width x height elements, planeBytes and rowBytes shared by all frames (one N x C x H x W tensor: planeFrames[f] = base +
 * f * channels * planeBytes).  The definition is HapGpuCompressPlanes': per element one binary32 multiply by scale[c],
 * then one binary32 add of bias[c] (two roundings, not fused), then NaN -> 0, anything not above 0 -> 0, 255 and above ->
 * 255, else to nearest with halves to even (0.5 -> 0, 1.5 -> 2); with channels 3, A is 255.  Every frame is byte for byte,
 * and in outputBuffersBytesUsed, what HapGpuEncodeFramesRGBA makes of the tensor's picture with the same count,
 * textureFormats, compressors, chunkCounts and flags.  No RGBA8 picture ever exists: per Hap Q block 96 bytes are read
 * from three half planes and 16 written, where converting with a tensor library first reads 96, writes 64 and reads 64
 * again.  The block encoder runs as a pass of its own in front of the second stage (the road RGB_DXT1 takes from RGBA8
 * pictures), never inside the fused compress kernel.
 * count 1: RGB_DXT1 (Hap), RGBA_DXT5 (Hap Alpha), YCoCg_DXT5 (Hap Q) or A_RGTC1 (Hap Alpha-Only, from the fourth plane);
 * count 2: YCoCg_DXT5 then A_RGTC1 (Hap Q Alpha), both textures from one pass over the planes.  Second stage, frame
 * layout, chunk limiting, store-raw decisions, Buffer_Too_Small and every encode flag are HapGpuEncodeFrames';
 * HAPGPU_ENCODE_BPTC_BLOCKS is ignored, HAPGPU_ENCODE_REFINE_ENDPOINTS is honoured (count 1, RGB_DXT1 and RGBA_DXT5: the
 * blocks HapGpuEncodeFramesRGBA makes with it of the pictures of the quantised bytes).  scale and bias point to `channels` floats each and are copied by the call.
 * Alignment as for HapGpuCompressPlanes.  ...Begin is the first half of the call as HapGpuEncodeFramesRGBABegin is (at
 * most 32768 frames; scale and bias need live no longer than the other argument arrays); HapGpuEncodeFramesFinish
 * finishes it.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written, no device touched -- for a NULL array, scale
 * or bias, a width or height that is no multiple of 4, channels other than 3 or 4, an element outside the enum, a
 * rowBytes or planeBytes that breaks the alignment rule or is too short, more than 65535 block rows, a set of formats
 * outside the above.  A frame whose tensor is NULL, in host memory or misaligned is Bad_Arguments alone, its output
 * buffer untouched, and the other frames are encoded.  The function's result is the first failure.  A context between a
 * ...Begin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: Hap R (BC7) and Hap HDR (BC6H) destinations, a one-plane tensor as a Hap Alpha-Only source, host
 * tensors, scaled or rectangular sources, ...OnDevices and ...Sequence forms of this call, and reading the planes inside
 * the fused compress kernel. */
unsigned int HapGpuEncodeFramesPlanes(HapGpuContext *context, unsigned int frameCount,
                                      const void *const *planeFrames,
                                      unsigned int channels, unsigned int element,
                                      unsigned long planeBytes, unsigned long rowBytes,
                                      const float *scale, const float *bias,
                                      unsigned int width, unsigned int height,
                                      unsigned int count,
                                      const unsigned int *textureFormats,
                                      const unsigned int *compressors,
                                      const unsigned int *chunkCounts,
                                      void *const *outputBuffers,
                                      const unsigned long *outputBuffersBytes,
                                      unsigned long *outputBuffersBytesUsed,
                                      unsigned int *results,
                                      unsigned int flags);
unsigned int HapGpuEncodeFramesPlanesBegin(HapGpuContext *context, unsigned int frameCount,
                                           const void *const *planeFrames,
                                           unsigned int channels, unsigned int element,
                                           unsigned long planeBytes, unsigned long rowBytes,
                                           const float *scale, const float *bias,
                                           unsigned int width, unsigned int height,
                                           unsigned int count,
                                           const unsigned int *textureFormats,
                                           const unsigned int *compressors,
                                           const unsigned int *chunkCounts,
                                           void *const *outputBuffers,
                                           const unsigned long *outputBuffersBytes,
                                           unsigned long *outputBuffersBytesUsed,
                                           unsigned int *results,
                                           unsigned int flags);

/* The colour matrix and the range of a video picture's Y, Cb, Cr samples (HapGpuCompressNV12, HapGpuEncodeFramesNV12,
 * HapGpuDecompressNV12, HapGpuDecodeFramesNV12) */
enum HapGpuYCbCrMatrix { HapGpuYCbCrMatrix_BT601 = 0, HapGpuYCbCrMatrix_BT709 = 1 };
enum HapGpuYCbCrRange { HapGpuYCbCrRange_Limited = 0, HapGpuYCbCrRange_Full = 1 };

/* One NV12 video picture in DEVICE memory -> one block-compressed texture: what a hardware video decoder leaves of
 * H.264, HEVC or ProRes footage, converted to RGB by the block encoder itself as it loads the samples: no RGBA8 picture
 * is written or read back.  NV12 is a Y plane of width x height bytes (luma, rows lumaRowBytes apart) and a plane of
 * (width / 2) x (height / 2) interleaved Cb, Cr byte pairs (chroma, rows chromaRowBytes apart).
 * The definition.  Texel (x, y) takes Y[y][x] and the pair Cb, Cr = UV[y >> 1][2 * (x >> 1)], UV[y >> 1][2 * (x >> 1) + 1]:
 * chroma is replicated over its 2 x 2 luma samples, with no filtering across samples.  With y' = Y - 16 (Limited) or Y
 * (Full), u = Cb - 128 and v = Cr - 128, all in 32-bit signed integers with >> arithmetic:
 *     R = clamp255((cy * y' + crv * v           + 32768) >> 16)
 *     G = clamp255((cy * y' - cgu * u - cgv * v + 32768) >> 16)
 *     B = clamp255((cy * y' + cbu * u           + 32768) >> 16)        A = 255
 * where clamp255 holds its argument to 0 .. 255 and the coefficients are the standards' exact rationals times 65536,
 * rounded to nearest -- Kr, Kb = 0.299, 0.114 (BT601) or 0.2126, 0.0722 (BT709); Limited scales luma by 255/219 and
 * chroma by 255/224:
 *     matrix, range        cy     crv     cbu    cgu    cgv
 *     BT601  Limited    76309  104597  132201  25675  53279
 *     BT601  Full       65536   91881  116130  22553  46802
 *     BT709  Limited    76309  117489  138438  13975  34925
 *     BT709  Full       65536  103206  121609  12276  30679
 * The accumulators stay below 3.6e7 in magnitude; before the clamp every channel is within 0.5016 of the exact real
 * value.  Samples outside the nominal range or the gamut (Y < 16, Y > 235, ...) are simply clamped: defined behaviour,
 * not an error.  The picture of an NV12 source is the RGBA8 picture of these bytes, and the texture is byte for byte what
 * HapGpuCompressRGBA makes of that picture: YCoCg_DXT5 goes YCbCr -> RGB bytes -> the YCoCg block code, with no direct
 * YCbCr -> YCoCg shortcut.
 * textureFormat: RGB_DXT1 or YCoCg_DXT5.  output is host or device, under HapGpuCompressRGBA's rules (a device output
 * aligned to its blocks; too small: Buffer_Too_Small).  width and height multiples of 4, at most 65535 block rows.  Both
 * planes are in device memory; their addresses and both pitches are multiples of 4, what a lane loads per row;
 * lumaRowBytes >= width and chromaRowBytes >= width (width / 2 pairs).  Only the samples are read, nothing between rows.
 * Bad_Arguments, and nothing written, for anything else: a NULL, host or misaligned plane, a matrix or range outside the
 * enums, another format, a bad pitch.
 * Out of scope here: the way back (textures or frames -> NV12) is HapGpuDecompressNV12 and HapGpuDecodeFramesNV12's; P010
 * and other 10/16-bit layouts; planar I420, 4:2:2 and 4:4:4; filtered or sited chroma upsampling, which needs neighbours
 * across blocks; a separate A8 plane, and with it Hap Alpha, Hap Q Alpha and Hap Alpha-Only destinations; BC7 / BC6H
 * destinations; host pictures. */
unsigned int HapGpuCompressNV12(HapGpuContext *context,
                                const void *luma, unsigned long lumaRowBytes,
                                const void *chroma, unsigned long chromaRowBytes,
                                unsigned int matrix, unsigned int range,
                                unsigned int width, unsigned int height, unsigned int textureFormat,
                                void *output, unsigned long outputBytes,
                                unsigned long *outputBytesUsed);

/* NV12 video pictures in, frames out: HapGpuEncodeFramesRGBA with the pictures of HapGpuCompressNV12 in place of RGBA8
 * ones.  lumaPlanes[f] and chromaPlanes[f] are frame f's Y plane and its plane of interleaved Cb, Cr pairs, both in DEVICE
 * memory, lumaRowBytes and chromaRowBytes shared by all frames.  The definition is HapGpuCompressNV12's: texel (x, y)
 * takes Y[y][x] and the pair UV[y >> 1][2 * (x >> 1)], UV[y >> 1][2 * (x >> 1) + 1] (chroma replicated over 2 x 2 luma
 * samples, no filtering), and with y' = Y - 16 (Limited) or Y (Full), u = Cb - 128, v = Cr - 128 in 32-bit integers
 *     R = clamp255((cy * y' + crv * v + 32768) >> 16)      G = clamp255((cy * y' - cgu * u - cgv * v + 32768) >> 16)
 *     B = clamp255((cy * y' + cbu * u + 32768) >> 16)      A = 255
 * with the coefficients of the table there (matrix: HapGpuYCbCrMatrix, range: HapGpuYCbCrRange).  Every frame is byte
 * for byte, and in outputBuffersBytesUsed, what HapGpuEncodeFramesRGBA makes of the RGBA8 picture of these bytes with
 * the same count, textureFormats, compressors, chunkCounts and flags.  No RGBA8 picture ever exists: per block 24 bytes
 * are read and 8 or 16 written, where converting with a tensor library first reads 24, writes 64 and reads 64 again.
 * The block encoder runs as a pass of its own in front of the second stage, never inside the fused compress kernel.
 * count == 1 with RGB_DXT1 (Hap) or YCoCg_DXT5 (Hap Q).  Second stage, frame layout, chunk limiting, store-raw
 * decisions, Buffer_Too_Small, results[] and every encode flag are HapGpuEncodeFramesPlanes': HAPGPU_ENCODE_BPTC_BLOCKS
 * is ignored, HAPGPU_ENCODE_REFINE_ENDPOINTS is honoured (RGB_DXT1: the blocks HapGpuEncodeFramesRGBA makes with it of
 * the converted pictures).  Plane addresses and both pitches are multiples of 4; lumaRowBytes >= width, chromaRowBytes >=
 * width; width and height multiples of 4, at most 65535 block rows.  ...Begin is the first half of the call as
 * HapGpuEncodeFramesRGBABegin is (at most 32768 frames; the two arrays of planes are copied by the call and need live
 * no longer than the other argument arrays); HapGpuEncodeFramesFinish finishes it.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written, no device touched -- for a NULL array, a
 * matrix or range outside the enums, a width or height that is no multiple of 4, a pitch that is no multiple of 4 or
 * below width, more than 65535 block rows, count == 2 or another format.  A frame either of whose planes is NULL, in
 * host memory or misaligned is Bad_Arguments alone, its output buffer untouched, and the other frames are encoded.  The
 * function's result is the first failure.  A context between a ...Begin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope here: the way back (frames -> NV12) is HapGpuDecodeFramesNV12's; P010 and other 10/16-bit layouts; planar
 * I420, 4:2:2 and 4:4:4; filtered or sited chroma upsampling, which needs neighbours across blocks; a separate A8 plane,
 * and with it Hap Alpha, Hap Q Alpha and Hap Alpha-Only destinations; BC7 / BC6H destinations; host pictures;
 * ...OnDevices and ...Sequence forms of this call; and reading the planes inside the fused compress kernel. */
unsigned int HapGpuEncodeFramesNV12(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *lumaPlanes, unsigned long lumaRowBytes,
                                    const void *const *chromaPlanes, unsigned long chromaRowBytes,
                                    unsigned int matrix, unsigned int range,
                                    unsigned int width, unsigned int height,
                                    unsigned int count,
                                    const unsigned int *textureFormats,
                                    const unsigned int *compressors,
                                    const unsigned int *chunkCounts,
                                    void *const *outputBuffers,
                                    const unsigned long *outputBuffersBytes,
                                    unsigned long *outputBuffersBytesUsed,
                                    unsigned int *results,
                                    unsigned int flags);
unsigned int HapGpuEncodeFramesNV12Begin(HapGpuContext *context, unsigned int frameCount,
                                         const void *const *lumaPlanes, unsigned long lumaRowBytes,
                                         const void *const *chromaPlanes, unsigned long chromaRowBytes,
                                         unsigned int matrix, unsigned int range,
                                         unsigned int width, unsigned int height,
                                         unsigned int count,
                                         const unsigned int *textureFormats,
                                         const unsigned int *compressors,
                                         const unsigned int *chunkCounts,
                                         void *const *outputBuffers,
                                         const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed,
                                         unsigned int *results,
                                         unsigned int flags);

/* The way back of HapGpuCompressNV12: one block-compressed texture -> one NV12 video picture in DEVICE memory, what a
 * video encoder or a network sender takes, converted from RGB by the block decoder itself before it stores: no RGBA8
 * picture is written or read back.  The picture is W x H = (width >> scaleLog2) x (height >> scaleLog2): a Y plane of
 * W x H bytes (luma, rows lumaRowBytes apart) and a plane of (W / 2) x (H / 2) interleaved Cb, Cr byte pairs (chroma,
 * rows chromaRowBytes apart).
 * The definition.  d is the RGBA8 picture HapGpuDecompressRGBA writes for the texture at scaleLog2 == 0, and at
 * scaleLog2 1 or 2 the one HapGpuDecompressRGBAScaled writes; alpha is ignored.  All in 32-bit signed integers with >>
 * arithmetic:
 *     Y[y][x]  = lo + ((yr * R + yg * G + yb * B + 32768) >> 16)      of texel d(x, y); no clamp is ever needed
 *     Rs, Gs, Bs = the sums of R, G, B over the four texels d(2i..2i+1, 2j..2j+1)      (0 .. 1020)
 *     Cb[j][i] = clamp255((-cbr * Rs - cbg * Gs + ch * Bs + (128 << 18) + (1 << 17)) >> 18)
 *     Cr[j][i] = clamp255(( ch * Rs - crg * Gs - crb * Bs + (128 << 18) + (1 << 17)) >> 18)
 * with Cb[j][i], Cr[j][i] = UV[j][2 * i], UV[j][2 * i + 1].  Each chroma sample is the mean of its 2 x 2 texels with one
 * rounding, the counterpart of the encode side's replication; no filtering reaches across samples, so a 4 x 4 block gives
 * exactly 4 x 4 Y samples and 2 x 2 pairs.  The coefficients are the standards' exact rationals times 65536 -- Kr, Kb =
 * 0.299, 0.114 (BT601) or 0.2126, 0.0722 (BT709); Limited scales luma by 219/255 and chroma by 224/255 -- rounded to
 * nearest, except one per row that is chosen by subtraction so that the row sums are exact: yg = round(65536 * sy) - yr -
 * yb, cbg = ch - cbr, crg = ch - crb:
 *     matrix, range        yr     yg    yb    cbr    cbg     ch    crg   crb   lo
 *     BT601  Limited    16829  33039  6416   9714  19070  28784  24103  4681   16
 *     BT601  Full       19595  38470  7471  11058  21710  32768  27439  5329    0
 *     BT709  Limited    11966  40254  4064   6596  22188  28784  26145  2639   16
 *     BT709  Full       13933  46871  4732   7509  25259  32768  29763  3005    0
 * Greys give Cb = Cr = 128 exactly; white and black give 235 / 16 (Limited) or 255 / 0 (Full).  The chroma accumulators
 * stay within 0 .. 2^26; Full range reaches 256 before the clamp, so the clamp is part of the definition.  Over all 2^24
 * colours with four equal texels every sample is within 0.5021 of the exact real value, and RGB -> this definition ->
 * HapGpuCompressNV12's comes back within 1, 1, 2 (Limited) and 1, 1, 1 (Full) of R, G, B.  With four different texels
 * luma is per texel and keeps its bound; chroma, over every one of the 1021^3 sums (Rs, Gs, Bs), is within 0.5024 of the
 * exact chroma of the texels' exact mean.
 * textureFormat: RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; texture is host or device, under HapGpuDecompressRGBA's rules, and a
 * device texture is aligned to what a lane reads of a block row (its block << scaleLog2, at most 16 bytes).  width and
 * height are the texture's, multiples of 4 << scaleLog2; scaleLog2 0 to 2; at most 65535 output block rows.  Both planes
 * are in DEVICE memory; their addresses and both pitches are multiples of 4, what a lane stores per row; lumaRowBytes >=
 * W and chromaRowBytes >= W (W / 2 pairs).  Only the samples are written, nothing between rows.  Bad_Arguments, and
 * nothing written, for anything else: a NULL, host or misaligned plane, a matrix or range outside the enums, another
 * format, scaleLog2 above 2, a bad size or pitch.
 * Out of scope: Hap R (BC7), Hap HDR (BC6H) and Alpha-Only (RGTC1) sources; an A8 plane beside the NV12; P010 and other
 * 10/16-bit layouts, planar I420, 4:2:2 and 4:4:4; sited or filtered chroma, which needs neighbours across blocks;
 * rectangles; host planes. */
unsigned int HapGpuDecompressNV12(HapGpuContext *context,
                                  const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                  unsigned int width, unsigned int height, unsigned int scaleLog2,
                                  unsigned int matrix, unsigned int range,
                                  void *luma, unsigned long lumaRowBytes,
                                  void *chroma, unsigned long chromaRowBytes);

/* Frames in, NV12 video pictures out -- the way back of HapGpuEncodeFramesNV12: HapGpuDecodeFramesRGBA[Scaled] with the
 * pictures of HapGpuDecompressNV12 in place of RGBA8 ones.  lumaPlanes[f] and chromaPlanes[f] are frame f's Y plane and
 * its plane of interleaved Cb, Cr pairs, both in DEVICE memory, lumaRowBytes and chromaRowBytes shared by all frames;
 * the pictures are W x H = (width >> scaleLog2) x (height >> scaleLog2), width and height being the FRAMES' geometry.
 * The definition is HapGpuDecompressNV12's, with d the RGBA8 picture HapGpuDecodeFramesRGBA (scaleLog2 0) or
 * HapGpuDecodeFramesRGBAScaled (1, 2) writes for the frame with the same textureCount and flags, alpha ignored, in
 * 32-bit integers:
 *     Y[y][x]  = lo + ((yr * R + yg * G + yb * B + 32768) >> 16)      of texel d(x, y)
 *     Cb[j][i] = clamp255((-cbr * Rs - cbg * Gs + ch * Bs + (128 << 18) + (1 << 17)) >> 18)
 *     Cr[j][i] = clamp255(( ch * Rs - crg * Gs - crb * Bs + (128 << 18) + (1 << 17)) >> 18)
 * Rs, Gs, Bs being the sums over the four texels d(2i..2i+1, 2j..2j+1) and the coefficients those of the table there
 * (matrix: HapGpuYCbCrMatrix, range: HapGpuYCbCrRange).  No RGBA8 picture ever exists: per Hap Q block 16 bytes are read
 * and 24 written at full size, where decoding to RGBA8 and converting with a tensor library moves 16 + 64 + 64 + 24.
 * Frames: Hap, Hap Alpha, Hap Q, and Hap Q Alpha with textureCount 2; the alpha plane is never block-decoded.  Mixed
 * batches (one block-decode launch per format present), slicing, the second-stage flags and results[f] are
 * HapGpuDecodeFramesRGBA's; HAPGPU_DECODE_BPTC_PICTURES is ignored.  Plane addresses and both pitches are multiples of
 * 4; lumaRowBytes >= W and chromaRowBytes >= W; width and height multiples of 4 << scaleLog2; scaleLog2 0 to 2; at most
 * 65535 output block rows.  Only the samples are written, nothing between rows.
 * A broken frame (HapDecode's code), a frame of another format or geometry, or a frame either of whose planes is NULL, in
 * host memory or misaligned (Bad_Arguments) fails alone: its planes are left untouched and the other frames are
 * decoded.  The function's result is the first failure.  Bad_Arguments for the whole call -- every results[f] set,
 * nothing written, no device touched -- for a NULL array, scaleLog2 above 2, a width or height that is no multiple of
 * 4 << scaleLog2, a pitch that is no multiple of 4 or below W, more than 65535 output block rows, a textureCount other
 * than 1 or 2, or a matrix or range outside the enums.  A context between a ...Begin and HapGpuEncodeFramesFinish:
 * Internal_Error.
 * Out of scope: Hap R (BC7), Hap HDR (BC6H) and Alpha-Only (RGTC1) sources; an A8 plane beside the NV12; P010 and other
 * 10/16-bit layouts, planar I420, 4:2:2 and 4:4:4; sited or filtered chroma, which needs neighbours across blocks;
 * rectangles; host planes; ...OnDevices and ...Sequence forms of this call. */
unsigned int HapGpuDecodeFramesNV12(HapGpuContext *context, unsigned int frameCount,
                                    const void *const *inputBuffers,
                                    const unsigned long *inputBuffersBytes,
                                    unsigned int textureCount,
                                    void *const *lumaPlanes, unsigned long lumaRowBytes,
                                    void *const *chromaPlanes, unsigned long chromaRowBytes,
                                    unsigned int matrix, unsigned int range,
                                    unsigned int width, unsigned int height, unsigned int scaleLog2,
                                    unsigned int *results,
                                    unsigned int flags);

/* Hap HDR frames in, RGBA16F pictures out: HapGpuDecodeFramesRGBA for frames of one BC6H texture (unsigned or
 * signed; a batch may mix the two: one block-decode launch per signedness present), pictures as
 * HapGpuDecompressRGBAHalf makes them (rowBytes a multiple of 16, at least width * 8; device pictures 16-byte
 * aligned; host or device; host pictures with longer rows are written row by row).  flags: the decode flags, as for
 * HapGpuDecodeFrameTextures.  results[f]: HapDecode's code for the frame; Bad_Arguments for a frame of another
 * format (Hap, Hap Q, Hap R ...) or geometry, whose picture is left untouched. */
unsigned int HapGpuDecodeFramesRGBAHalf(HapGpuContext *context, unsigned int frameCount,
                                        const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                        void *const *rgbaHalfFrames,
                                        unsigned int width, unsigned int height, unsigned long rowBytes,
                                        unsigned int *results, unsigned int flags);

/* Hap Alpha-Only frames in, A8 pictures out: HapGpuDecodeFramesRGBA for frames of one A_RGTC1 texture, pictures as
 * HapGpuDecompressAlpha makes them (the rules of the ...Alpha calls above: rowBytes a multiple of 4, at least width;
 * device pictures 4-byte aligned; host or device; host pictures with longer rows are written row by row).  The batch
 * is worked through in slices like the other roads.  flags: the decode flags, as for HapGpuDecodeFrameTextures.
 * results[f]: HapDecode's code for the frame (a broken frame: Bad_Frame); Bad_Arguments for a frame of another format
 * (Hap, Hap Q, Hap Q Alpha ...) or geometry, whose picture is left untouched.  The function's result is the first
 * failure. */
unsigned int HapGpuDecodeFramesAlpha(HapGpuContext *context, unsigned int frameCount,
                                     const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                     void *const *alphaFrames,
                                     unsigned int width, unsigned int height, unsigned long rowBytes,
                                     unsigned int *results, unsigned int flags);

/* --- frames to frames: another flavour or size without a picture in between ------------------- */

/* One texture (alphaTexture != NULL: + its RGTC1 alpha plane, Hap Q Alpha's second texture) in, `count` textures of
 * (width >> scaleLog2) x (height >> scaleLog2) out: outputs[i] is byte for byte what HapGpuCompressRGBA(...,
 * outputFormats[i], ...) makes of the picture HapGpuDecompressRGBA (scaleLog2 0) or HapGpuDecompressRGBAScaled (1, 2)
 * writes for the source -- made by one kernel that decodes a block's texels and encodes them again in registers; no such
 * picture ever exists.  So a source without alpha gives A = 255, RGB_DXT1 output drops alpha, and YCoCg is converted
 * back to RGB and forward again.  Sources: RGB_DXT1, RGBA_DXT5, YCoCg_DXT5.  Outputs, count 1: RGB_DXT1, RGBA_DXT5 or
 * YCoCg_DXT5; count 2: YCoCg_DXT5 then A_RGTC1 (Hap Q Alpha, both textures in one pass).  The one exception: the
 * destination set the source is already (the same format, with a plane exactly when count is 2) at scaleLog2 0 is copied,
 * not encoded again -- no generation loss.
 * width and height are the SOURCE's, multiples of 4 << scaleLog2, scaleLog2 0 to 2; at most 65535 output block rows.
 * Buffers may be host or device; a device source is aligned to its block << scaleLog2 (at most 16 bytes; the plane
 * likewise, from 8), device outputs to their blocks.  outputsBytesUsed may be NULL.  Bad_Arguments for anything else
 * (nothing is written); Buffer_Too_Small for an output shorter than its texture.
 * Out of scope: BC7 and BC6H as a source or destination of the kernel, A8 and RGBA16F, rectangles. */
unsigned int HapGpuTranscodeTexture(HapGpuContext *context,
                                    const void *texture, unsigned long textureBytes, unsigned int textureFormat,
                                    const void *alphaTexture, unsigned long alphaTextureBytes,
                                    unsigned int width, unsigned int height, unsigned int scaleLog2,
                                    unsigned int count, const unsigned int *outputFormats,
                                    void *const *outputs, const unsigned long *outputsBytes,
                                    unsigned long *outputsBytesUsed);

/* Frames in, frames of other texture formats or of half / quarter size out, in one call and without a picture in
 * between: a Hap Q master to quarter-size Hap proxies, Hap Alpha to Hap Q Alpha, Hap Q to Hap, another encoder's frames
 * to frames with this library's fragment table.
 * The definition: a transcoded frame is byte for byte the frame HapGpuEncodeFramesRGBA(..., width >> scaleLog2,
 * height >> scaleLog2, ..., count, textureFormats, compressors, chunkCounts, ..., encodeFlags) makes of the picture that
 * HapGpuDecodeFramesRGBA (scaleLog2 1 or 2: HapGpuDecodeFramesRGBAScaled) writes for the source frame with
 * sourceTextureCount and decodeFlags.  No such picture ever exists: the textures go from the decoder's second stage
 * through HapGpuTranscodeTexture's kernel (one launch per source format present: a batch may mix flavours) to the
 * encoder's second stage, 16 + 16 bytes of traffic per block for Hap Q where the two calls move 16 + 64 + 64 + 16, and
 * the host is waited for twice per slice of frames: for the decode's results and at the end.
 * width and height are the SOURCE frames', multiples of 4 << scaleLog2; scaleLog2 0 to 2; sources are what
 * HapGpuDecodeFramesRGBA takes without HAPGPU_DECODE_BPTC_PICTURES (Hap, Hap Alpha, Hap Q, Hap Q Alpha);
 * destinations, count 1: RGB_DXT1, RGBA_DXT5 or YCoCg_DXT5; count 2: YCoCg_DXT5 then A_RGTC1.
 * Pass-through, the one exception to the definition: a frame whose own textures (sourceTextureCount of them, in order)
 * have the formats textureFormats, at scaleLog2 0, is not encoded again -- its textures go to the second stage as they
 * are, without generation loss.  That holds for every format HapEncode accepts, RGBA_BPTC_UNORM, the BC6H formats and
 * a lone A_RGTC1 included, and is how another encoder's frames get a fragment table or fine chunks.  A destination set
 * outside the four above is therefore legal at scaleLog2 0 only, and a frame that cannot pass through it is
 * Bad_Arguments alone.
 * The second stage, frame layout, chunk-count limiting, store-raw decisions, outputBuffersBytes / Buffer_Too_Small and
 * encodeFlags are HapGpuEncodeFrames' (HAPGPU_ENCODE_BPTC_BLOCKS and HAPGPU_ENCODE_REFINE_ENDPOINTS are ignored: the
 * destination blocks stay as the default encode would make them); decodeFlags are
 * HapGpuDecodeFrameTextures'.  Buffers may be host or device.
 * results[f]: where the decode of frame f fails, the decode's code -- HapDecode's (a broken frame: Bad_Frame), or
 * Bad_Arguments for a frame of another geometry or format; else the encode's code (a NULL output: Bad_Arguments, a short
 * one: Buffer_Too_Small).  A failed frame's output buffer is not written.  The function's result is the first failure.
 * Bad_Arguments for the whole call -- every results[f] set, nothing written -- for a NULL array, scaleLog2 above 2, a
 * width or height that is no multiple of 4 << scaleLog2, sourceTextureCount or count other than 1 or 2, a destination
 * set that is illegal at that scale, and what HapGpuEncodeFrames refuses of textureFormats, compressors and
 * chunkCounts.  A context between HapGpuEncodeFramesRGBABegin and HapGpuEncodeFramesFinish: Internal_Error.
 * Out of scope: BC7 and BC6H as a source or destination of the re-encoding kernel, A8 and RGBA16F pictures'
 * flavours (Hap Alpha-Only, Hap HDR) other than by pass-through, rectangles, and ...Begin, ...OnDevices and
 * ...Sequence forms of this call. */
unsigned int HapGpuTranscodeFrames(HapGpuContext *context, unsigned int frameCount,
                                   const void *const *inputBuffers, const unsigned long *inputBuffersBytes,
                                   unsigned int sourceTextureCount,
                                   unsigned int width, unsigned int height, unsigned int scaleLog2,
                                   unsigned int count, const unsigned int *textureFormats,
                                   const unsigned int *compressors, const unsigned int *chunkCounts,
                                   void *const *outputBuffers, const unsigned long *outputBuffersBytes,
                                   unsigned long *outputBuffersBytesUsed, unsigned int *results,
                                   unsigned int decodeFlags, unsigned int encodeFlags);

/* --- one batch over several GPUs: independent frames per GPU ------------------- */

/* HapGpuEncodeFramesRGBA / HapGpuEncodeFrames / HapGpuDecodeFrames with the batch dealt out over `contextCount`
 * contexts -- normally one per GPU of the node (HapGpuCreate(device, ...)): frame f is worked on by context
 * f mod contextCount, each context on a host thread of its own, no data moves between devices and there is no
 * collective (frames are independent; a frame's buffers should live on the device that works on it, else they are
 * reached over the fabric or staged like any host pointer).  Arguments, per-frame results and the function result are
 * those of the single-context call, and so are the bytes written, whatever contextCount is (tests: 2, 3 and 8
 * contexts).  The contexts may share a device.  What the reference's clients do with a pool of threads calling
 * HapEncode / HapDecode frame by frame (hap.h:98-140). */
unsigned int HapGpuEncodeFramesRGBAOnDevices(HapGpuContext *const *contexts, unsigned int contextCount,
                                             unsigned int frameCount,
                                             const void *const *rgbaFrames,
                                             unsigned int width, unsigned int height, unsigned long rowBytes,
                                             unsigned int count,
                                             const unsigned int *textureFormats,
                                             const unsigned int *compressors,
                                             const unsigned int *chunkCounts,
                                             void *const *outputBuffers,
                                             const unsigned long *outputBuffersBytes,
                                             unsigned long *outputBuffersBytesUsed,
                                             unsigned int *results,
                                             unsigned int flags);
unsigned int HapGpuEncodeFramesOnDevices(HapGpuContext *const *contexts, unsigned int contextCount,
                                         unsigned int frameCount, unsigned int count,
                                         const void *const *inputBuffers,
                                         const unsigned long *inputBuffersBytes,
                                         const unsigned int *textureFormats,
                                         const unsigned int *compressors,
                                         const unsigned int *chunkCounts,
                                         void *const *outputBuffers,
                                         const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed,
                                         unsigned int *results,
                                         unsigned int flags);
unsigned int HapGpuDecodeFramesOnDevices(HapGpuContext *const *contexts, unsigned int contextCount,
                                         unsigned int frameCount,
                                         const void *const *inputBuffers,
                                         const unsigned long *inputBuffersBytes,
                                         unsigned int index,
                                         void *const *outputBuffers,
                                         const unsigned long *outputBuffersBytes,
                                         unsigned long *outputBuffersBytesUsed,
                                         unsigned int *outputTextureFormats,
                                         unsigned int *results,
                                         unsigned int flags);

/* --- one frame split over several GPUs by chunk groups ------------------------ */

/* HapDecode restricted to the chunks [firstChunk, firstChunk + chunkCount) of texture `index`:
 * outputBuffer is laid out as the WHOLE texture and only the group's byte range is written; the
 * rest is left untouched.  This is what a HapDecodeCallback that runs a subset of the work items
 * obtains from HapDecode (reference hap.h:113-130, hap.c:852-862); like there, frames that are
 * not chunked or have a single chunk are decoded completely.  *outputBufferBytesUsed is the
 * size of the whole texture.  inputBuffer / outputBuffer: host or device. */
unsigned int HapGpuDecodeChunkGroup(HapGpuContext *context,
                                    const void *inputBuffer, unsigned long inputBufferBytes,
                                    unsigned int index,
                                    unsigned int firstChunk, unsigned int chunkCount,
                                    void *outputBuffer, unsigned long outputBufferBytes,
                                    unsigned long *outputBufferBytesUsed,
                                    unsigned int *outputBufferTextureFormat);

/* Where each chunk of texture `index` lands in the decoded texture: the running sum of decoded
 * chunk sizes that the reference decoder builds (hap.c:794-838).  Writes chunkCount + 1 offsets
 * (the last one is the decoded size of the texture); Buffer_Too_Small if capacity is less.
 * Needs no GPU (inputBuffer: host or device). */
unsigned int HapGpuGetFrameTextureChunkLayout(const void *inputBuffer, unsigned long inputBufferBytes,
                                              unsigned int index, unsigned int capacity,
                                              unsigned long *decodedOffsets, unsigned int *chunkCount);

/* Joins frames that each hold one contiguous group of the chunks of the same texture(s) -- e.g.
 * bands of block rows encoded on different GPUs -- into one ordinary Hap frame whose chunk list
 * is the concatenation of the groups' lists, in the order given (frame layout: reference
 * hap.c:430-442, 562-598).  All groups must have the same texture count and formats.  A group
 * stored without chunks contributes a single chunk; if no chunk of a texture is compressed the
 * texture is written as a plain uncompressed section, as the reference does when Snappy gains
 * nothing (hap.c:478-495).  Fragment-size sections (type 0x46) are carried over when every
 * group has a compatible one.  Host pointers only; needs no GPU.
 * outputBufferBytes: the sum of the groups' sizes plus 64 always suffices. */
unsigned int HapGpuJoinChunkGroups(unsigned int groupCount,
                                   const void *const *groupFrames,
                                   const unsigned long *groupFramesBytes,
                                   void *outputBuffer, unsigned long outputBufferBytes,
                                   unsigned long *outputBufferBytesUsed);

/* The same join for group frames AND output in HIP device memory of `context`'s device (band frames that arrived
 * over xGMI): the groups' headers and tables are read through the host, the joined frame's headers are made there and
 * uploaded, every table and payload byte moves device to device.  Version-3 fragment tables (group tables) are
 * carried over by both joins when every group has one with the same block layout, so a joined frame decodes through
 * the block-per-lane kernel like its parts.  Bad_Arguments for host pointers. */
unsigned int HapGpuJoinChunkGroupsDevice(HapGpuContext *context, unsigned int groupCount,
                                         const void *const *groupFrames,
                                         const unsigned long *groupFramesBytes,
                                         void *outputBuffer, unsigned long outputBufferBytes,
                                         unsigned long *outputBufferBytesUsed);

/* --- measurement hooks (used by bench.py; see DESIGN.md "Measurement") --- */

/* Kernel classes whose launches are bracketed with HIP events on the
 * context's stream while profiling is enabled. */
enum HapGpuKernelClass {
    HapGpuKernel_BlockEncode = 0,
    HapGpuKernel_SnappyCompress = 1,
    HapGpuKernel_FramePack = 2,
    HapGpuKernel_FrameGather = 3,
    HapGpuKernel_DecodePlan = 4,
    HapGpuKernel_SnappyDecode = 5,
    HapGpuKernel_BlockDecode = 6,
    HapGpuKernel_BlockScan = 7,       /* finding the 64 KiB blocks of other encoders' Snappy streams */
    HapGpuKernel_EncodeFused = 8,     /* RGBA -> blocks -> Snappy fragments in one kernel (the calls that start from pictures) */
    HapGpuKernel_ClassCount = 9
};

/* enable != 0: record a start/stop event pair around every kernel launch. */
unsigned int HapGpuSetProfiling(HapGpuContext *context, unsigned int enable);
/* Drains recorded events: launches[k] and milliseconds[k] are ADDED to for every class k < classCount (the entries
 * the caller's arrays have; pass HapGpuKernel_ClassCount of the header the client was built with: a later library may
 * know more classes, and drops what the arrays have no room for). Synchronises. */
unsigned int HapGpuCollectProfileN(HapGpuContext *context, unsigned int classCount, unsigned long *launches, double *milliseconds);
/* The same for arrays of EIGHT entries (classes 0..7: the signature of the first release, which had no count). */
unsigned int HapGpuCollectProfile(HapGpuContext *context, unsigned long *launches, double *milliseconds);
/* Wall-clock bracket on the context's stream with HIP events. */
unsigned int HapGpuTimerStart(HapGpuContext *context);
unsigned int HapGpuTimerStop(HapGpuContext *context, double *milliseconds);

#ifdef __cplusplus
}
#endif

#endif /* HAP_AMD_HAP_GPU_H */

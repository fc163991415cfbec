"""BC7 (BPTC, RGBA_BPTC_UNORM) on the CPU: a scalar reference decoder, a seeded block generator and Pillow's decoder.

The decoder is written from the BPTC definition the Hap spec cites for Hap R (OpenGL ARB_texture_compression_bptc;
the same BC7 section is in the Khronos Data Format Specification): a 128-bit block read least significant bit first,
the mode as a unary prefix, then partition / rotation / index-selection fields, the colour endpoints channel by channel,
the alpha endpoints, the p-bits and the indices.  It reads one field at a time and is meant to be read, not to be fast;
every GPU test compares against it.

The generator draws from splitmix64 written out below (not numpy's generator), so the block sets -- and the digests
tests/golden/bptc_pillow.json records for them -- depend on nothing but this file.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------- the BPTC tables
# Per mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits, endpoint p-bits,
# shared p-bits, index bits, second index bits.
MODES = [
    (3, 4, 0, 0, 4, 0, 1, 0, 3, 0),
    (2, 6, 0, 0, 6, 0, 0, 1, 3, 0),
    (3, 6, 0, 0, 5, 0, 0, 0, 2, 0),
    (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
    (1, 0, 2, 1, 5, 6, 0, 0, 2, 3),
    (1, 0, 2, 0, 7, 8, 0, 0, 2, 2),
    (1, 0, 0, 0, 7, 7, 1, 0, 4, 0),
    (2, 6, 0, 0, 5, 5, 1, 0, 2, 0),
]

# two subsets: bit i of the mask = subset of texel i (texels in row-major order)
PARTITIONS_2 = [
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80,
    0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE,
    0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A,
    0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C,
    0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22,
]

# three subsets: bits 2i..2i+1 = subset of texel i
PARTITIONS_3 = [
    0xAA685050, 0x6A5A5040, 0x5A5A4200, 0x5450A0A8, 0xA5A50000, 0xA0A05050, 0x5555A0A0, 0x5A5A5050,
    0xAA550000, 0xAA555500, 0xAAAA5500, 0x90909090, 0x94949494, 0xA4A4A4A4, 0xA9A59450, 0x2A0A4250,
    0xA5945040, 0x0A425054, 0xA5A5A500, 0x55A0A0A0, 0xA8A85454, 0x6A6A4040, 0xA4A45000, 0x1A1A0500,
    0x0050A4A4, 0xAAA59090, 0x14696914, 0x69691400, 0xA08585A0, 0xAA821414, 0x50A4A450, 0x6A5A0200,
    0xA9A58000, 0x5090A0A8, 0xA8A09050, 0x24242424, 0x00AA5500, 0x24924924, 0x24499224, 0x50A50A50,
    0x500AA550, 0xAAAA4444, 0x66660000, 0xA5A0A5A0, 0x50A050A0, 0x69286928, 0x44AAAA44, 0x66666600,
    0xAA444444, 0x54A854A8, 0x95809580, 0x96969600, 0xA85454A8, 0x80959580, 0xAA141414, 0x96960000,
    0xAAAA1414, 0xA05050A0, 0xA0A5A5A0, 0x96000000, 0x40804080, 0xA9A8A9A8, 0xAAAAAA44, 0x2A4A5254,
]

# anchor texel of subset 1 (two subsets), of subsets 1 and 2 (three subsets); subset 0's anchor is texel 0
ANCHORS_2 = [
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6,
    6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15,
]
ANCHORS_3A = [
    3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3,
    3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
    8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15,
    3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3,
]
ANCHORS_3B = [
    15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8,
    15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
    15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8,
    15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8,
]

WEIGHTS = {
    2: [0, 21, 43, 64],
    3: [0, 9, 18, 27, 37, 46, 55, 64],
    4: [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64],
}


def subset_of(subsets, partition, texel):
    if subsets == 1:
        return 0
    if subsets == 2:
        return (PARTITIONS_2[partition] >> texel) & 1
    return (PARTITIONS_3[partition] >> (2 * texel)) & 3


def anchors_of(subsets, partition):
    if subsets == 1:
        return [0]
    if subsets == 2:
        return [0, ANCHORS_2[partition]]
    return [0, ANCHORS_3A[partition], ANCHORS_3B[partition]]


# ---------------------------------------------------------------------------------------------------- the decoder
class _Bits:
    def __init__(self, block):
        self.v = int.from_bytes(bytes(block), "little")
        self.pos = 0

    def take(self, n):
        r = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return r


def _unquantize(value, bits):
    """value of `bits` bits (p-bit appended) -> 8 bits: the MSB moved to bit 7, the top bits copied into the low bits."""
    v = value << (8 - bits)
    return v | (v >> bits)


def _interpolate(e0, e1, w):
    return ((64 - w) * e0 + w * e1 + 32) >> 6


def decode_block(block):
    """16 bytes -> [16][4] RGBA8 texels (row-major).  Blocks without a mode bit in the first byte are reserved and
    decode to (0, 0, 0, 0)."""
    bits = _Bits(block)
    mode = 0
    while mode < 8 and bits.take(1) == 0:
        mode += 1
    if mode == 8:
        return [[0, 0, 0, 0] for _ in range(16)]
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    partition = bits.take(pb)
    rotation = bits.take(rb)
    index_selection = bits.take(isb)
    # endpoints: channel by channel (R, G, B, then A), within a channel subset by subset, two endpoints per subset
    ends = [[0, 0, 0, 0] for _ in range(2 * ns)]
    for c in range(3):
        for e in range(2 * ns):
            ends[e][c] = bits.take(cb)
    for e in range(2 * ns):
        ends[e][3] = bits.take(ab) if ab else 0
    if epb:
        pbits = [bits.take(1) for _ in range(2 * ns)]
    elif spb:
        shared = [bits.take(1) for _ in range(ns)]
        pbits = [shared[e // 2] for e in range(2 * ns)]
    else:
        pbits = None
    for e in range(2 * ns):
        for c in range(4):
            width = cb if c < 3 else ab
            if c == 3 and ab == 0:
                ends[e][c] = 255
                continue
            if pbits is not None:
                ends[e][c] = _unquantize((ends[e][c] << 1) | pbits[e], width + 1)
            else:
                ends[e][c] = _unquantize(ends[e][c], width)
    anchors = anchors_of(ns, partition)
    primary = []
    for t in range(16):
        primary.append(bits.take(ib - 1 if t in anchors else ib))
    secondary = [bits.take(ib2 - 1 if t == 0 else ib2) for t in range(16)] if ib2 else None
    assert bits.pos == 128, (mode, bits.pos)
    out = []
    for t in range(16):
        s = subset_of(ns, partition, t)
        e0, e1 = ends[2 * s], ends[2 * s + 1]
        if secondary is None:
            ci, cbits, ai, abits = primary[t], ib, primary[t], ib
        elif index_selection == 0:
            ci, cbits, ai, abits = primary[t], ib, secondary[t], ib2
        else:
            ci, cbits, ai, abits = secondary[t], ib2, primary[t], ib
        px = [_interpolate(e0[c], e1[c], WEIGHTS[cbits][ci]) for c in range(3)]
        px.append(_interpolate(e0[3], e1[3], WEIGHTS[abits][ai]))
        if rotation:
            px[rotation - 1], px[3] = px[3], px[rotation - 1]
        out.append(px)
    return out


def decode(blocks, w, h):
    """BC7 texture (blocks row-major, w and h multiples of 4) -> uint8 [h, w, 4]."""
    data = bytes(blocks)
    bw = w // 4
    assert len(data) >= (w // 4) * (h // 4) * 16
    img = np.zeros((h, w, 4), dtype=np.uint8)
    cache = {}
    for b in range((w // 4) * (h // 4)):
        blk = data[16 * b: 16 * b + 16]
        px = cache.get(blk)
        if px is None:
            px = cache[blk] = np.array(decode_block(blk), dtype=np.uint8).reshape(4, 4, 4)
        by, bx = divmod(b, bw)
        img[4 * by: 4 * by + 4, 4 * bx: 4 * bx + 4] = px
    return img


def reserved_mask(blocks, w, h):
    """bool [h, w]: texels of reserved blocks (first byte 0)."""
    data = np.frombuffer(bytes(blocks), dtype=np.uint8)[: (w // 4) * (h // 4) * 16].reshape(h // 4, w // 4, 16)
    m = data[..., 0] == 0
    return np.repeat(np.repeat(m, 4, axis=0), 4, axis=1)


def pillow_bc7_decode(blocks, w, h):
    """Pillow's BC7 decoder (third-party code).  It gives (0, 0, 0, 255) for reserved blocks where the specification
    and D3D hardware give (0, 0, 0, 0): comparisons leave those texels out (reserved_mask)."""
    from PIL import Image
    img = Image.frombuffer("RGBA", (w, h), bytes(blocks)[: (w // 4) * (h // 4) * 16], "bcn", (7,))
    return np.asarray(img, dtype=np.uint8).reshape(h, w, 4)


# ---------------------------------------------------------------------------------------------------- the generator
_M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & _M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def bits(self, n):
        v = 0
        got = 0
        while got < n:
            v |= self.next() << got
            got += 64
        return v & ((1 << n) - 1)


def _header(mode, partition=0, rotation=0, index_selection=0):
    """(value, bits) of a mode's leading fields."""
    ns, pb, rb, isb = MODES[mode][:4]
    v = 1 << mode
    pos = mode + 1
    v |= partition << pos
    pos += pb
    v |= rotation << pos
    pos += rb
    v |= index_selection << pos
    pos += isb
    return v, pos


def make_block(mode, rng, partition=0, rotation=0, index_selection=0, saturate=None):
    """One mode-`mode` block with the given leading fields and random (or, saturate = 0 / 1, all-zero / all-one)
    endpoints and p-bits; indices random."""
    v, pos = _header(mode, partition, rotation, index_selection)
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    end_bits = 2 * ns * (3 * cb + ab) + (2 * ns if epb else ns if spb else 0)
    if saturate is None:
        ends = rng.bits(end_bits)
    else:
        ends = (1 << end_bits) - 1 if saturate else 0
    v |= ends << pos
    pos += end_bits
    v |= rng.bits(128 - pos) << pos
    return v.to_bytes(16, "little")


def block_sets(seed=0x42433731):
    """name -> bytes of blocks: one set per mode (every partition, rotation and index selection of the mode, saturated
    endpoints and p-bits, random fields), a set of reserved blocks, and a mixed set of all of them shuffled."""
    rng = SplitMix64(seed)
    sets = {}
    for mode in range(8):
        ns, pb, rb, isb = MODES[mode][:4]
        out = []
        for partition in range(1 << pb):
            for rotation in range(1 << rb):
                for sel in range(1 << isb):
                    for sat in (None, None, None, 0, 1):
                        out.append(make_block(mode, rng, partition, rotation, sel, sat))
        while len(out) % 16:
            out.append(make_block(mode, rng, rng.bits(pb), rng.bits(rb), rng.bits(isb)))
        sets["mode%d" % mode] = b"".join(out)
    reserved = []
    for i in range(16):
        reserved.append(bytes([0]) + rng.bits(120).to_bytes(15, "little") if i else bytes(16))
    sets["reserved"] = b"".join(reserved)
    allb = [b for name in sorted(sets) for b in (sets[name][i:i + 16] for i in range(0, len(sets[name]), 16))]
    for i in range(len(allb) - 1, 0, -1):                  # Fisher-Yates with the same generator
        j = rng.next() % (i + 1)
        allb[i], allb[j] = allb[j], allb[i]
    while len(allb) % 16:
        allb.append(allb[len(allb) % 7])
    sets["mixed"] = b"".join(allb)
    return sets


def random_blocks(n, seed):
    """n blocks of uniformly random bits (every mode appears, mode 0 most often, about 1 in 256 reserved)."""
    rng = SplitMix64(seed)
    return b"".join(rng.bits(128).to_bytes(16, "little") for _ in range(n))


def geometry(nblocks):
    """(w, h) of a picture 16 blocks wide holding nblocks blocks (nblocks a multiple of 16)."""
    assert nblocks % 16 == 0
    return 64, 4 * (nblocks // 16)

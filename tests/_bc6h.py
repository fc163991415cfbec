"""BC6H (BPTC float, RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT) on the CPU: a scalar reference decoder, a seeded
block generator and Pillow's decoder.

The decoder is written from the BC6H section of ARB_texture_compression_bptc (the same text is in the Khronos Data
Format Specification): a 128-bit block read least significant bit first; a 2-bit mode (low bits 00 or 01) or a 5-bit
one; the endpoint bits of the mode scattered over the header in the order of the mode's layout (some runs stored
bit-reversed); a 5-bit partition for two-region modes; the indices.  Transformed modes store a base endpoint and
deltas from it.  Endpoints are unquantised to 16 bits, interpolated with the 3-bit or 4-bit BPTC weights and finished
to a half-float bit pattern (x 31/64 unsigned, x 31/32 with the sign in bit 15 signed).  Reserved modes give RGB 0.
It reads one field at a time and is meant to be read, not to be fast; every GPU test compares against it.

Output: uint16 [h, w, 4] half-float bit patterns, alpha always 1.0 (0x3C00).  The generator is _bptc's splitmix64, so
the block sets -- and the digests tests/golden/bc6h_pillow.json records for them -- depend on nothing but these files.
"""
import numpy as np

from _bptc import ANCHORS_2, PARTITIONS_2, WEIGHTS, SplitMix64

# ---------------------------------------------------------------------------------------------------- the BC6H tables
# The twelve endpoint fields: w, x of region 0 and y, z of region 1, per channel.
FIELDS = ["rw", "gw", "bw", "rx", "gx", "bx", "ry", "gy", "by", "rz", "gz", "bz"]

# Per mode, in the order of the specification's table: mode value, regions, transformed, endpoint precision, delta
# precision (R, G, B), and the header layout after the mode bits -- runs "f[hi:lo]" stored lowest bit first, "f[lo:hi]"
# (lo < hi) stored reversed, "f[b]" one bit.  Two-region layouts end at bit 77, where the partition starts.
MODES = [
    (0x00, 2, True, 10, (5, 5, 5),
     "gy[4] by[4] bz[4] rw[9:0] gw[9:0] bw[9:0] rx[4:0] gz[4] gy[3:0] gx[4:0] bz[0] gz[3:0] bx[4:0] bz[1] by[3:0] "
     "ry[4:0] bz[2] rz[4:0] bz[3]"),
    (0x01, 2, True, 7, (6, 6, 6),
     "gy[5] gz[4] gz[5] rw[6:0] bz[0] bz[1] by[4] gw[6:0] by[5] bz[2] gy[4] bw[6:0] bz[3] bz[5] bz[4] rx[5:0] "
     "gy[3:0] gx[5:0] gz[3:0] bx[5:0] by[3:0] ry[5:0] rz[5:0]"),
    (0x02, 2, True, 11, (5, 4, 4),
     "rw[9:0] gw[9:0] bw[9:0] rx[4:0] rw[10] gy[3:0] gx[3:0] gw[10] bz[0] gz[3:0] bx[3:0] bw[10] bz[1] by[3:0] "
     "ry[4:0] bz[2] rz[4:0] bz[3]"),
    (0x06, 2, True, 11, (4, 5, 4),
     "rw[9:0] gw[9:0] bw[9:0] rx[3:0] rw[10] gz[4] gy[3:0] gx[4:0] gw[10] gz[3:0] bx[3:0] bw[10] bz[1] by[3:0] "
     "ry[3:0] bz[0] bz[2] rz[3:0] gy[4] bz[3]"),
    (0x0A, 2, True, 11, (4, 4, 5),
     "rw[9:0] gw[9:0] bw[9:0] rx[3:0] rw[10] by[4] gy[3:0] gx[3:0] gw[10] bz[0] gz[3:0] bx[4:0] bw[10] by[3:0] "
     "ry[3:0] bz[1] bz[2] rz[3:0] bz[4] bz[3]"),
    (0x0E, 2, True, 9, (5, 5, 5),
     "rw[8:0] by[4] gw[8:0] gy[4] bw[8:0] bz[4] rx[4:0] gz[4] gy[3:0] gx[4:0] bz[0] gz[3:0] bx[4:0] bz[1] by[3:0] "
     "ry[4:0] bz[2] rz[4:0] bz[3]"),
    (0x12, 2, True, 8, (6, 5, 5),
     "rw[7:0] gz[4] by[4] gw[7:0] bz[2] gy[4] bw[7:0] bz[3] bz[4] rx[5:0] gy[3:0] gx[4:0] bz[0] gz[3:0] bx[4:0] "
     "bz[1] by[3:0] ry[5:0] rz[5:0]"),
    (0x16, 2, True, 8, (5, 6, 5),
     "rw[7:0] bz[0] by[4] gw[7:0] gy[5] gy[4] bw[7:0] gz[5] bz[4] rx[4:0] gz[4] gy[3:0] gx[5:0] gz[3:0] bx[4:0] "
     "bz[1] by[3:0] ry[4:0] bz[2] rz[4:0] bz[3]"),
    (0x1A, 2, True, 8, (5, 5, 6),
     "rw[7:0] bz[1] by[4] gw[7:0] by[5] gy[4] bw[7:0] bz[5] bz[4] rx[4:0] gz[4] gy[3:0] gx[4:0] bz[0] gz[3:0] "
     "bx[5:0] by[3:0] ry[4:0] bz[2] rz[4:0] bz[3]"),
    (0x1E, 2, False, 6, (6, 6, 6),
     "rw[5:0] gz[4] bz[0] bz[1] by[4] gw[5:0] gy[5] by[5] bz[2] gy[4] bw[5:0] gz[5] bz[3] bz[5] bz[4] rx[5:0] "
     "gy[3:0] gx[5:0] gz[3:0] bx[5:0] by[3:0] ry[5:0] rz[5:0]"),
    (0x03, 1, False, 10, (10, 10, 10),
     "rw[9:0] gw[9:0] bw[9:0] rx[9:0] gx[9:0] bx[9:0]"),
    (0x07, 1, True, 11, (9, 9, 9),
     "rw[9:0] gw[9:0] bw[9:0] rx[8:0] rw[10] gx[8:0] gw[10] bx[8:0] bw[10]"),
    (0x0B, 1, True, 12, (8, 8, 8),
     "rw[9:0] gw[9:0] bw[9:0] rx[7:0] rw[10:11] gx[7:0] gw[10:11] bx[7:0] bw[10:11]"),
    (0x0F, 1, True, 16, (4, 4, 4),
     "rw[9:0] gw[9:0] bw[9:0] rx[3:0] rw[10:15] gx[3:0] gw[10:15] bx[3:0] bw[10:15]"),
]
RESERVED = (0x13, 0x17, 0x1B, 0x1F)
MODE_OF_VALUE = {m[0]: i for i, m in enumerate(MODES)}


def layout(mode):
    """[(field, [endpoint bit of each block bit, in block order])] of mode index `mode` (0..13)."""
    out = []
    for tok in MODES[mode][5].split():
        name, rng = tok[:2], tok[3:-1]
        if ":" in rng:
            a, b = (int(x) for x in rng.split(":"))
            bits = list(range(b, a + 1)) if a > b else list(range(b, a - 1, -1))
        else:
            bits = [int(rng)]
        out.append((name, bits))
    return out


def mode_bits(value):
    return 2 if value < 2 else 5


def mode_index(block):
    """(mode index 0..13 or None for a reserved mode, mode value)."""
    v = bytes(block)[0]
    value = v & 3 if v & 3 < 2 else v & 0x1F
    return MODE_OF_VALUE.get(value), value


# ---------------------------------------------------------------------------------------------------- the decoder
def _sext(v, bits):
    return v - (1 << bits) if v & (1 << (bits - 1)) else v


def _unquantize(comp, prec, signed):
    """An endpoint of `prec` bits -> 16 bits (unsigned: 0..0xFFFF; signed: -0x7FFF..0x7FFF)."""
    if not signed:
        if prec >= 15 or comp == 0:
            return comp
        if comp == (1 << prec) - 1:
            return 0xFFFF
        return ((comp << 16) + 0x8000) >> prec
    if prec >= 16:
        return comp
    neg = comp < 0
    mag = -comp if neg else comp
    if mag == 0:
        unq = 0
    elif mag >= (1 << (prec - 1)) - 1:
        unq = 0x7FFF
    else:
        unq = ((mag << 15) + 0x4000) >> (prec - 1)
    return -unq if neg else unq


def _interpolate(a, b, w, rounding=32):
    return ((64 - w) * a + w * b + rounding) >> 6         # arithmetic shift: floor for negative sums


def _finish(v, signed):
    """An interpolated 16-bit value -> half-float bit pattern.  The sign comes from `v`: -1 gives 0x8000."""
    if not signed:
        return (v * 31) >> 6
    if v < 0:
        return 0x8000 | (((-v) * 31) >> 5)
    return (v * 31) >> 5


def fields(block):
    """name -> value of the endpoint fields of a non-reserved block, as stored (deltas not yet applied)."""
    mode, _value = mode_index(block)
    value, regions = MODES[mode][:2]
    v = int.from_bytes(bytes(block), "little")
    pos = mode_bits(value)
    e = dict.fromkeys(FIELDS, 0)
    for name, bits in layout(mode):
        for b in bits:
            e[name] |= ((v >> pos) & 1) << b
            pos += 1
    assert pos == (77 if regions == 2 else 65), (mode, pos)
    return e


def endpoints(block, signed):
    """(regions, partition, endpoint precision, [[R, G, B] of w, x, y, z] before unquantisation) of a non-reserved
    block, transformed endpoints already resolved (base + delta) and, signed, sign-extended."""
    mode, _value = mode_index(block)
    value, regions, transformed, prec, deltas, _ = MODES[mode]
    v = int.from_bytes(bytes(block), "little")
    e = fields(block)
    partition = (v >> 77) & 31 if regions == 2 else 0
    ends = [[e[c + k] for c in "rgb"] for k in "wxyz"[: 2 * regions]]
    mask = (1 << prec) - 1
    for k in range(1, 2 * regions):
        for c in range(3):
            if transformed:
                ends[k][c] = (ends[0][c] + _sext(ends[k][c], deltas[c])) & mask
            elif signed:
                ends[k][c] = _sext(ends[k][c], prec)
    if signed:
        for k in range(2 * regions):
            for c in range(3):
                if transformed or k == 0:
                    ends[k][c] = _sext(ends[k][c], prec)
    return regions, partition, prec, ends


def decode_block(block, signed, rounding=32):
    """16 bytes -> [16][4] half-float bit patterns (row-major texels).  (rounding: the interpolation's rounding term,
    32 in the specification; pillow_mask() asks what 0 would give.)"""
    mode, _value = mode_index(block)
    if mode is None:
        return [[0, 0, 0, 0x3C00] for _ in range(16)]
    regions, partition, prec, ends = endpoints(block, signed)
    unq = [[_unquantize(x, prec, signed) for x in end] for end in ends]
    v = int.from_bytes(bytes(block), "little")
    ib = 3 if regions == 2 else 4
    pos = 82 if regions == 2 else 65
    anchors = (0, ANCHORS_2[partition]) if regions == 2 else (0,)
    out = []
    for t in range(16):
        n = ib - 1 if t in anchors else ib
        idx = (v >> pos) & ((1 << n) - 1)
        pos += n
        s = (PARTITIONS_2[partition] >> t) & 1 if regions == 2 else 0
        w = WEIGHTS[ib][idx]
        rgb = [_finish(_interpolate(unq[2 * s][c], unq[2 * s + 1][c], w, rounding), signed) for c in range(3)]
        out.append(rgb + [0x3C00])
    assert pos == 128
    return out


def decode(blocks, w, h, signed):
    """BC6H texture (blocks row-major, w and h multiples of 4) -> uint16 [h, w, 4] half-float bit patterns."""
    data = bytes(blocks)
    bw = w // 4
    assert len(data) >= (w // 4) * (h // 4) * 16
    img = np.zeros((h, w, 4), dtype=np.uint16)
    cache = {}
    for b in range((w // 4) * (h // 4)):
        blk = data[16 * b: 16 * b + 16]
        px = cache.get(blk)
        if px is None:
            px = cache[blk] = np.array(decode_block(blk, signed), dtype=np.uint16).reshape(4, 4, 4)
        by, bx = divmod(b, bw)
        img[4 * by: 4 * by + 4, 4 * bx: 4 * bx + 4] = px
    return img


# ---------------------------------------------------------------------------------------------------- Pillow
def to_pillow_8bit(pic):
    """What Pillow makes of half-float RGB: 0 below zero (and for -0), 255 above 1.0, else trunc(h * 255).  uint8
    [h, w, 3] of a uint16 [h, w, 4] picture."""
    f = pic[..., :3].view(np.float16).astype(np.float64)
    out = np.floor(np.clip(f, 0.0, 1.0) * 255.0)
    return out.astype(np.uint8)


def pillow_bc6h_decode(blocks, w, h, signed):
    """Pillow's BC6H decoder (third-party code): uint8 [h, w, 3]."""
    from PIL import Image
    img = Image.frombytes("RGB", (w, h), bytes(blocks)[: (w // 4) * (h // 4) * 16], "bcn",
                          (6, "BC6HS" if signed else "BC6H"))
    return np.asarray(img, dtype=np.uint8).reshape(h, w, 3)


def pillow_mask(blocks, w, h, signed):
    """bool [h, w]: texels where Pillow (12.2) departs from the specification, so comparisons with it leave them out.

    1. Pillow interpolates as ((64 - w) * a + w * b) >> 6, without the specification's + 32: texels whose 8-bit value
       that rounding changes.
    2. Signed format, transformed modes: Pillow does not sign-extend the endpoints it rebuilds from base + delta, so a
       region with a negative endpoint comes out wrong: every texel of such a region.
    Outside the mask Pillow and the reference agree exactly (tests/test_bc6h_reference.py); hand-worked blocks there pin
    the specification's side of both points."""
    data = bytes(blocks)
    bw = w // 4
    m = np.zeros((h, w), dtype=bool)
    for b in range((w // 4) * (h // 4)):
        blk = data[16 * b: 16 * b + 16]
        mode, _value = mode_index(blk)
        if mode is None:
            continue
        by, bx = divmod(b, bw)
        spec = to_pillow_8bit(np.array(decode_block(blk, signed), dtype=np.uint16).reshape(4, 4, 4))
        trunc = to_pillow_8bit(np.array(decode_block(blk, signed, rounding=0), dtype=np.uint16).reshape(4, 4, 4))
        bad = (spec != trunc).any(-1).reshape(16)
        if signed and MODES[mode][2]:
            regions, partition, _prec, ends = endpoints(blk, signed)
            for t in range(16):
                s = (PARTITIONS_2[partition] >> t) & 1 if regions == 2 else 0
                bad[t] |= min(ends[2 * s] + ends[2 * s + 1]) < 0
        m[4 * by: 4 * by + 4, 4 * bx: 4 * bx + 4] = bad.reshape(4, 4)
    return m


# ---------------------------------------------------------------------------------------------------- the generator
def _band_endpoint(rng, prec, signed):
    """An endpoint whose unquantised value finishes inside (0, 1.0]: the band Pillow's 8-bit output resolves."""
    # half 0x1C00 (2^-8) .. 0x3C00 (1.0) -> 16-bit values before the finish, then back to `prec` bits
    h = 0x1C00 + rng.next() % 0x2000
    unq = (h * 64 + 30) // 31 if not signed else (h * 32 + 30) // 31
    top = 0xFFFF if not signed else 0x7FFF
    if prec >= (15 if not signed else 16):
        return min(unq, top)
    if not signed:
        return min(max((unq * ((1 << prec) - 1) + 0x8000) >> 16, 1), (1 << prec) - 2)
    return min(max((unq * ((1 << (prec - 1)) - 1) + 0x4000) >> 15, 1), (1 << (prec - 1)) - 2)


def _store(v, pos, mode, values):
    """OR the endpoint fields `values` (name -> value) into block integer v from bit `pos` in the mode's layout."""
    for name, bits in layout(mode):
        for b in bits:
            v |= ((values.get(name, 0) >> b) & 1) << pos
            pos += 1
    return v, pos


def make_block(mode, rng, partition=0, signed=False, band=False, saturate=None, wrap=False):
    """One block of mode index `mode` (0..13): endpoint fields random, or (band) chosen so the region's endpoints finish
    inside Pillow's band, or (saturate 0 / 1) all zero / all one, or (wrap, transformed modes) bases of 0..3 with
    negative deltas that take the endpoints below zero, so that they wrap; partition as given; indices random."""
    value, regions, transformed, prec, deltas, _ = MODES[mode]
    widths = dict.fromkeys(FIELDS, 0)
    for name, bits in layout(mode):
        widths[name] = max(widths[name], max(bits) + 1)
    if saturate is not None:
        values = {n: ((1 << widths[n]) - 1) * saturate for n in FIELDS}
    elif wrap and transformed:
        values = {}
        for ci, c in enumerate("rgb"):
            values[c + "w"] = rng.next() % 4
            for k in "xyz"[: 2 * regions - 1]:
                d = deltas[ci]
                values[c + k] = -(4 + rng.next() % ((1 << (d - 1)) - 4)) & ((1 << d) - 1)
    elif band:
        # base endpoints in the band, the others either in the band too (untransformed) or small deltas from the base
        values = {}
        for k in "wxyz"[: 2 * regions]:
            for ci, c in enumerate("rgb"):
                n = c + k
                if k == "w" or not transformed:
                    e = _band_endpoint(rng, prec, signed)
                    values[n] = e & ((1 << widths[n]) - 1)
                else:
                    d = deltas[ci]
                    small = rng.next() % (1 << max(d - 2, 1))
                    values[n] = (small if rng.next() & 1 else -small) & ((1 << d) - 1)
    else:
        values = {n: rng.bits(widths[n]) for n in FIELDS if widths[n]}
    v = value
    v, pos = _store(v, mode_bits(value), mode, values)
    if regions == 2:
        v |= partition << pos
        pos += 5
    v |= rng.bits(128 - pos) << pos
    return v.to_bytes(16, "little")


def reserved_block(value, rng):
    return ((rng.bits(123) << 5) | value).to_bytes(16, "little")


def block_sets(seed=0x42433648):
    """name -> bytes of blocks.  Per signedness s in ("u", "s"): "mode<value>_<s>" for each mode (every partition of a
    two-region mode; random, band-biased, saturated and wrapping endpoints), "reserved_<s>", and "mixed_<s>": all of
    them shuffled.  The signed sets are made for the signed format (band endpoints there are positive); each set decodes
    under either."""
    rng = SplitMix64(seed)
    sets = {}
    for s, signed in (("u", False), ("s", True)):
        names = []
        for mode, m in enumerate(MODES):
            out = []
            for partition in range(32 if m[1] == 2 else 4):
                for kind in ("wrap" if partition % 4 == 3 else "random", "band", "band", "sat%d" % (partition % 2)):
                    out.append(make_block(mode, rng, partition if m[1] == 2 else 0, signed, band=kind == "band",
                                          saturate=int(kind[3]) if kind.startswith("sat") else None,
                                          wrap=kind == "wrap"))
            while len(out) % 16:
                out.append(make_block(mode, rng, rng.bits(5) if m[1] == 2 else 0, signed, band=True))
            name = "mode%02x_%s" % (m[0], s)
            sets[name] = b"".join(out)
            names.append(name)
        sets["reserved_" + s] = b"".join(reserved_block(RESERVED[i % 4], rng) for i in range(16))
        names.append("reserved_" + s)
        allb = [b for name in names for b in (sets[name][i:i + 16] for i in range(0, len(sets[name]), 16))]
        for i in range(len(allb) - 1, 0, -1):                  # Fisher-Yates with the same generator
            j = rng.next() % (i + 1)
            allb[i], allb[j] = allb[j], allb[i]
        sets["mixed_" + s] = b"".join(allb)
    return sets


def set_is_signed(name):
    return name.endswith("_s")


def random_blocks(n, seed):
    """n blocks of uniformly random bits (every mode appears; 4 in 32 of 5-bit-mode blocks are reserved)."""
    rng = SplitMix64(seed)
    return b"".join(rng.bits(128).to_bytes(16, "little") for _ in range(n))


def geometry(nblocks):
    """(w, h) of a picture 16 blocks wide holding nblocks blocks (nblocks a multiple of 16)."""
    assert nblocks % 16 == 0
    return 64, 4 * (nblocks // 16)

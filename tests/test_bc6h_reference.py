"""The CPU reference of BC6H (tests/_bc6h.py) that the GPU tests of the BC6H -> RGBA16F kernel compare against: pinned
to Pillow's decoder through recorded digests (tests/golden/bc6h_pillow.json) and live where Pillow is installed, and
to blocks worked out by hand from the BC6H definition.

Pillow returns 8-bit RGB only: 0 below zero, 255 above 1.0, trunc(h * 255) between (_bc6h.to_pillow_8bit).  It departs
from the specification in two places, and the comparisons leave those texels out (_bc6h.pillow_mask): it interpolates
without the + 32 rounding term, and for the signed format it does not sign-extend the endpoints of transformed modes
after adding the deltas.  test_interpolation_rounds and test_transformed_two_region_mode_with_a_wrapping_delta pin the
specification's side of both."""
import hashlib
import json
import os

import numpy as np
import pytest

import _bc6h as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc6h_pillow.json")
ONE = 0x3C00


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["sets"]


class BitWriter:
    """Fields appended least significant bit first, as BPTC reads them."""

    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        self.v |= value << self.n
        self.n += bits
        return self

    def block(self):
        assert self.n == 128, self.n
        return self.v.to_bytes(16, "little")


def _blocks(data):
    return [data[i:i + 16] for i in range(0, len(data), 16)]


def _projection(data, signed):
    """(reference projected through Pillow's 8-bit mapping, with the texels of pillow_mask set to 0; the mask)"""
    w, h = B.geometry(len(data) // 16)
    ref = B.to_pillow_8bit(B.decode(data, w, h, signed))
    mask = B.pillow_mask(data, w, h, signed)
    ref[mask] = 0
    return ref, mask


def test_block_sets_are_what_the_digests_were_made_from():
    sets = B.block_sets()
    golden = _golden()
    assert sorted(sets) == sorted(golden)
    for name, data in sets.items():
        assert hashlib.sha256(data).hexdigest() == golden[name]["blocks_sha256"], name
        assert golden[name]["signed"] == B.set_is_signed(name)


def test_block_sets_cover_every_mode_partition_and_reserved_value():
    sets = B.block_sets()
    for s in ("u", "s"):
        seen = set()
        for name, data in sets.items():
            if not name.endswith("_" + s):
                continue
            for blk in _blocks(data):
                mode, value = B.mode_index(blk)
                if mode is None:
                    seen.add(("reserved", value))
                    continue
                partition = (int.from_bytes(blk, "little") >> 77) & 31
                seen.add((value, partition if B.MODES[mode][1] == 2 else 0))
        for m in B.MODES:
            for p in range(32 if m[1] == 2 else 1):
                assert (m[0], p) in seen, (s, hex(m[0]), p)
        for value in B.RESERVED:
            assert ("reserved", value) in seen, (s, value)


def test_block_sets_have_saturated_endpoints_and_wrapping_deltas():
    sets = B.block_sets()
    for s in ("u", "s"):
        for mode, m in enumerate(B.MODES):
            value, regions, transformed, prec, deltas, _ = m
            blocks = _blocks(sets["mode%02x_%s" % (value, s)])
            fields = [B.fields(b) for b in blocks]
            # every endpoint field all ones in some block, all zeros in another
            assert any(all(f[n] == max(g[n] for g in fields) for n in B.FIELDS) and f["rw"] for f in fields), (s, value)
            assert any(not any(f.values()) for f in fields), (s, value)
            if not transformed:
                continue
            # a negative delta whose sum with the base leaves the endpoint range and wraps
            wraps = False
            for f in fields:
                for ci, c in enumerate("rgb"):
                    base = f[c + "w"]
                    for k in "xyz"[: 2 * regions - 1]:
                        d = B._sext(f[c + k], deltas[ci])
                        wraps |= d < 0 and base + d < 0
            assert wraps, (s, value)


def test_block_sets_put_a_share_of_texels_in_pillows_band():
    """Pillow's 8-bit picture only resolves halves between 2^-8 and 1.0: at least a quarter of the texels of every
    set (at the signedness it was made for) fall there, so the pin to Pillow is more than zeros and 255s."""
    for name, data in B.block_sets().items():
        if name.startswith("reserved"):
            continue
        ref, mask = _projection(data, B.set_is_signed(name))
        band = ((ref > 0) & (ref < 255)).any(-1) & ~mask
        assert band.mean() >= 0.25, (name, band.mean())


def test_reference_matches_the_recorded_pillow_digests():
    sets = B.block_sets()
    for name, rec in _golden().items():
        data = sets[name]
        assert (rec["width"], rec["height"]) == B.geometry(len(data) // 16)
        ref, _mask = _projection(data, rec["signed"])
        assert hashlib.sha256(ref.tobytes()).hexdigest() == rec["pillow_sha256"], name


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_reference_matches_live_pillow(seed, signed):
    pytest.importorskip("PIL")
    data = B.random_blocks(1024, 0x5EED0600 + seed)
    rng = B.SplitMix64(seed * 2 + signed)
    for mode, m in enumerate(B.MODES):                   # and fresh band-biased blocks of every mode
        data += b"".join(B.make_block(mode, rng, rng.bits(5) if m[1] == 2 else 0, signed, band=True) for _ in range(32))
    w, h = B.geometry(len(data) // 16)
    ref, mask = _projection(data, signed)
    theirs = B.pillow_bc6h_decode(data, w, h, signed)
    assert np.array_equal(ref[~mask], theirs[~mask])
    assert mask.mean() < 0.75                            # (random signed blocks: about half have a negative endpoint)


def test_pillows_8bit_mapping_over_the_whole_range():
    """Mode 0x0F with all indices 0 puts its 16-bit endpoint on every texel unchanged: every half 0 .. 0x7BFF
    (unsigned) and every signed value goes through Pillow and lands where to_pillow_8bit says."""
    pytest.importorskip("PIL")
    mode = B.MODE_OF_VALUE[0x0F]

    def block(e):
        v, _pos = B._store(0x0F, 5, mode, {"rw": e, "gw": e, "bw": e})
        return v.to_bytes(16, "little")

    data = b"".join(block(e) for e in range(0x10000))
    for signed in (False, True):
        pic = B.decode(data, 1024, 1024, signed)
        theirs = B.pillow_bc6h_decode(data, 1024, 1024, signed)
        assert np.array_equal(B.to_pillow_8bit(pic), theirs), signed


# ------------------------------------------------------------------------------------------- hand-worked blocks
def test_mode_03_raw_endpoints():
    # mode 0x03: one region, 10-bit endpoints stored as they are; 462 -> ((462 << 16) + 0x8000) >> 10 = 29600;
    # x 31 / 64 = 14337 = 0x3801 (0.50049).  Pillow: trunc(0.50049 * 255) = 127.  All indices 0: endpoint w everywhere.
    w = BitWriter().put(0x03, 5)
    for _ in range(3):
        w.put(462, 10)
    for _ in range(3):
        w.put(0, 10)
    w.put(0, 63)
    assert B.decode_block(w.block(), False) == [[0x3801] * 3 + [ONE]] * 16
    assert B.to_pillow_8bit(np.array([[0x3801, 0x3801, 0x3801, ONE]], dtype=np.uint16))[0].tolist() == [127] * 3


def test_unsigned_maximum():
    # endpoint 1023 of 10 bits -> 0xFFFF -> 0xFFFF * 31 >> 6 = 0x7BFF (65504, the largest finite half)
    w = BitWriter().put(0x03, 5)
    for _ in range(6):
        w.put(1023, 10)
    w.put(0, 63)
    assert B.decode_block(w.block(), False) == [[0x7BFF] * 3 + [ONE]] * 16


def test_interpolation_rounds():
    # mode 0x03, w = 0, x = 1023 (0xFFFF); texel 0 index 0 (3 bits), the others index 1 (weight 4):
    # (60 * 0 + 4 * 65535 + 32) >> 6 = 4096 -> 4096 * 31 >> 6 = 1984 = 0x07C0 (without the + 32: 4095 -> 0x07BF)
    w = BitWriter().put(0x03, 5)
    for _ in range(3):
        w.put(0, 10)
    for _ in range(3):
        w.put(1023, 10)
    w.put(0, 3)
    for _ in range(15):
        w.put(1, 4)
    got = B.decode_block(w.block(), False)
    assert got[0] == [0, 0, 0, ONE]
    assert got[1:] == [[0x07C0] * 3 + [ONE]] * 15


def _mode_00_block(rx):
    """Mode 0x00 (two regions, transformed, 10-bit base, 5-bit deltas), partition 0 (texels 2, 3, 6, 7, 10, 11, 14,
    15 in region 1; anchor 15), every channel alike: w = 2, x = delta rx, y = z = delta 0.  Indices: 0 on texel 0 and
    region 1, 7 on the other region-0 texels.  Fields in the mode's order: m[1:0] gy[4] by[4] bz[4] rw[9:0] gw[9:0]
    bw[9:0] rx[4:0] gz[4] gy[3:0] gx[4:0] bz[0] gz[3:0] bx[4:0] bz[1] by[3:0] ry[4:0] bz[2] rz[4:0] bz[3] d[4:0]."""
    w = BitWriter().put(0, 2).put(0, 1).put(0, 1).put(0, 1)
    w.put(2, 10).put(2, 10).put(2, 10)
    w.put(rx, 5).put(0, 1).put(0, 4).put(rx, 5).put(0, 1).put(0, 4).put(rx, 5).put(0, 1).put(0, 4)
    w.put(0, 5).put(0, 1).put(0, 5).put(0, 1)
    w.put(0, 5)                                            # partition 0
    region1 = (0xCCCC >> np.arange(16)) & 1
    for t in range(16):
        bits = 2 if t in (0, 15) else 3
        w.put(0 if t == 0 or region1[t] else 7, bits)
    return w.block(), region1


def test_transformed_two_region_mode_with_a_wrapping_delta():
    # delta rx = -3 (0b11101): x = (2 - 3) & 0x3FF = 1023.
    # Unsigned: w = 2 -> ((2 << 16) + 0x8000) >> 10 = 160 -> 160 * 31 >> 6 = 77 = 0x004D; x = 1023 -> 0xFFFF -> 0x7BFF.
    # Signed: x sign-extends to -1 -> -(((1 << 15) + 0x4000) >> 9) = -96; w = 2 -> 160 -> 160 * 31 >> 5 = 155 = 0x009B;
    # weight 64: (64 * -96 + 32) >> 6 = -96 -> 0x8000 | (96 * 31 >> 5) = 0x805D.  (Pillow, which leaves x at +1023 after
    # the add, gives 255 for those texels: the specification says negative.)
    blk, region1 = _mode_00_block(0b11101)
    assert B.endpoints(blk, False)[3] == [[2] * 3, [1023] * 3, [2] * 3, [2] * 3]
    assert B.endpoints(blk, True)[3] == [[2] * 3, [-1] * 3, [2] * 3, [2] * 3]
    for signed, at_w, at_x in ((False, 0x004D, 0x7BFF), (True, 0x009B, 0x805D)):
        got = B.decode_block(blk, signed)
        for t in range(16):
            want = at_w if t == 0 or region1[t] else at_x
            assert got[t] == [want] * 3 + [ONE], (signed, t)
    # a positive delta: 2 + 15 = 17
    blk, _ = _mode_00_block(15)
    assert B.endpoints(blk, False)[3][1] == [17] * 3


def _mode_0f_block(r, g, b, index=0):
    """Mode 0x0F (one region, 16-bit base, 4-bit deltas 0): m[4:0] rw[9:0] gw[9:0] bw[9:0] rx[3:0] rw[10:15] gx[3:0]
    gw[10:15] bx[3:0] bw[10:15] -- the top six bits of each base stored reversed (bit 15 first)."""
    def rev6(v):
        return int("{:06b}".format(v >> 10)[::-1], 2)
    w = BitWriter().put(0x0F, 5)
    for e in (r, g, b):
        w.put(e & 0x3FF, 10)
    for e in (r, g, b):
        w.put(0, 4).put(rev6(e), 6)
    w.put(index, 3)
    for _ in range(15):
        w.put(index, 4)
    return w.block()


def test_sixteen_bit_mode_with_reversed_runs():
    # R = 0xC000: its top six bits 110000 are stored 0, 0, 0, 0, 1, 1 from the lowest block bit up -- a decoder that
    # does not reverse them would read 0x0C00.  G = 0x0401 (low and high part), B = 0.  Unsigned, 16 bits: no
    # unquantisation; 0xC000 * 31 >> 6 = 0x5D00, 0x0401 * 31 >> 6 = 496 = 0x01F0.
    blk = _mode_0f_block(0xC000, 0x0401, 0)
    assert B.fields(blk)["rw"] == 0xC000 and B.fields(blk)["gw"] == 0x0401
    assert B.decode_block(blk, False) == [[0x5D00, 0x01F0, 0, ONE]] * 16


def test_signed_negative_endpoint_and_negative_zero():
    # signed: 0xC000 is -16384 -> 0x8000 | (16384 * 31 >> 5) = 0xBE00 (-1.5); 0xFFFF is -1: (64 * -1 + 32) >> 6 = -1
    # -> 0x8000 | (31 >> 5) = 0x8000, negative zero, kept as it is; 0x0401 -> 1025 * 31 >> 5 = 992 = 0x03E0
    assert B.decode_block(_mode_0f_block(0xC000, 0xFFFF, 0x0401), True) == [[0xBE00, 0x8000, 0x03E0, ONE]] * 16


@pytest.mark.parametrize("value", B.RESERVED)
def test_reserved_modes(value):
    rng = B.SplitMix64(value)
    for _ in range(4):
        blk = B.reserved_block(value, rng)
        assert B.mode_index(blk) == (None, value)
        for signed in (False, True):
            assert B.decode_block(blk, signed) == [[0, 0, 0, ONE]] * 16
    if value == B.RESERVED[0]:
        pytest.importorskip("PIL")
        data = b"".join(B.reserved_block(v, rng) for v in B.RESERVED * 4)
        for signed in (False, True):
            assert not B.pillow_bc6h_decode(data, 64, 4, signed).any()

"""The CPU reference of BC7 (tests/_bptc.py) that the GPU tests of the BC7 -> RGBA kernel compare against: pinned to
Pillow's decoder through recorded digests (tests/golden/bptc_pillow.json) and live where Pillow is installed, and to a
few blocks worked out by hand from the BPTC definition."""
import hashlib
import json
import os

import numpy as np
import pytest

import _bptc as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bptc_pillow.json")


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


def test_block_sets_are_what_the_digests_were_made_from():
    sets = B.block_sets()
    golden = _golden()
    assert sorted(sets) == sorted(golden)
    for name, data in sets.items():
        assert hashlib.sha256(data).hexdigest() == golden[name]["blocks_sha256"], name


def test_block_sets_cover_every_mode_partition_rotation_and_selection():
    sets = B.block_sets()
    seen = set()
    for name, data in sets.items():
        for i in range(0, len(data), 16):
            v = int.from_bytes(data[i:i + 16], "little")
            if v & 0xFF == 0:
                seen.add(("reserved",))
                continue
            mode = (v & -v).bit_length() - 1
            ns, pb, rb, isb = B.MODES[mode][:4]
            f = v >> (mode + 1)
            seen.add((mode, "partition", f & ((1 << pb) - 1)))
            seen.add((mode, "rotation", (f >> pb) & ((1 << rb) - 1), (f >> (pb + rb)) & ((1 << isb) - 1)))
    for mode in range(8):
        ns, pb, rb, isb = B.MODES[mode][:4]
        for p in range(1 << pb):
            assert (mode, "partition", p) in seen
        for r in range(1 << rb):
            for s in range(1 << isb):
                assert (mode, "rotation", r, s) in seen
    assert ("reserved",) in seen
    # saturated endpoints and p-bits: in every mode some block has all of them one (white; opaque where the mode has
    # no alpha) and some all of them zero
    for mode in range(8):
        data = sets["mode%d" % mode]
        pics = [B.decode_block(data[i:i + 16]) for i in range(0, len(data), 16)]
        assert [[255, 255, 255, 255]] * 16 in pics, mode
        assert [[0, 0, 0, 0 if B.MODES[mode][5] else 255]] * 16 in pics, mode


def test_reference_matches_the_recorded_pillow_digests():
    """Pillow's pictures of every block set, recorded where Pillow was installed; its (0, 0, 0, 255) for reserved
    blocks (the specification says (0, 0, 0, 0)) is put into the reference's picture before hashing."""
    sets = B.block_sets()
    for name, rec in _golden().items():
        data = sets[name]
        w, h = rec["width"], rec["height"]
        pic = B.decode(data, w, h)
        pic[B.reserved_mask(data, w, h)] = (0, 0, 0, 255)
        assert hashlib.sha256(pic.tobytes()).hexdigest() == rec["pillow_sha256"], name


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_matches_live_pillow(seed):
    pytest.importorskip("PIL")
    data = B.random_blocks(1024, 0x5EED0000 + seed)
    for i, mode in enumerate(range(8)):                  # and fresh blocks of every mode from the generator
        rng = B.SplitMix64(seed * 8 + mode)
        ns, pb, rb, isb = B.MODES[mode][:4]
        data += b"".join(B.make_block(mode, rng, rng.bits(pb), rng.bits(rb), rng.bits(isb)) for _ in range(64))
    w, h = B.geometry(len(data) // 16)
    ref = B.decode(data, w, h)
    theirs = B.pillow_bc7_decode(data, w, h)
    keep = ~B.reserved_mask(data, w, h)        # reserved blocks: Pillow gives (0, 0, 0, 255), the specification zeros
    assert np.array_equal(ref[keep], theirs[keep])


def test_solid_mode_6_block():
    # mode 6: 7-bit RGBA endpoints with a p-bit each, 4-bit indices; endpoint 0 with p-bit 0: (0x55, 0x2A, 0x7F, 0)
    # -> (0xAA, 0x54, 0xFE, 0x00); all indices 0 -> every texel is endpoint 0
    w = BitWriter().put(1 << 6, 7)
    for c0, c1 in ((0x55, 0x55), (0x2A, 0x2A), (0x7F, 0x7F), (0x00, 0x00)):
        w.put(c0, 7).put(c1, 7)
    w.put(0, 1).put(1, 1)                        # p-bits of endpoints 0 and 1
    w.put(0, 3)                                  # texel 0 (anchor): 3 bits
    for _ in range(15):
        w.put(0, 4)
    assert B.decode_block(w.block()) == [[170, 84, 254, 0]] * 16


def test_mode_4_rotation_swaps_red_and_alpha():
    # mode 4, rotation 1 (A <-> R), index selection 0; 5-bit colour, 6-bit alpha, no p-bits:
    # R 31 -> 255, G 0 -> 0, B 16 -> 128 | 4 = 132, A 0 -> 0; (255, 0, 132, 0) rotated -> (0, 0, 132, 255)
    w = BitWriter().put(1 << 4, 5).put(1, 2).put(0, 1)
    for c in (31, 0, 16):
        w.put(c, 5).put(c, 5)
    w.put(0, 6).put(0, 6)
    w.put(0, 31).put(0, 47)                      # 2-bit and 3-bit indices, all 0
    assert B.decode_block(w.block()) == [[0, 0, 132, 255]] * 16


def test_three_subset_block_with_both_anchors():
    # mode 2, partition 0: subsets 0 0 1 1 / 0 0 1 1 / 0 2 2 1 / 2 2 2 2, anchors texel 0, 3 (subset 1), 15 (subset 2)
    # grey endpoints (5 bits, no p-bit): subset 0: 0 -> 0, 31 -> 255; subset 1: 0 -> 0, 16 -> 132; subset 2:
    # 8 -> 66, 24 -> 198.  Indices: 1 on the anchors (1 bit: weight 21), 3 elsewhere (weight 64 = endpoint 1)
    w = BitWriter().put(1 << 2, 3).put(0, 6)
    ends = (0, 31, 0, 16, 8, 24)
    for _ in range(3):
        for e in ends:
            w.put(e, 5)
    for t in range(16):
        if t in (0, 3, 15):
            w.put(1, 1)
        else:
            w.put(3, 2)
    got = [px[0] for px in B.decode_block(w.block())]
    # texel 0: (43 * 0 + 21 * 255 + 32) >> 6 = 84; texel 3: (21 * 132 + 32) >> 6 = 43;
    # texel 15: (43 * 66 + 21 * 198 + 32) >> 6 = 109
    assert got == [84, 255, 132, 43, 255, 255, 132, 132, 255, 198, 198, 132, 198, 198, 198, 109]
    assert all(px[3] == 255 and px[0] == px[1] == px[2] for px in B.decode_block(w.block()))


def test_reserved_block_decodes_to_zeros():
    assert B.decode_block(bytes(16)) == [[0, 0, 0, 0]] * 16
    assert B.decode_block(bytes([0]) + bytes(range(1, 16))) == [[0, 0, 0, 0]] * 16

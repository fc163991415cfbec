"""CPU half of the value-space sweeps (tests/_value_space.py): the coverage each sweep claims is reached, the oracle's
block decoders equal a plain integer restatement of the formats on every sweep, and Pillow's DDS reader agrees on
the DXT1, DXT5 and RGTC1 sweeps.  The GPU half, tests/test_value_space_gpu.py, holds the kernels to the oracle on the
same sweeps; tests/test_value_space_derived_gpu.py does so for the half- and quarter-size, region, planes, composite
and measure launches, whose sweeps with random codes are held here to every residue of the region sums."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V


def _report(capsys, line):
    with capsys.disabled():
        print("\n  value space: " + line, end="")


def _alpha_fields(blocks8):
    """(a0, a1, codes [n, 16]) of 8-byte alpha blocks."""
    b = blocks8.astype(np.uint64)
    bits = np.zeros(len(b), dtype=np.uint64)
    for i in range(6):
        bits |= b[:, 2 + i] << np.uint64(8 * i)
    codes = ((bits[:, None] >> (np.uint64(3) * np.arange(16, dtype=np.uint64))[None, :]) & np.uint64(7)).astype(np.int64)
    return blocks8[:, 0].astype(np.int64), blocks8[:, 1].astype(np.int64), codes


def _colour_fields(blocks8):
    """(c0, c1, indices [n, 16]) of 8-byte colour blocks."""
    b = blocks8.astype(np.int64)
    c0, c1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    idx = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    return c0, c1, (idx[:, None] >> (2 * np.arange(16))[None, :]) & 3


def _expand(c):
    """int [n] 5:6:5 -> [n, 3] 8-bit channels"""
    return np.stack([V.E5[c >> 11], V.E6[(c >> 5) & 63], V.E5[c & 31]], axis=-1)


# ---- the formats restated: integer division as Python (and numpy on non-negative values) define it --
def restated_alpha(blocks8):
    a0, a1, codes = _alpha_fields(blocks8)
    i = np.arange(1, 7)[None, :]
    eight = ((7 - i) * a0[:, None] + i * a1[:, None]) // 7
    i = np.arange(1, 5)[None, :]
    six = ((5 - i) * a0[:, None] + i * a1[:, None]) // 5
    six = np.concatenate([six, np.zeros((len(a0), 1), np.int64), np.full((len(a0), 1), 255)], axis=1)
    pal = np.concatenate([a0[:, None], a1[:, None], np.where((a0 > a1)[:, None], eight, six)], axis=1)
    return np.take_along_axis(pal, codes, axis=1)


def restated_colour(blocks8, dxt1_modes):
    """[n, 16, 3]"""
    c0, c1, idx = _colour_fields(blocks8)
    e0, e1 = _expand(c0), _expand(c1)
    four = (~dxt1_modes | (c0 > c1))[:, None]
    p2 = np.where(four, (2 * e0 + e1) // 3, (e0 + e1) // 2)
    p3 = np.where(four, (e0 + 2 * e1) // 3, 0)
    pal = np.stack([e0, e1, p2, p3], axis=1)                                 # [n, 4, 3]
    return np.take_along_axis(pal, idx[:, :, None].repeat(3, axis=2), axis=1)


def truncating_divide(c, s):
    """c / s rounded toward zero (C's integer division), c of either sign, s > 0"""
    return np.sign(c) * (np.abs(c) // s)


def restated_hapq(blocks16):
    """[n, 16, 4] RGBA of scaled YCoCg-DXT5 blocks"""
    y = restated_alpha(blocks16[:, :8])
    pal = restated_colour(blocks16[:, 8:], np.zeros(len(blocks16), bool))
    s = (pal[..., 2] >> 3) + 1
    co = truncating_divide(pal[..., 0] - 128, s)
    cg = truncating_divide(pal[..., 1] - 128, s)
    rgb = np.stack([y + co - cg, y + cg, y - co - cg], axis=-1)
    return np.concatenate([np.clip(rgb, 0, 255), np.full(y.shape + (1,), 255)], axis=-1)


def _oracle_blocks(blocks, fmt):
    """oracle decoder on a picture of the blocks -> [n, 16, 4] (RGTC1: [n, 16])"""
    w = 4 * V.BLOCK_ROW
    h = 4 * len(blocks) // V.BLOCK_ROW
    pic = D.oracle_bc_decode(np.ascontiguousarray(blocks).tobytes(), fmt, w, h)
    if fmt == L.FMT_RGTC1:
        return V.blocks_of_picture(np.repeat(pic[..., None], 4, axis=2))[..., 0]
    return V.blocks_of_picture(pic)


# ------------------------------------------------------------------------------------------------- coverage --
def test_ramp_sweep_coverage(capsys):
    b = V.ramp_blocks()
    a0, a1, codes = _alpha_fields(b)
    pairs = set(zip(a0.tolist(), a1.tolist()))
    assert len(pairs) == 65536
    assert int((a0 > a1).sum()) == 32640 and int((a0 <= a1).sum()) == 32896          # 8-value and 6-value palettes
    assert all(len(set(row)) == 8 for row in codes[:: 97].tolist()) and (np.sort(codes, axis=1) == np.repeat(np.arange(8), 2)).all()
    code_pos = {(c, p) for p in range(16) for c in np.unique(codes[:, p]).tolist()}
    assert len(code_pos) == 8 * 16
    _report(capsys, "ramp blocks: %d (a0, a1) pairs, %d codes x positions" % (len(pairs), len(code_pos)))


def test_colour_sweep_coverage(capsys):
    c0, c1, idx = _colour_fields(V.colour_blocks())
    fields = {"red": (c0 >> 11, c1 >> 11, 32), "green": ((c0 >> 5) & 63, (c1 >> 5) & 63, 64), "blue": (c0 & 31, c1 & 31, 32)}
    counts = []
    for name, (x0, x1, q) in fields.items():
        assert len(set(zip(x0.tolist(), x1.tolist()))) == q * q, name
        for mode in (c0 > c1, c0 <= c1):
            n = len(set(zip(x0[mode].tolist(), x1[mode].tolist())))
            if name != "red":                       # (red decides the order whenever its two values differ)
                assert n == q * q, name
            counts.append(n)
    assert int((c0 == c1).sum()) == 65536 and len(set(c0[c0 == c1].tolist())) == 65536
    ip = {(k, p) for p in range(16) for k in np.unique(idx[:, p]).tolist()}
    assert len(ip) == 4 * 16
    _report(capsys, "colour blocks: %d; ordered endpoint pairs in c0 > c1 / c0 <= c1 order: red %d / %d, green %d / %d, "
            "blue %d / %d; c0 == c1: 65536; indices x positions %d" % ((len(c0),) + tuple(counts) + (len(ip),)))


def test_hapq_colour_sweep_coverage(capsys):
    c0, c1, idx = _colour_fields(V.hapq_colour_blocks())
    e0, e1 = _expand(c0), _expand(c1)
    pal = np.stack([e0, e1, (2 * e0 + e1) // 3, (e0 + 2 * e1) // 3], axis=1)       # [n, slot, channel]
    # what any 5:6:5 palette can hold in each slot (red / green and blue are independent fields)
    p5 = np.array([(a, b) for a in range(32) for b in range(32)])
    p6 = np.array([(a, b) for a in range(64) for b in range(64)])
    all5 = V._palette_entries(V.E5[p5[:, 0]], V.E5[p5[:, 1]])
    all6 = V._palette_entries(V.E6[p6[:, 0]], V.E6[p6[:, 1]])
    got_total = want_total = 0
    scales = set()
    for slot in range(4):
        s_all = np.unique((all5[:, slot] >> 3) + 1)
        s = (pal[:, slot, 2] >> 3) + 1
        scales |= set(s.tolist())
        for ch, allv in ((0, all5), (1, all6)):
            want = {(v, t) for v in np.unique(allv[:, slot]).tolist() for t in s_all.tolist()}
            got = set(zip(pal[:, slot, ch].tolist(), s.tolist()))
            assert got == want, (slot, ch, len(want - got))
            got_total += len(got)
            want_total += len(want)
    assert scales == set(range(1, 33))
    ip = {(k, p) for p in range(16) for k in np.unique(idx[:, p]).tolist()}
    assert len(ip) == 64
    _report(capsys, "Hap Q colour blocks: %d; (chroma byte, scale) pairs over 4 slots x Co, Cg: %d of %d; scales %d" % (
        len(c0), got_total, want_total, len(scales)))


def test_encode_picture_coverage(capsys):
    px = V.blocks_of_picture(V.ramp_picture()).astype(np.int64)
    assert (px == px[..., :1]).all()                                          # R = G = B = A
    v = px[..., 3]
    lo, hi = v.min(axis=1), v.max(axis=1)
    assert len(set(zip(lo.tolist(), hi.tolist()))) == 255 * 256 // 2
    d, u = hi - lo, hi[:, None] - v
    du = np.unique(d[:, None] * 256 + u)
    assert len(du) == sum(dd + 1 for dd in range(1, 256))                    # every (d, u), u = 0..d
    key = lo * 256 + hi
    seen = np.zeros((65536, 256), dtype=bool)
    seen[np.repeat(key, 16), v.ravel()] = True                               # (values lie in lo..hi by construction)
    assert seen.sum() == sum((h - l + 1) for l in range(256) for h in range(l + 1, 256))   # every value of every ramp
    img = V.all_colours_picture()
    c = img[..., 0].astype(np.int64) | img[..., 1].astype(np.int64) << 8 | img[..., 2].astype(np.int64) << 16
    assert np.bincount(c.ravel(), minlength=1 << 24).min() == 1 and c.size == 1 << 24
    # len2 from the endpoints of the oracle's own blocks
    pic = V.two_colour_picture()
    c0, c1, _ = _colour_fields(np.frombuffer(D.oracle_bc_encode(pic, L.FMT_DXT1), np.uint8).reshape(-1, 8))
    l2 = ((_expand(c0) - _expand(c1)) ** 2).sum(axis=1)
    got = np.unique(l2[c0 != c1])
    want, formable = V.encodable_len2(), V.formable_len2()
    assert np.array_equal(got, want)
    assert np.isin(want, formable).all()
    # the inset rule keeps every encoder out of the rest: not one of the 2^20 all-colour blocks reaches a len2 outside
    c0, c1, _ = _colour_fields(np.frombuffer(D.oracle_bc_encode(img, L.FMT_DXT1), np.uint8).reshape(-1, 8))
    l2 = ((_expand(c0) - _expand(c1)) ** 2).sum(axis=1)
    assert np.isin(np.unique(l2[c0 != c1]), want).all()
    # Hap Q scale edges: the largest |C - 128| of the blocks, and the scale the oracle picks
    pic = V.scale_edge_picture()
    rgb = V.blocks_of_picture(pic)[..., :3].astype(np.int64)
    co, cg = V.ycocg(rgb)
    m = np.maximum(np.abs(co - 128), np.abs(cg - 128)).max(axis=1)
    assert set(V.SCALE_EDGES) <= set(m.tolist()) and {127, 128} <= set(m.tolist())
    assert co.max() == 256 and co.min() == 1 and cg.max() == 256 and cg.min() == 1
    blocks = np.frombuffer(D.oracle_bc_encode(pic, L.FMT_YCOCG), np.uint8).reshape(-1, 16)
    s = (blocks[:, 8] & 31).astype(np.int64) + 1
    assert np.array_equal(s, np.where(m <= 31, 4, np.where(m <= 63, 2, 1)))
    _report(capsys, "encode pictures: %d (lo, hi) ramps, %d d values, %d (d, u) pairs, %d RGB colours, len2 values %d of "
            "the %d the inset endpoint rule allows (%d formable by any two 5:6:5 codes), scale edges %s" % (
                255 * 256 // 2, len(np.unique(d)), len(du), 1 << 24, len(got), len(want), len(formable),
                sorted(set(m.tolist()) & set(V.SCALE_EDGES + (127, 128)))))


# ------------------------------------------------------------- sweeps for the half- and quarter-size decoders --
def _region_sums(pic, s):
    """[h, w, c] -> int64 [h >> s, w >> s, c]: the sums of the 2^s x 2^s regions"""
    k = 1 << s
    h, w, c = pic.shape
    return pic.astype(np.int64).reshape(h // k, k, w // k, k, c).sum(axis=(1, 3))


def _picture(blocks, fmt, plane=None):
    """The oracle's picture of a sweep (A from the RGTC1 plane where there is one)"""
    w, h = 4 * V.BLOCK_ROW, 4 * len(blocks) // V.BLOCK_ROW
    pic = D.oracle_bc_decode(np.ascontiguousarray(blocks).tobytes(), fmt, w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(np.ascontiguousarray(plane).tobytes(), L.FMT_RGTC1, w, h)
    return pic


def _scaled_sweep(name):
    """(blocks, the rotating sweep they come from, format, plane | None, its rotating form | None)"""
    if name == "dxt1":
        return V.dxt1_scaled_sweep(), V.pad_blocks(V.colour_blocks()), L.FMT_DXT1, None, None
    if name == "dxt5":
        return V.dxt5_scaled_sweep(), V.dxt5_sweep(), L.FMT_DXT5, None, None
    (blocks, plane), (old, old_plane) = V.hapq_scaled_sweep(), V.hapq_sweep()
    if name == "hapq":
        plane = old_plane = None
    return blocks, old, L.FMT_YCOCG, plane, old_plane


def _flat_codes(codes):
    """the codes of the blocks whose 16 texels all carry the same one"""
    return set(codes[(codes == codes[:, :1]).all(axis=1), 0].tolist())


def test_rotating_codes_reach_only_even_region_sums():
    """Why the sweeps above are not enough at half and quarter size: with the code (p + k) % 4 at texel p, every region
    of a block holds every index it holds equally often, so the colour sums are multiples of 2 (s = 1) or 4 (s = 2)
    and the neighbours of the rounding term, half - 1 and half + 1, never occur."""
    pic = _picture(V.dxt5_sweep(), L.FMT_DXT5)
    for s in (1, 2):
        seen = np.unique(_region_sums(pic, s)[..., :3] % (1 << 2 * s))
        assert seen.tolist() == list(range(0, 1 << 2 * s, 1 << s)), (s, seen)


@pytest.mark.parametrize("name", ["dxt1", "dxt5", "hapq", "hapq_alpha"])
def test_scaled_sweep_coverage(capsys, name):
    blocks, old, fmt, plane, old_plane = _scaled_sweep(name)
    assert blocks.shape == old.shape and len(blocks) % V.BLOCK_ROW == 0
    # endpoints kept, code fields replaced: the value coverage of the rotating sweeps carries over
    colour = blocks if fmt == L.FMT_DXT1 else blocks[:, 8:]
    ramps = {} if fmt == L.FMT_DXT1 else {"first": blocks[:, :8]}
    assert np.array_equal(colour[:, :4], (old if fmt == L.FMT_DXT1 else old[:, 8:])[:, :4])
    if ramps:
        assert np.array_equal(blocks[:, :2], old[:, :2])
    if plane is not None:
        assert plane.shape == old_plane.shape and np.array_equal(plane[:, :2], old_plane[:, :2])
        ramps["plane"] = plane
    # both ramp orders and a0 == a1; all three colour orders; flat blocks with every code
    for what, half in ramps.items():
        a0, a1, codes = _alpha_fields(half)
        assert (a0 > a1).any() and (a0 < a1).any() and (a0 == a1).any(), what
        assert _flat_codes(codes) == set(range(8)), what
        assert len(np.unique(codes[1::4], axis=0)) > len(codes) // 8, what          # (the others are not flat)
    c0, c1, idx = _colour_fields(colour)
    assert (c0 > c1).any() and (c0 < c1).any() and (c0 == c1).any()
    assert _flat_codes(idx) == set(range(4))
    pic = _picture(blocks, fmt, plane)
    if fmt == L.FMT_YCOCG:
        # every scale code at a texel that picks it, and texels beyond either end of the byte range
        y = restated_alpha(blocks[:, :8])
        pal = restated_colour(colour, np.zeros(len(blocks), bool))
        scale = (pal[..., 2] >> 3) + 1
        assert set(np.unique(scale).tolist()) == set(range(1, 33))
        co, cg = truncating_divide(pal[..., 0] - 128, scale), truncating_divide(pal[..., 1] - 128, scale)
        rgb = np.stack([y + co - cg, y + cg, y - co - cg], axis=-1)
        texels = V.blocks_of_picture(pic)[..., :3]
        assert (rgb < 0).any() and (texels[rgb < 0] == 0).all()
        assert (rgb > 255).any() and (texels[rgb > 255] == 255).all()
    # the oracle's picture: every residue of the region sums in every channel that is not constant
    live = [c for c in range(4) if pic[..., c].min() != pic[..., c].max()]
    assert live == ([0, 1, 2] if name in ("dxt1", "hapq") else [0, 1, 2, 3])
    rarest = {}
    for s in (1, 2):
        texels = 1 << 2 * s
        sums = _region_sums(pic, s)
        counts = np.stack([np.bincount(sums[..., c].ravel() % texels, minlength=texels) for c in live])
        assert counts.min() > 0, (s, counts.tolist())
        rarest[s] = int(counts.min())
        if 3 in live:
            assert sums[..., 3].max() == texels * 255, s                            # no accumulator may wrap there
    _report(capsys, "%s at half / quarter size: %d blocks, rarest residue of a region sum %d / %d times" % (
        name, len(blocks), rarest[1], rarest[2]))


# ------------------------------------------------------------------------ oracle against the restatement --
def test_oracle_decoders_equal_the_restated_formats():
    ramps = V.ramp_blocks()
    assert np.array_equal(_oracle_blocks(ramps, L.FMT_RGTC1), restated_alpha(ramps))
    cols = V.pad_blocks(V.colour_blocks())
    got = _oracle_blocks(cols, L.FMT_DXT1)
    assert np.array_equal(got[..., :3], restated_colour(cols, np.ones(len(cols), bool))) and (got[..., 3] == 255).all()
    dxt5 = V.dxt5_sweep()
    got = _oracle_blocks(dxt5, L.FMT_DXT5)
    assert np.array_equal(got[..., :3], restated_colour(dxt5[:, 8:], np.zeros(len(dxt5), bool)))
    assert np.array_equal(got[..., 3], restated_alpha(dxt5[:, :8]))
    hapq, _alpha = V.hapq_sweep()
    assert np.array_equal(_oracle_blocks(hapq, L.FMT_YCOCG), restated_hapq(hapq))


# --------------------------------------------------------------------------------------------------- Pillow --
@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5, L.FMT_RGTC1])
def test_sweeps_against_pillow(fmt):
    pytest.importorskip("PIL")
    blocks = {L.FMT_DXT1: lambda: V.pad_blocks(V.colour_blocks()), L.FMT_DXT5: V.dxt5_sweep, L.FMT_RGTC1: V.ramp_blocks}[fmt]()
    w, h = 4 * V.BLOCK_ROW, 4 * len(blocks) // V.BLOCK_ROW
    data = np.ascontiguousarray(blocks).tobytes()
    theirs = D.pillow_bc_decode(data, fmt, w, h)
    ours = D.oracle_bc_decode(data, fmt, w, h)
    if fmt == L.FMT_RGTC1:
        assert np.array_equal(theirs, ours)
    elif fmt == L.FMT_DXT1:
        assert np.array_equal(theirs[..., :3], ours[..., :3])              # (DXT1's transparent texels: Hap1 is opaque)
    else:
        assert np.array_equal(theirs, ours)


def test_len2_sweep_shows_an_off_by_one_reciprocal(capsys):
    """Reaching a len2 is not enough: floor(3 * 2^24 / len2) off by one changes an index only for a texel that projects
    right at a third of the segment.  The numpy model of the oracle's colour encoder (checked against the oracle on the
    whole picture) recomputes every index of the two-colour sweep with m24 + 1 and m24 - 1: each must change an index
    for every len2 where some texel of the block's box can show it (an exhaustive search over the box decides that)."""
    px, reached = V.two_colour_boundary_blocks()
    pic = V.two_colour_picture()
    assert np.array_equal(V.blocks_of_picture(pic)[: len(px), :, :3].astype(np.int64), px)
    c0, c1, idx = _colour_fields(np.frombuffer(D.oracle_bc_encode(pic, L.FMT_DXT1), np.uint8).reshape(-1, 8))
    model = V.colour_block_model(px)
    n = len(px)
    assert np.array_equal(model["c0"], c0[:n]) and np.array_equal(model["c1"], c1[:n])
    assert np.array_equal(model["indices"], idx[:n])
    assert np.array_equal(np.unique(model["len2"]), V.encodable_len2()) and len(model["len2"]) == len(V.encodable_len2())
    shown = []
    for off, cols in ((1, slice(0, 6, 2)), (-1, slice(1, 6, 2))):
        changed = (V.colour_block_model(px, off)["indices"] != model["indices"]).any(axis=1)
        can = reached[:, cols].any(axis=1)
        assert np.array_equal(changed, can), (off, int((can & ~changed).sum()), int((changed & ~can).sum()))
        shown.append(int(changed.sum()))
    neither = int((~reached.any(axis=1)).sum())
    _report(capsys, "len2 values where m24 + 1 / m24 - 1 changes an index: %d / %d of %d; where no texel of the box can "
            "show either: %d (smallest len2 %s)" % (shown[0], shown[1], n, neither,
                                                   np.sort(model["len2"][~reached.any(axis=1)])[:6].tolist()))


def test_hapq_projection_coverage_is_measured(capsys):
    """The Hap Q encoder projects scaled (Co, Cg) pixels (bc_encode_core.hpp: s * m24, the wrap-around offset, v_dot2):
    its (scale, len2) values come from scaled boxes, not from the DXT1 set the two-colour sweep enumerates.  A numpy
    model of the oracle's YCoCg encoder, checked against the oracle on every block of the all-colour and scale-edge
    pictures, measures how many (scale, len2) values those pictures reach and at how many an off-by-one m24 would
    change an index."""
    counts = {}
    for name in ("all_colours", "scale_edges"):
        pic = V.ENCODE_PICTURES[name]()
        co, cg = V.ycocg(V.blocks_of_picture(pic)[..., :3].astype(np.int64))
        model = V.ycocg_block_model(co, cg)
        c0, c1, idx = _colour_fields(np.frombuffer(D.oracle_bc_encode(pic, L.FMT_YCOCG), np.uint8).reshape(-1, 16)[:, 8:])
        assert np.array_equal(model["c0"], c0) and np.array_equal(model["c1"], c1) and np.array_equal(model["indices"], idx)
        key = model["scale"] * (1 << 20) + model["len2"]
        live = model["c0"] != model["c1"]
        counts.setdefault("reached", set()).update(np.unique(key[live]).tolist())
        for off in (1, -1):
            changed = (V.ycocg_block_model(co, cg, off)["indices"] != model["indices"]).any(axis=1)
            counts.setdefault(off, set()).update(np.unique(key[live & changed]).tolist())
    per_scale = {s: sum(1 for k in counts["reached"] if k >> 20 == s) for s in (1, 2, 4)}
    assert all(per_scale.values())
    _report(capsys, "Hap Q projection: (scale, len2) values reached %d (scale 1 / 2 / 4: %d / %d / %d), of which m24 + 1 / "
            "m24 - 1 changes an index at %d / %d" % (len(counts["reached"]), per_scale[1], per_scale[2], per_scale[4],
                                                      len(counts[1]), len(counts[-1])))

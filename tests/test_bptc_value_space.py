"""The BPTC value-space sweeps (tests/_bptc_value_space.py) on the CPU.

(a) What the families reach, measured on the reference encoders' own intermediates (their TRACE hook) and asserted as
    conditions: a family that misses one fails.  The counts are printed (pytest -s shows them).
(b) The kernels' block functions are __host__ __device__: tests/c/bptc_block_host.hip compiles bc6h_encode.hip and
    bptc_encode.hip for the host (no device pass) and every picture of the sweeps comes out byte-identical to the
    definition, in both BC6H formats.  The device-only parts (v_rcp_f32 in rdiv, the ballots, partial waves) are
    tests/test_bptc_value_space_gpu.py's.

One condition of the plan cannot exist: (|n| + d / 2) mod d = d - 1 in the refit's rdiv.  With v = 64 - w the determinant
is d = 4096 * sum over pairs (w_i - w_j)^2 = 4096 D and every numerator is 4096 N, so the remainder is a multiple of 4096
(2048 when D is odd) and never d - 1.  Its reachable neighbour is asserted instead: the reduced remainder
(|N| + floor(D / 2)) mod D = D - 1 (odd D: (2 |N| + D) mod 2 D = 2 D - 2), the quotient one reduced step below an integer.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _bc6h_encode as E6
import _bc7_encode as E7
import _bptc_value_space as V
import _libs as L

ROOT = L.ROOT


# ------------------------------------------------------------------------------------------------ (a) coverage --
def _rdiv_cases(records, top):
    """counts of the rdiv cases over records of (n [N, C], d [N, 1])"""
    out = dict.fromkeys(("exact", "one_below", "clamped", "negative", "det0"), 0)
    for n, d in records:
        n, d = np.broadcast_arrays(n, d)
        ok = d > 0
        out["det0"] += int((d[:, 0] == 0).sum())
        n, d = n[ok], d[ok]
        g = np.where((d // 4096) % 2 == 1, 2048, 4096)
        assert (d % 4096 == 0).all() and (n % g == 0).all()
        rem = (np.abs(n) + d // 2) % d
        out["exact"] += int(((rem == 0) & (n != 0)).sum())
        out["one_below"] += int((rem == d - g).sum())
        out["clamped"] += int(((np.abs(n) + d // 2) // d > top).sum())
        out["negative"] += int((n < 0).sum())
    return out


def _shift_sides(records, base, signed):
    """{shift value v >= 1: [operands of 2^t - 1, of 2^t, of 2^t + 1 seen]}, t = base + v - 1.  Two values of the unsigned
    working domain ceil(64 h / 31) are never 2^t +- 1 apart for t >= 6: there 2^t - 2 and 2^t + 2 are the nearest and
    count instead; the signed format must show 2^t +- 1 themselves."""
    out = {}
    for operand, shift in records:
        operand = np.asarray(operand).reshape(-1)
        for v in range(1, 17 - base):
            edge = 1 << (base + v - 1)
            c = out.setdefault(v, [0, 0, 0])
            c[0] += int(((operand == edge - 1) | ((operand == edge - 2) & (not signed))).sum())
            c[1] += int((operand == edge).sum())
            c[2] += int(((operand == edge + 1) | ((operand == edge + 2) & (not signed))).sum())
    return out


_measured = {}


def measured6(signed):
    """family -> (blocks, modes [n], records, encoded blocks) of the reference on the BC6H families"""
    if signed not in _measured:
        out = {}
        for name, f in V.BC6H_FAMILIES.items():
            blocks = f(signed)
            (enc, _p, modes), rec = V.trace(E6, lambda: E6.encode_blocks(blocks, signed))
            out[name] = (blocks, modes, rec, enc)
        _measured[signed] = out
    return _measured[signed]


def measured7():
    """the same for the BC7 families"""
    if "bc7" not in _measured:
        out = {}
        for name, f in V.BC7_FAMILIES.items():
            blocks = f()
            (enc, _p, modes), rec = V.trace(E7, lambda: E7.encode_blocks(blocks))
            out[name] = (blocks, modes, rec, enc)
        _measured["bc7"] = out
    return _measured["bc7"]


@pytest.mark.parametrize("signed", [False, True])
def test_bc6h_families_reach_what_they_aim_at(signed):
    m = measured6(signed)
    top = V.TOP[signed]
    report = {}
    # every half pattern in every channel, solid and mixed
    blocks = m["all_halves"][0]
    for c in range(3):
        assert len(np.unique(blocks[:65536, :, c])) == 65536 and (blocks[:65536, 0, c] == blocks[:65536, 15, c]).all()
        assert len(np.unique(blocks[65536:, :, c])) == 65536
    # the shifts: cs and ps straight from a range, s from the endpoints' distance, each step from both sides
    rec = m["range_edges"][2]
    cs = _shift_sides([(r[np.arange(len(p)), p], s) for r, p, s in V.records_of(rec, "cs")], 11, signed)
    s = _shift_sides([(big, sh) for big, sh, _n, _d, _b in V.records_of(rec, "s")], 10, signed)
    asked = V.records_of(rec, "asked")[0][1]
    ps = _shift_sides([(r[asked], sh[asked]) for r, sh in V.records_of(rec, "ps")], 10, signed)
    report["cs"], report["s"], report["ps (asking blocks)"] = cs, s, ps
    for name, sides, last in (("cs", cs, 5), ("s", s, 6), ("ps", ps, 6)):
        for v in range(1, last + 1):
            assert sides[v][0] > 0 and sides[v][1] > 0, (name, v, sides[v])
            assert name == "s" or v == last or sides[v][2] > 0, (name, v, sides[v])    # (s: from endpoints, not a range)
    pivots = np.concatenate([p for _r, p, _s in V.records_of(rec, "cs")[:1]])
    rngs = V.records_of(rec, "cs")[0][0]
    assert set(pivots.tolist()) == {0, 1, 2} and (rngs[:, 0] == rngs[:, 1]).sum() > 0
    x = E6.to_working(E6.normalise(m["range_edges"][0], signed), signed)
    rs = V.reachable(signed)
    full = (x.min((1, 2)) == min(rs[0], 0)) & (x.max((1, 2)) == rs[-1]) & (x.min(1) == x.min((1, 2))[:, None]).all(1)
    assert full.sum() >= 5, full.sum()                                     # 0 / the lowest against the largest finite value
    # the delta limits of every transformed mode and channel: both limits and both first excluded values
    rec = m["delta_edges"][2]
    deltas = {}
    for c, bits, d in V.records_of(rec, "delta"):
        lim = 1 << (bits - 1)
        for what, v in (("lowest", -lim), ("highest", lim - 1), ("below", -lim - 1), ("above", lim)):
            deltas[(bits, c, what)] = deltas.get((bits, c, what), 0) + int((d == v).sum())
    report["deltas (bits, channel, value)"] = deltas
    for bits in (9, 8, 4, 6, 5):
        for c in range(3):
            for what in ("lowest", "highest", "below", "above"):
                assert deltas.get((bits, c, what), 0) > 0, (bits, c, what)
    # the refit's division
    cases = _rdiv_cases(V.records_of(m["refit_edges"][2], "rdiv"), top)
    report["rdiv"] = cases
    assert all(v > 0 for v in cases.values()), cases
    # blocks whose bytes the +1 and the -1 repair of the kernels' rdiv decide: the definition encoded with the kernels'
    # float quotient and one repair left out gives other bytes
    plus, minus = V.repair_decides(m["repair_blocks"][0], signed)
    report["blocks the rdiv repairs decide (+1, -1)"] = (int(plus.sum()), int(minus.sum()))
    assert plus.sum() > 0 and minus.sum() > 0, (plus.sum(), minus.sum())
    # ties
    rec = m["tie_blocks"][2]
    ties = {"index": 0, "quantiser": 0, "partition": 0, "candidates": 0}
    for _big, _s, num, den, b in V.records_of(rec, "s"):
        w = E6.W[b]
        for k in range(1, len(w)):
            ties["index"] += int(((128 * num == ((w[k - 1] + w[k]) * den)[:, None]) & (den > 0)[:, None]).sum())
    ties["quantiser"] = sum(int(t.sum()) for (t,) in V.records_of(rec, "quant_tie"))
    ties["partition"] = sum(int(t.sum()) for (t,) in V.records_of(rec, "score_tie"))
    cands = [c for (cl,) in V.records_of(rec, "candidates") for c in cl]          # the first four: the one-region modes
    best = np.min([np.where(v, e, 1 << 62) for _m, e, v in cands[:4]], 0)
    ties["candidates"] = int((sum(((e == best) & v).astype(int) for _m, e, v in cands[:4]) > 1).sum())
    report["ties"] = ties
    assert all(v > 0 for v in ties.values()), ties
    # every partition wins, and every anchor meets the swap taken and not taken in either region
    _blocks, modes, rec, part_blocks = m["partition_blocks"]
    two = np.isin(modes, E6.TWO_REGION)
    parts = (part_blocks[:, 9] >> 5) | ((part_blocks[:, 10] & 3) << 3)     # bits 77 .. 81
    assert set(parts[two].tolist()) == set(range(32)), sorted(set(range(32)) - set(parts[two].tolist()))
    assert (parts[two] == (np.arange(len(modes)) // 12)[two]).all()
    swaps = set()
    for _prec, anchor, swap in V.records_of(rec, "swap"):
        swaps |= set(zip(np.asarray(anchor)[two].tolist(), swap[two].tolist()))
    report["anchor swaps"] = sorted(swaps)
    assert swaps == {(a, t) for a in (0, 2, 8, 15) for t in (False, True)}, swaps
    # the trigger: the closest errors a bounded search finds on either side
    _tb, err = V.trigger_blocks(signed)
    report["trigger errors (threshold %d)" % E6.TWO_REGION_ERROR] = err.tolist()
    k = len(err) // 2
    assert (err[:k] <= E6.TWO_REGION_ERROR).all() and (err[k:] > E6.TWO_REGION_ERROR).all()
    # the last block that does not ask is there: a block at exactly the threshold (the kernel's > against >=); the
    # nearest asking block within two steps of a texel's error (about 32 each), every block within eight
    assert (err[:k] == E6.TWO_REGION_ERROR).any(), err
    assert err[k] - E6.TWO_REGION_ERROR <= 64 and (np.abs(err - E6.TWO_REGION_ERROR) <= 256).all(), err
    # every mode wins at least 64 blocks
    wins = {mode: sum(int((mm == mode).sum()) for _b, mm, _r, _e in m.values()) for mode in E6.MODES_USED}
    report["mode wins"] = {hex(k): v for k, v in wins.items()}
    print("\nBC6H %s" % ("signed" if signed else "unsigned"))
    for k, v in report.items():
        print("  %s: %s" % (k, v))
    assert all(v >= 64 for v in wins.values()), wins


def test_bc7_families_reach_what_they_aim_at():
    report = {}
    m = measured7()
    fam, modes, rec = ({name: v[i] for name, v in m.items()} for i in range(3))
    for c in range(4):
        assert len(np.unique(fam["all_bytes"][:256, :, c])) == 256 and len(np.unique(fam["all_bytes"][512:, :, c])) == 256
    a = fam["alpha_edges"][..., 3]
    assert ((a == 254).sum(1) == 1).any() and (a == 254).all(1).any() and (a == 255).all(1).any()
    r = rec["low_entropy"]
    ties = {"p-bit mode 6": 0, "p-bit mode 1": 0, "index": 0, "quantiser": 0, "partition": 0, "errors 6 = 1": 0, "errors 6 = 5": 0}
    for kind, t in V.records_of(r, "p_tie"):
        ties["p-bit mode %d" % kind] += int(t.sum())
    for num, den, b in V.records_of(r, "index"):
        w = E7.W[b]
        for k in range(1, len(w)):
            ties["index"] += int(((128 * num == ((w[k - 1] + w[k]) * den)[:, None]) & (den > 0)[:, None]).sum())
    ties["quantiser"] = sum(int(t.sum()) for (t,) in V.records_of(r, "quant_tie"))
    ties["partition"] = sum(int(t.sum()) for (t,) in V.records_of(r, "score_tie"))
    opaque, e6, e1, e5 = V.records_of(r, "errors")[0]
    ties["errors 6 = 1"], ties["errors 6 = 5"] = int((opaque & (e6 == e1)).sum()), int((~opaque & (e6 == e5)).sum())
    report["ties"] = ties
    assert all(v > 0 for v in ties.values()), ties
    cases = dict.fromkeys(("n <= 0", "255 and beyond", "exact", "det0"), 0)
    for n, d in V.records_of(r, "rdiv"):
        n, d = np.broadcast_arrays(n, d)
        cases["det0"] += int((d[:, 0] == 0).sum())
        n, d = n[d > 0], d[d > 0]
        cases["n <= 0"] += int((n <= 0).sum())
        cases["255 and beyond"] += int(((n > 0) & ((n + d // 2) // d >= 255)).sum())
        cases["exact"] += int(((n > 0) & ((n + d // 2) % d == 0)).sum())
    report["rdiv"] = cases
    assert all(v > 0 for v in cases.values()), cases
    # blocks whose bytes the +1 and the -1 repair decide
    plus, minus = V.repair_decides(fam["repair_blocks"], "bc7")
    report["blocks the rdiv repairs decide (+1, -1)"] = (int(plus.sum()), int(minus.sum()))
    assert plus.sum() > 0 and minus.sum() > 0, (plus.sum(), minus.sum())
    blocks, one = m["partition_blocks"][3], modes["partition_blocks"] == 1
    parts = blocks[:, 0] >> 2
    assert set(parts[one].tolist()) == set(range(64)), sorted(set(range(64)) - set(parts[one].tolist()))
    swaps = set()
    for b, anchor, swap in V.records_of(rec["partition_blocks"], "swap"):
        if b == 3:
            swaps |= set(zip(np.asarray(anchor)[one].tolist(), swap[one].tolist()))
    report["anchor swaps"] = sorted(swaps)
    assert swaps == {(a, t) for a in (0, 2, 6, 8, 15) for t in (False, True)}, swaps
    wins = {mode: sum(int((mm == mode).sum()) for mm in modes.values()) for mode in E7.MODES_USED}
    report["mode wins"] = wins
    print("\nBC7")
    for k, v in report.items():
        print("  %s: %s" % (k, v))
    assert all(v >= 64 for v in wins.values()), wins


def test_the_wave_layouts_put_the_lone_lanes_where_they_say():
    quiet, loud = np.zeros((2, 16, 4), np.uint8), np.ones((3, 16, 4), np.uint8)
    px, flags = V.wave_layout(quiet, loud, rows=3)
    assert (px[:, 0, 0].astype(bool) == flags).all() and V.WAVE_ROW % 64 == 37 and (4 * V.WAVE_ROW) % 256
    row = flags[: V.WAVE_ROW]
    waves = [row[i: i + 64] for i in range(0, V.WAVE_ROW, 64)]
    assert [np.flatnonzero(w).tolist() for w in (waves[0], waves[1], waves[2], waves[4])] == [[], [0], [63], [36]]
    assert waves[3].all() and len(waves[4]) == 37
    for signed in (False, True):
        blocks, err = V.trigger_blocks(signed)
        pic = V.trigger_picture(signed)
        got = V.best_one_region_error(V.blocks_of_picture(pic), signed) > E6.TWO_REGION_ERROR
        assert (got == np.concatenate([row] * 4)).all()
        # a lane that does not ask would get other bytes from the two-region code its wave runs for a neighbour
        k = len(blocks) // 2
        assert np.isin(E6.encode_blocks(blocks[:k], signed, threshold=-1)[2], E6.TWO_REGION).all()
        assert np.isin(E6.encode_blocks(blocks[:k], signed)[2], E6.ONE_REGION).all()
    pic = V.bc7_wave_picture()
    blocks = V.blocks_of_picture(pic)
    alpha = (blocks[..., 3] != 255).any(1)
    assert (alpha == np.concatenate([row, row, ~row, ~row])).all()
    # the same for the mode-1 and mode-5 ballots: every opaque lane is a mode-1 block, which no block with alpha can be,
    # and the lanes with alpha hold mode-5 blocks, which no opaque block can be
    modes = E7.encode_blocks(blocks)[2]
    assert (modes[~alpha] == 1).all() and set(modes[alpha].tolist()) == {5, 6}


# ---------------------------------------------------------------------- (b) the kernels' block functions on the host --
@pytest.fixture(scope="module")
def host_blocks(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bptc_host") / "libbptc_block_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "bptc_block_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.bc6h_encode_blocks.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lib.bc7_encode_blocks.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.bc6h_encode_blocks.restype = lib.bc7_encode_blocks.restype = None
    return lib


def _first_difference(got, want, inputs, what):
    bad = np.flatnonzero((got != want).any(1))
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d blocks differ; first: block %d\n  input      %s\n  kernel     %s\n  definition %s" % (
            what, len(bad), len(got), i, inputs[i].tolist(), got[i].tobytes().hex(), want[i].tobytes().hex()))


@pytest.mark.parametrize("signed", [False, True])
def test_bc6h_block_function_on_the_host_is_the_definition(host_blocks, signed):
    for name, pic in V.bc6h_pictures(signed).items():
        blocks = np.ascontiguousarray(V.blocks_of_picture(pic))
        got = np.zeros((len(blocks), 16), np.uint8)
        host_blocks.bc6h_encode_blocks(blocks.ctypes.data, len(blocks), int(signed), got.ctypes.data)
        if name in measured6(signed):                                      # block i of a family is block i of its picture
            want = V.cycle_to(measured6(signed)[name][3], len(blocks))
        else:
            want = np.frombuffer(E6.encode(pic, signed), np.uint8).reshape(-1, 16)
        _first_difference(got, want, blocks, "bc6h_encode.hip on the host, %s, signed %s" % (name, signed))


def test_bc7_block_function_on_the_host_is_the_definition(host_blocks):
    for name, pic in V.bc7_pictures().items():
        blocks = np.ascontiguousarray(V.blocks_of_picture(pic))
        got = np.zeros((len(blocks), 16), np.uint8)
        host_blocks.bc7_encode_blocks(blocks.ctypes.data, len(blocks), got.ctypes.data)
        if name in measured7():
            want = V.cycle_to(measured7()[name][3], len(blocks))
        else:
            want = np.frombuffer(E7.encode(pic), np.uint8).reshape(-1, 16)
        _first_difference(got, want, blocks, "bptc_encode.hip on the host, " + name)


# ------------------------------------------------------------------------------------------- decode block sets --
def _pin(blocks):
    """every 97th block, or all of a set of at most 64"""
    return range(len(blocks)) if len(blocks) <= 64 else range(0, len(blocks), 97)


@pytest.mark.parametrize("signed", [False, True])
def test_bc6h_decode_sets_walk_every_code_and_the_array_decoder_is_the_scalar_one(signed):
    import _bc6h as H6
    sets = V.bc6h_decode_sets()
    assert len(sets) == 15
    for mi, (mv, regions, transformed, prec, deltas, _l) in enumerate(H6.MODES):
        blocks = sets["mode%02x" % mv]
        assert len(blocks) == 1 << prec
        fields = [H6.fields(b.tobytes()) for b in blocks[:: max(1, len(blocks) >> 10)]] if prec > 12 else [H6.fields(b.tobytes()) for b in blocks]
        for name in H6.FIELDS:
            seen = {f[name] for f in fields}
            width = max([max(fb) + 1 for n, fb in H6.layout(mi) if n == name] or [0])
            if width and prec <= 12:
                assert seen == set(range(1 << width)), (hex(mv), name, len(seen))        # every code of every field
        bits = V.bits_of(blocks)
        if prec > 12:                                                                    # 0x0F: the base fields from the bytes
            rw = V._field(bits, 5, 10) | (sum(bits[:, 39 + k].astype(np.int64) << (15 - k) for k in range(6)))
            assert len(np.unique(rw)) == 65536
        else:
            rw = np.array([f["rw"] for f in fields])
        if regions == 2:
            parts = {(int.from_bytes(b.tobytes(), "little") >> 77) & 31 for b in blocks}
            assert parts == set(range(min(32, len(blocks))))
        # every weight meets the lowest, the highest and a middle base code (the unquantiser's three cases)
        cls = np.where(rw == 0, 0, np.where(rw == (1 << prec) - 1, 2, 1))
        met = set(zip(np.repeat(cls, 16).tolist(), V.bc6h_indices(bits, regions).ravel().tolist()))
        assert met == {(c, w) for c in range(3) for w in range(8 if regions == 2 else 16)}, (hex(mv), len(met))
    got = {k: V.decode_bc6h_blocks(b, signed) for k, b in sets.items()}
    for k, b in sets.items():
        for i in _pin(b):
            assert (got[k][i] == np.array(H6.decode_block(b[i].tobytes(), signed))).all(), (k, i)
    # the pairs: every weight between 0 and 0xFFFF (unsigned), -0x7FFF and 0x7FFF (signed)
    ends = {tuple(H6.endpoints(b.tobytes(), signed)[3][k][0] for k in (0, 1)) for b in sets["pairs"]}
    assert ((0, 1023) in ends and (1023, 0) in ends) if not signed else ((-511, 511) in ends and (511, -511) in ends)
    p = got["pairs"]
    lo, hi = (0, (0xFFFF * 31) >> 6) if not signed else (0x8000 | ((0x7FFF * 31) >> 5), (0x7FFF * 31) >> 5)
    rows = p[:16] if not signed else p[32:48]
    # (texel 0 is the anchor: its eight indices; the block set's second half holds the pair the other way round)
    assert all(len(np.unique(rows[:, t, 0])) == (16 if t else 8) for t in range(16)) and lo in rows[..., 0] and hi in rows[..., 0]
    print("\nBC6H decode sets (%s): %s" % ("signed" if signed else "unsigned", {k: len(v) for k, v in sets.items()}))


def test_bc7_decode_sets_walk_every_code_and_the_array_decoder_is_the_scalar_one():
    import _bptc as H7
    sets = V.bc7_decode_sets()
    for mode, (ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2) in enumerate(H7.MODES):
        blocks = sets["mode%d" % mode]
        bits = V.bits_of(blocks)
        pos = mode + 1
        assert set(V._field(bits, pos, pb).tolist()) == set(range(1 << pb))
        rot_sel = set(zip(V._field(bits, pos + pb, rb).tolist(), V._field(bits, pos + pb + rb, isb).tolist()))
        assert len(rot_sel) == (1 << rb) * (1 << isb)
        pos += pb + rb + isb
        npb = 2 * ns if epb else ns if spb else 0
        ppos = pos + 2 * ns * (3 * cb + ab)
        pbits = V._field(bits, ppos, npb)
        for wd, count in ((cb, 6 * ns), (ab, 2 * ns if ab else 0)):
            for _ in range(count):
                code = V._field(bits, pos, wd)
                if npb:                                                    # every code with each p-bit pattern
                    assert len(set(zip(code.tolist(), (pbits & 3).tolist()))) == (1 << wd) * (4 if npb > 1 else 2), (mode, pos)
                else:
                    assert set(code.tolist()) == set(range(1 << wd)), (mode, pos)
                pos += wd
        got = V.decode_bc7_blocks(blocks)
        for i in _pin(blocks):
            assert (got[i] == np.array(H7.decode_block(blocks[i].tobytes()))).all(), (mode, i)
    print("\nBC7 decode sets: %s" % {k: len(v) for k, v in sets.items()})

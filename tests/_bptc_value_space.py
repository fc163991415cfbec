"""Deterministic sweeps over the edges of the BC6H and BC7 encoders' definitions (tests/_bc6h_encode.py,
tests/_bc7_encode.py; kernels hap_amd/csrc/bc6h_encode.hip, bptc_encode.hip).

Pictures of the real pipelines reach every mode, but hardly the places where one comparison or one rounding decides:
the +-1 repair of the kernels' reciprocal division, the shifts chosen by the bit length of a range, the limits of the
transformed modes' deltas, the two-region trigger and the ballots around it, ties.  These generators aim at them; what
they reach is measured on the reference (trace(), conditions in tests/test_bptc_value_space.py), never on the kernel.

BC6H families (blocks uint16 [n, 16, 4] of half patterns, alpha is noise: the encoder ignores it), per format:
  all_halves        every one of the 65 536 patterns in R, G and B: once in solid blocks, once eight to a block among
                    ordinary values
  range_edges       the widest working-domain range of a block 2^k - 2 .. 2^k + 2 (k = 1 .. 15; the
                    unsigned domain ceil(64 h / 31) has no two values 2^k +- 1 apart for k >= 6, so there 2^k - 2 is the
                    low side of the step) and the largest there is; at the bottom, the middle, the top of the domain and
                    (signed) across zero; R, G, B as the pivot and a tie of R and G; two-valued (the one-region modes fit them: the range reaches the index shift s
                    unchanged) and spread (they ask for two regions: the range reaches the partition shift ps)
  delta_edges       per transformed mode and channel, endpoint distances around the delta limit times the code step
  refit_edges       clusters whose means end in .5 (the rounding division exact), small regions (quotients one reduced
                    step below an integer), blocks against the top and the bottom of the domain (clamps, n < 0), solid
                    blocks (det = 0)
  repair_blocks     ramps with noise whose refit is solved as a lattice over two texels' values (_lattice) for quotients
                    at which the float quotient the kernels' rdiv starts from is one too low or one too high
                    (float_quotient_error) on a quantiser boundary: the +1 and the -1 repair decide the bytes
  tie_blocks        short integer ramps (index-rule equalities), endpoints on quantiser midpoints, masks with equal
                    partition scores, solid blocks (equal candidate errors)
  partition_blocks  per partition: its two regions as two clusters with crossed gradients, either direction in either
                    region (the anchor swap taken and not taken), at three sizes up to 0 against the largest finite value
  trigger_blocks    blocks whose best one-region error is the closest a bounded search finds below or at, and above,
                    TWO_REGION_ERROR
trigger_picture() lays them out by wave: no lane asking, lane 0 alone, lane 63 alone, all lanes, and in the partial last
wave of a row the last live lane alone; non-asking lanes hold blocks that two regions would encode better.

BC7 families (uint8 [n, 16, 4]): every 8-bit value per channel solid and mixed, alpha 254 / 255 edges, low-entropy blocks
(p-bit, index, score and error ties; rdiv at 0, 255 and exact quotients), blocks constructed like repair_blocks whose
bytes rdiv's +1 and -1 repair decide, all 64 partitions with either gradient
direction per region, and a wave-layout picture of opaque and alpha blocks like the trigger picture.

Everything is computed here (numpy, fixed seeds); nothing is read from disk.  Block i of a family is block i of its
picture (picture_of_blocks of tests/_value_space.py works on any dtype).
"""
import numpy as np

import _bc6h as H6
import _bc6h_encode as E6
import _bc7_encode as E7
import _bptc as H7
from _value_space import blocks_of_picture, cycle_to
from _value_space import picture_of_blocks as _whole_rows

ROW = 256                             # blocks per picture row of the family pictures
WAVE_ROW = 4 * 64 + 37                # blocks per row of the wave-layout pictures: four whole waves and 37 lanes
TOP = {False: 0xFFFF, True: 0x7FFF}


def picture_of_blocks(px, row=ROW):
    """[n, 16, 4] -> picture of whole rows of `row` blocks, the blocks repeated from the first to fill the last row"""
    return _whole_rows(cycle_to(px, -(-len(px) // row) * row), row=row)


# --------------------------------------------------------------------------------------- working domain <-> halves --
def _table(signed):
    mag = np.arange(0x7C00, dtype=np.int64)
    return (32 * mag + 30) // 31 if signed else (64 * mag + 30) // 31


def reachable(signed):
    """sorted working values that some half pattern normalises to"""
    t = _table(signed)
    return np.unique(np.concatenate([-t, t])) if signed else t


def snap(x, signed):
    """the largest reachable working value <= x (elementwise; x at or above the smallest one)"""
    r = reachable(signed)
    return r[np.clip(np.searchsorted(r, np.asarray(x, np.int64), side="right") - 1, 0, len(r) - 1)]


def patterns(x, signed):
    """reachable working values -> half patterns (uint16)"""
    x = np.asarray(x, np.int64)
    t = _table(signed)
    mag = np.searchsorted(t, np.abs(x))
    assert (t[np.clip(mag, 0, len(t) - 1)] == np.abs(x)).all(), "not a reachable working value"
    return (mag | np.where(x < 0, 0x8000, 0)).astype(np.uint16)


def exact_pair(r, near, signed):
    """(lo, lo + r), both reachable, lo the first such at or above `near` (None if there is none within 4096 values)"""
    rs = reachable(signed)
    i = np.searchsorted(rs, near)
    lo = rs[i: i + 4096]
    ok = np.isin(lo + r, rs)
    return (int(lo[ok][0]), int(lo[ok][0]) + r) if ok.any() else None


def with_alpha(px, rng):
    """[n, 16, 3] patterns -> [n, 16, 4] with noise in alpha"""
    a = rng.integers(0, 65536, px.shape[:2] + (1,))
    return np.concatenate([px, a], -1).astype(np.uint16)


def _blocks6(x, signed, rng):
    return with_alpha(patterns(x, signed), rng)


# --------------------------------------------------------------------------------------------------- BC6H families --
def all_halves(signed=False):
    """(the same patterns in both formats; `signed` is accepted for uniformity)"""
    rng = np.random.default_rng(0xA11)
    p = np.arange(65536, dtype=np.int64)
    solid = np.stack([p, (p + 21845) & 0xFFFF, (p + 43690) & 0xFFFF], -1)[:, None, :].repeat(16, 1)
    j = np.arange(8192)
    mixed = rng.integers(0x3000, 0x4000, (8192, 16, 3))
    t = (np.arange(8)[None, :] * 2 + j[:, None]) % 16                     # eight texels, rotating
    v = 8 * j[:, None] + np.arange(8)[None, :]
    for c, off in enumerate((0, 21845, 43690)):
        mixed[j[:, None], t, c] = (v + off) & 0xFFFF
    return with_alpha(np.concatenate([solid, mixed]), rng)


def range_edges(signed):
    rng = np.random.default_rng(0xED6E + signed)
    rs = reachable(signed)
    lo_dom, hi_dom = int(rs[0]), int(rs[-1])
    ranges = sorted({r for k in range(1, 16) for r in ((1 << k) - 2, (1 << k) - 1, 1 << k, (1 << k) + 1, (1 << k) + 2) if r > 0} | {hi_dom - lo_dom, hi_dom})
    out = []
    for r in ranges:
        places = [lo_dom, (lo_dom + hi_dom - r) // 2, hi_dom - r - 600]
        if signed:
            places.append(-(r // 2) - 1)
        for place in places:
            pair = exact_pair(r, max(lo_dom, place), signed)
            if pair is None or pair[1] > hi_dom:
                continue
            lo, hi = pair
            for pivot in (0, 1, 2, 3):                                      # 3: R and G tie
                for spread in (False, True):
                    x = np.empty((16, 3), np.int64)
                    mask = rng.integers(0, 2, 16).astype(bool)
                    mask[rng.integers(0, 16)] = True
                    mask[(np.flatnonzero(mask)[0] + 5) % 16] = False
                    for c in range(3):
                        full = c == pivot or (pivot == 3 and c < 2)
                        clo, chi = (lo, hi) if full else (int(snap(lo + r // 8, signed)), int(snap(lo + r // 2, signed)))
                        if spread:
                            v = snap(rng.integers(clo, chi + 1, 16), signed)
                            v = np.clip(v, clo, chi)
                            v[rng.permutation(16)[:2]] = (clo, chi)
                        else:
                            v = np.where(mask, chi, clo)
                        x[:, c] = v
                    out.append(x)
    # 0 against the largest finite value in all three channels at once
    ends = [(0, hi_dom)] + ([(lo_dom, hi_dom), (lo_dom, 0)] if signed else [])
    for a, b in ends:
        for m in (0x00FF, 0xCCCC, 0x8000, 0x7FFF, 0x5A5A):
            mask = np.array([(m >> t) & 1 for t in range(16)], bool)
            out.append(np.where(mask[:, None], b, a) * np.ones((16, 3), np.int64))
    return _blocks6(np.array(out), signed, rng)


TRANSFORMED = ((0x07, 1, 11, 9), (0x0B, 1, 12, 8), (0x0F, 1, 16, 4), (0x01, 2, 7, 6), (0x00, 2, 10, 5))
_MASKS = E6.P2_MASKS


def delta_edges(signed, per_case=320):
    """Endpoint distances of (limit - 2 .. limit + 2) code steps on one channel, rising and falling from texel 0: the
    stored delta lands on both limits and beyond them."""
    rng = np.random.default_rng(0xDE17A + signed)
    rs = reachable(signed)
    lo_dom, hi_dom = int(rs[0]), int(rs[-1])
    out = []
    for _mode, regions, prec, dbits in TRANSFORMED:
        step, limit = 1 << (16 - prec), 1 << (dbits - 1)
        for c in range(3):
            for i in range(per_case):
                r = int(rng.integers((limit - 2) * step, (limit + 2) * step + 1))
                lo = int(rng.integers(lo_dom + 64, hi_dom - r - 64))
                rising = bool(i & 1)
                x = np.empty((16, 3), np.int64)
                if regions == 1:
                    g = np.sort(rng.integers(0, 1025, 16))
                    g[0], g[-1] = 0, 1024
                    g = g if rising else g[::-1]
                    for cc in range(3):
                        rr = r if cc == c else r // (4 + cc)
                        base = lo if cc == c else int(rng.integers(lo_dom + 64, hi_dom - rr - 64))
                        x[:, cc] = base + (g * rr) // 1024
                else:
                    m = _MASKS[int(rng.integers(0, 32))]
                    w = int(rng.integers(4, 12)) * step
                    for cc in range(3):
                        base = lo if cc == c else int(rng.integers(lo_dom + 64 + w, hi_dom - w - 64))
                        other = r if cc == c else 0
                        # the regions' own gradients run in different channels: one region cannot hold both
                        g0 = rng.integers(0, w + 1, 16) if cc == (c + 1) % 3 else 0
                        g1 = rng.integers(0, w + 1, 16) if cc == (c + 2) % 3 else 0
                        a, b = (base, base + other) if rising else (base + other, base)
                        x[:, cc] = np.where(m, b + g1, a + g0)
                out.append(np.clip(x, lo_dom, hi_dom))
    return _blocks6(snap(np.array(out), signed), signed, rng)


def refit_edges(signed, n=1536):
    rng = np.random.default_rng(0x4EF17 + signed)
    rs = reachable(signed)
    lo_dom, hi_dom = int(rs[0]), int(rs[-1])
    out = []
    # two clusters far apart, members a few steps from each other: each endpoint is a cluster's mean
    for i in range(n):
        k = int(rng.integers(1, 16))
        mask = np.zeros(16, bool)
        mask[rng.permutation(16)[:k]] = True
        a = int(rng.integers(lo_dom, hi_dom - 9000))
        b = int(rng.integers(a + 4000, hi_dom - 16))
        x = np.where(mask[:, None], b, a) + rng.integers(0, 3, (16, 3)) * (i % 3 + 1)
        out.append(x)
    # small regions: few texels, small determinants
    for i in range(n):
        m = _MASKS[(2, 4, 8, 11, 15, 17, 18, 20, 22, 24)[i % 10]]
        a = rng.integers(lo_dom, hi_dom - 3000, 3)
        x = np.where(m[:, None], a + rng.integers(0, 2600, (16, 3)), a + 1200 + rng.integers(0, 200, (16, 3)))
        out.append(x)
    # against the ends of the domain: a refit that overshoots is clamped (or, unsigned, has n < 0)
    for i in range(n):
        end = (hi_dom, lo_dom)[i & 1]
        sign = -1 if end == hi_dom else 1
        amp = int(rng.integers(2, 4000))
        x = end + sign * (rng.integers(0, amp, (16, 3)) * (rng.integers(0, 4, (16, 1)) == 0))
        out.append(x)
    x = np.clip(np.array(out), lo_dom, hi_dom)
    solid = rs[rng.integers(0, len(rs), (64, 1, 3))].repeat(16, 1)
    return _blocks6(np.concatenate([snap(x, signed), solid]), signed, rng)


def tie_blocks(signed, n=1024):
    rng = np.random.default_rng(0x71E5 + signed)
    rs = reachable(signed)
    lo_dom, hi_dom = int(rs[0]), int(rs[-1])
    out = []
    # short ramps: few distinct projections, so 128 num meets (W[k-1] + W[k]) den
    for i in range(n):
        r = int(rng.integers(2, 400))
        a = rng.integers(lo_dom, hi_dom - r - 8, 3)
        g = rng.integers(0, r + 1, 16)
        g[rng.permutation(16)[:2]] = (0, r)
        x = a + np.stack([g, (g * (i % 3)) // 2, np.zeros(16, np.int64)], -1)[:, np.array([i % 3, (i + 1) % 3, (i + 2) % 3])]
        out.append(x)
    # endpoints on the midpoints of the 10-, 11- and 12-bit quantisers (multiples of 64, 32, 16; two-valued blocks keep them)
    mult = rs[(rs % 64 == 0)]
    for i in range(n):
        a, b = np.sort(mult[rng.integers(0, len(mult), (2, 3))], 0)
        mask = rng.integers(0, 2, 16).astype(bool)
        mask[0], mask[15] = bool(i & 1), not (i & 1)
        out.append(np.where(mask[:, None], b, a))
    # two values on a mask that several partitions split equally well
    for i in range(n):
        mask = np.array([(m >> t) & 1 for m in [int(rng.integers(1, 0xFFFF))] for t in range(16)], bool)
        a = rng.integers(lo_dom, hi_dom - 5000, 3)
        x = np.where(mask[:, None], a + rng.integers(500, 5000, 3), a) + rng.integers(0, 2, (16, 3)) * int(rng.integers(0, 900))
        out.append(x)
    x = np.clip(np.array(out), lo_dom, hi_dom)
    solid = rs[rng.integers(0, len(rs), (64, 1, 3))].repeat(16, 1)
    solid[:3] = np.array([0, lo_dom, hi_dom])[:, None, None]                # every one-region mode holds these equally well
    return _blocks6(np.concatenate([snap(x, signed), solid]), signed, rng)


def partition_blocks(signed):
    rng = np.random.default_rng(0x9A47 + signed)
    rs = reachable(signed)
    lo_dom, hi_dom = int(rs[0]), int(rs[-1])
    out = []
    for p in range(32):
        m = _MASKS[p]
        order = np.where(m, np.cumsum(m) - 1, np.cumsum(~m) - 1)            # a texel's rank inside its region
        count = np.where(m, m.sum(), (~m).sum())
        for size in (900, 12000, hi_dom - lo_dom):
            a = lo_dom if size == hi_dom - lo_dom else int(rng.integers(lo_dom, hi_dom - size))
            b = a + size
            w = min(size // 3, 3000)
            for f0 in (False, True):
                for f1 in (False, True):
                    flip = np.where(m, f1, f0)
                    g = (np.where(flip, count - 1 - order, order) * w) // np.maximum(count - 1, 1)
                    x = np.empty((16, 3), np.int64)
                    x[:, 0] = np.where(m, b - g, a)                         # region 1's gradient in R (from the top)
                    x[:, 1] = np.where(m, b, a + g)                         # region 0's in G
                    x[:, 2] = np.where(m, b, a)
                    out.append(x)
    return _blocks6(snap(np.array(out), signed), signed, rng)


def best_one_region_error(blocks, signed):
    """the error the two-region trigger compares, from the reference"""
    h = E6.normalise(blocks, signed)
    x = E6.to_working(h, signed)
    err = None
    for _mode, _w, _d, e, valid in E6._one_region(x, h, signed):
        err = e if err is None else np.where(valid & (e < err), e, err)
    return err


_trigger_cache = {}


def _exactly_at_trigger(near, signed, reach=24):
    """Directed search from blocks near the trigger: one channel of one texel moved by up to `reach` half patterns either
    way; the variants whose best one-region error is exactly TWO_REGION_ERROR (the last block that does not ask)."""
    t, c, k = np.meshgrid(np.arange(16), np.arange(3), np.concatenate([np.arange(-reach, 0), np.arange(1, reach + 1)]), indexing="ij")
    t, c, k = t.ravel(), c.ravel(), k.ravel()
    found = []
    for base in near:
        v = np.repeat(base[None], len(t), 0)
        p = v[np.arange(len(t)), t, c].astype(np.int64)
        mag = np.clip((p & 0x7FFF) + k, 0, 0x7BFF)
        v[np.arange(len(t)), t, c] = (p & 0x8000) | mag
        hit = np.flatnonzero(best_one_region_error(v, signed) == E6.TWO_REGION_ERROR)
        if len(hit):
            found.append(v[hit[0]])
        if len(found) >= 2:
            break
    return np.array(found, np.uint16).reshape(-1, 16, 4)


def trigger_blocks(signed, pool=6144):
    """(blocks [2 * k, 16, 4]: k not asking then k asking, their errors): the k = 4 blocks of a pool of two-cluster
    blocks with noise of rising size whose best one-region error is nearest to TWO_REGION_ERROR on either side; the
    first of them is a block at exactly TWO_REGION_ERROR, from a directed search around the nearest ones.  The blocks
    that do not ask are ones that two regions would encode better: their bytes change if the trigger is taken for them."""
    if signed not in _trigger_cache:
        rng = np.random.default_rng(0x7416 + signed)
        rs = reachable(signed)
        lo_dom, hi_dom = int(rs[0]), int(rs[-1])
        x = np.empty((pool, 16, 3), np.int64)
        for i in range(pool):
            m = _MASKS[i % 32]
            a = rng.integers(lo_dom + 100, hi_dom - 4000, 3)
            amp = 40 + (i * 700) // pool
            x[i] = np.where(m[:, None], a + rng.integers(200, 900, 3), a) + rng.integers(0, amp, (16, 3))
        blocks = _blocks6(snap(x, signed), signed, rng)
        err = best_one_region_error(blocks, signed)
        below = np.flatnonzero(err <= E6.TWO_REGION_ERROR)
        above = np.flatnonzero(err > E6.TWO_REGION_ERROR)
        below = below[np.argsort(E6.TWO_REGION_ERROR - err[below], kind="stable")]
        above = above[np.argsort(err[above] - E6.TWO_REGION_ERROR, kind="stable")[:4]]
        at = _exactly_at_trigger(blocks[np.concatenate([below[:24], above])], signed)
        quiet = np.concatenate([at, blocks[below[:64]]])
        quiet = quiet[np.isin(E6.encode_blocks(quiet, signed, threshold=-1)[2], E6.TWO_REGION)][:4]
        picked = np.concatenate([quiet, blocks[above]])
        _trigger_cache[signed] = (picked, best_one_region_error(picked, signed))
    return _trigger_cache[signed]


def wave_layout(quiet, loud, rows=4):
    """Block order of a picture WAVE_ROW blocks wide: per row, wave 0 all quiet, wave 1 loud at lane 0 only, wave 2 at
    lane 63 only, wave 3 all loud, the 37-lane last wave loud at lane 36 only.  quiet / loud: [k, 16, 4] each; row y
    starts its rotation through them at y.  -> (blocks [rows * WAVE_ROW, 16, 4], loud flags)"""
    flags = np.zeros(WAVE_ROW, bool)
    flags[64] = flags[191] = flags[WAVE_ROW - 1] = True
    flags[192:256] = True
    out, marks = [], []
    for y in range(rows):
        i = np.arange(WAVE_ROW) + y
        out.append(np.where(flags[:, None, None], loud[i % len(loud)], quiet[i % len(quiet)]))
        marks.append(flags)
    return np.concatenate(out), np.concatenate(marks)


def trigger_picture(signed):
    blocks, _err = trigger_blocks(signed)
    k = len(blocks) // 2
    px, _flags = wave_layout(blocks[:k], blocks[k:])
    return picture_of_blocks(px, row=WAVE_ROW)


def float_quotient_error(n, d, top):
    """The kernels' rdiv takes trunc(float(n2) * (1.0f / float(d))), n2 = |n| + d / 2, and repairs it by one: this is that
    float quotient minus the true one (0 where d <= 0 or the early clamp answers), in numpy's float32."""
    n, d = np.broadcast_arrays(np.asarray(n, np.int64), np.asarray(d, np.int64))
    safe = np.where(d > 0, d, 1)
    n2 = np.abs(n) + safe // 2
    q = (n2.astype(np.float32) * (np.float32(1.0) / safe.astype(np.float32))).astype(np.int64)
    return np.where((d > 0) & (n2 < (top + 1) * safe), np.clip(q, 0, top + 1) - n2 // safe, 0)


def kernel_rdiv(n, d, top, unsigned_zero, plus=True, minus=True):
    """The kernels' rdiv as they compute it on the host (float quotient, then the repairs), with either repair left out on
    request; unsigned_zero: n < 0 gives 0 (BC6H unsigned, BC7), else the sign is kept."""
    n, d = np.broadcast_arrays(np.asarray(n, np.int64), np.asarray(d, np.int64))
    safe = np.where(d > 0, d, 1)
    n2 = np.abs(n) + safe // 2
    q = np.clip((n2.astype(np.float32) * (np.float32(1.0) / safe.astype(np.float32))).astype(np.int64), 0, top + 1)
    high, low = q * safe > n2, (q + 1) * safe <= n2
    q = q - (high & minus) + (low & ~high & plus)
    q = np.where(n2 >= (top + 1) * safe, top, np.minimum(q, top))
    return np.where(n < 0, 0, q) if unsigned_zero else np.sign(n) * q


def _encode_with(module, encode, rdiv):
    old = module._rdiv
    module._rdiv = rdiv
    try:
        return encode()
    finally:
        module._rdiv = old


def repair_decides(blocks, kind):
    """(bool [n], bool [n]): the blocks whose encoded bytes change when rdiv loses its +1 repair, its -1 repair; kind:
    False / True (BC6H unsigned / signed) or "bc7".  The definition is encoded with kernel_rdiv in place of its exact
    division: with both repairs it gives the definition's bytes (asserted), without one the difference is what that
    repair decides."""
    if kind == "bc7":
        module, top, enc = E7, 255, (lambda: E7.encode_blocks(blocks)[0])
        def make(**kw):
            return lambda n, d: kernel_rdiv(np.where(n < 0, 0, n), d, 255, True, **kw)
    else:
        module, top, enc = E6, TOP[kind], (lambda: E6.encode_blocks(blocks, kind)[0])
        def make(**kw):
            return lambda n, d, signed: kernel_rdiv(n, d, top, not signed, **kw)
    want = enc()
    assert (_encode_with(module, enc, make()) == want).all()
    return ((_encode_with(module, enc, make(plus=False)) != want).any(1),
            (_encode_with(module, enc, make(minus=False)) != want).any(1))


def _lattice(x, idx, weights, alt, top, unsigned_zero, codes, keep):
    """One block's refit as a lattice.  With the indices idx [16] held, a numerator of the refit is linear in the texels:
    n_e = sum_t g_e[t] x[t], g_0 = 64 (cc v - b w), g_1 = 64 (a w - b v), and d = det depends on the indices alone.  x
    [16, C]; alt [16, C, K] holds each value's neighbours (alt[..., 0] = x).  All pairs of texels s != t of one channel
    take all of their neighbours: the variants y [16, C] are returned (at most `keep`, evenly spread) for which the
    float quotient the kernels' rdiv starts from is one off for some numerator, and the quotient and the one-off value
    quantise to different codes (codes(q) -> [..., k] for the k precisions in play).  -> (variants, +1 or -1 each)"""
    w = weights[idx]
    v = 64 - w
    a, b, cc = (v * v).sum(), (v * w).sum(), (w * w).sum()
    det = a * cc - b * b
    if det <= 0:
        return [], []
    g = np.stack([64 * (cc * v - b * w), 64 * (a * w - b * v)])             # [2, 16]
    n = (g[:, :, None] * x[None]).sum(1)                                     # [2, C]
    dn = (g[:, :, None, None] * (alt - x[..., None])[None]).transpose(0, 2, 1, 3)      # [2, C, 16, K]
    n = n[:, :, None, None, None, None] + dn[:, :, :, :, None, None] + dn[:, :, None, None, :, :]
    if unsigned_zero:
        n = np.maximum(n, 0)
    e = float_quotient_error(n, det, top)
    t = np.arange(16)
    e[:, :, t, :, t, :] = 0
    hits = np.argwhere(e != 0)
    e = e[tuple(hits.T)]
    q = np.minimum((np.abs(n[tuple(hits.T)]) + det // 2) // det, top)
    ok = (codes(q) != codes(np.minimum(q + e, top))).any(-1)
    out, kind = [], []
    for which in (1, -1):                                                    # float quotient one too high: the -1 repair
        sel = hits[ok & (e == which)]
        for _e, c, s, ks, t, kt in sel[:: max(1, len(sel) // keep)][:keep]:
            y = x.copy()
            y[s, c], y[t, c] = alt[s, c, ks], alt[t, c, kt]
            out.append(y)
            kind.append(-which)
    return out, kind


_repair_cache = {}


def repair_blocks(signed, bases=160, keep=4):
    """Blocks whose bytes the +1 and the -1 repair of rdiv decide, constructed.  The float quotient is one off only where
    the true one lies within about q 2^-23 of an integer, and an endpoint one off changes bytes only where its code
    changes with it.  So: ramps with noise, up to 1800 wide (the 12-bit mode's reach) high in the domain or (signed)
    low in it, their first-pass indices from the definition, and _lattice over the neighbouring reachable values of two
    texels at a time, for quotients that sit on a boundary of the 10-, 11- or 12-bit quantiser.  The blocks whose bytes
    change without a repair (repair_decides) come first, those of the -1 repair before those of the +1 repair."""
    if signed not in _repair_cache:
        rng = np.random.default_rng(0x4E9A + signed)
        rs = reachable(signed)
        width = rng.integers(300, 1800, (bases, 1, 1))
        start = rs[rng.integers(len(rs) * 5 // 8, len(rs) - 1, (bases, 1, 3))] - width
        x = start + (width * rng.random((bases, 16, 1)) + rng.integers(0, 1 + width // 24, (bases, 16, 3))).astype(np.int64)
        x = snap(np.minimum(x, rs[-1]), signed)
        if signed:
            x = np.where(np.arange(bases)[:, None, None] % 2 == 1, -x, x)
        ones = np.ones((bases, 16), bool)
        e0, e1, lo, hi = E6._box_endpoints(x, ones)
        idx = E6._indices(x, lo, hi, E6.quantise(e0, 10, signed)[1], E6.quantise(e1, 10, signed)[1], 4)

        def codes(q):
            return np.stack([E6.quantise(q, prec, signed)[0] for prec in (10, 11, 12)], -1)
        out = []
        for i in range(bases):
            pos = np.searchsorted(rs, x[i])
            alt = rs[np.clip(pos[..., None] + np.array([0, -2, -1, 1, 2]), 0, len(rs) - 1)]
            out += _lattice(x[i], idx[i], E6.W[4], alt, TOP[signed], not signed, codes, keep)[0]
        cand = _blocks6(np.array(out), signed, rng)
        plus, minus = repair_decides(cand, signed)
        _repair_cache[signed] = cand[np.argsort(2 * ~(plus | minus) + ~minus, kind="stable")][:256]
    return _repair_cache[signed]


def bc7_repair_blocks(bases=4096, each=160, keep=8):
    """The same for bptc_encode.hip: quotients end at 255, so the float quotient is one off only where the reduced
    determinant is above 2^15 and the true quotient one reduced step from an integer.  Ramps through all four channels
    with noise (mode 6 wins them; every second one opaque), indices of mode 6's first pass; of those the index sets at
    whose determinant 1.0f / d is rounded up the most (the float quotient too high) and down the most; _lattice over
    values up to 3 away; mode 6 keeps 8 bits with its p-bit, so every quotient is on a code boundary for one p."""
    if "bc7" not in _repair_cache:
        rng = np.random.default_rng(0x4E97)
        lo, hi = rng.integers(0, 24, (bases, 1, 4)), rng.integers(226, 256, (bases, 1, 4))
        x = np.floor(lo + (hi - lo) * rng.random((bases, 16, 1)) + rng.integers(-3, 4, (bases, 16, 4)) + 0.5).astype(np.int64)
        x = np.clip(x, 0, 255)
        x[::2, :, 3] = 255
        opaque = (x[..., 3] == 255).all(1)
        e0, e1 = E7._box_endpoints(x, np.ones((bases, 16), bool))
        r = E7.quantize_mode6(e0, e1, opaque)
        idx = E7._indices(x, r[-2], r[-1], 4)
        w = E7.W[4][idx]
        det = ((64 - w) ** 2).sum(1) * (w * w).sum(1) - ((64 - w) * w).sum(1) ** 2
        bias = (np.float32(1.0) / det.astype(np.float32)).astype(np.float64) * det - 1   # of 1.0f / d: up, the -1 repair
        out = []
        for i in np.concatenate([np.argsort(-bias, kind="stable")[:each], np.argsort(bias, kind="stable")[:each]]):
            alt = np.clip(x[i][..., None] + np.array([0, -3, -2, -1, 1, 2, 3]), 0, 255)
            if opaque[i]:
                alt[:, 3] = 255
            out += _lattice(x[i], idx[i], E7.W[4], alt, 255, True, lambda q: q[..., None], keep)[0]
        cand = np.array(out).astype(np.uint8)
        plus, minus = repair_decides(cand, "bc7")
        _repair_cache["bc7"] = cand[np.argsort(2 * ~(plus | minus) + ~minus, kind="stable")][:256]
    return _repair_cache["bc7"]


BC6H_FAMILIES = {"all_halves": all_halves, "repair_blocks": repair_blocks, "range_edges": range_edges, "delta_edges": delta_edges,
                 "refit_edges": refit_edges, "tie_blocks": tie_blocks, "partition_blocks": partition_blocks,
                 "trigger_blocks": lambda signed: trigger_blocks(signed)[0]}


def bc6h_pictures(signed):
    """name -> uint16 [h, w, 4]"""
    out = {name: picture_of_blocks(f(signed), row=ROW) for name, f in BC6H_FAMILIES.items() if name != "trigger_blocks"}
    out["trigger_waves"] = trigger_picture(signed)                          # (holds the trigger blocks)
    return out


# ---------------------------------------------------------------------------------------------------- BC7 families --
def all_bytes():
    rng = np.random.default_rng(0xB7)
    v = np.arange(256)
    solid = np.stack([v, (v + 85) & 255, (v + 170) & 255, (v + 51) & 255], -1)[:, None, :].repeat(16, 1)
    opaque = solid.copy()
    opaque[..., 3] = 255
    mixed = rng.integers(0, 256, (512, 16, 4))
    j = np.arange(512)
    for c in range(4):
        mixed[j, (j + 3 * c) % 16, c] = (j + 64 * c) & 255
    mixed[256:, :, 3] = 255
    return np.concatenate([solid, opaque, mixed]).astype(np.uint8)


def alpha_edges():
    rng = np.random.default_rng(0xA1FA)
    px = rng.integers(0, 256, (256, 16, 4))
    px[:128] = px[:128, :1]                                                 # solid colours, then noisy ones
    px[..., 3] = 255
    k = np.arange(256)
    px[k[k % 4 == 1], k[k % 4 == 1] % 16, 3] = 254                          # one texel at 254
    px[k % 4 == 2, :, 3] = 254                                              # all at 254
    px[k % 4 == 3, ::2, 3] = 254
    return px.astype(np.uint8)


def low_entropy(n=4096):
    """Two or three levels a channel near the ends and the middle of the range, short ramps, opaque and not: p-bit, index,
    score and error ties, refits that leave 0 .. 255 and refits with exact quotients."""
    rng = np.random.default_rng(0x10E)
    out = []
    for i in range(n):
        kind = i % 4
        base = rng.integers(0, 256, 4)
        if kind == 0:
            mask = rng.integers(0, 2, 16).astype(bool)
            px = np.where(mask[:, None], rng.integers(0, 256, 4), base)
        elif kind == 1:
            r = int(rng.integers(1, 24))
            px = base + rng.integers(0, r + 1, (16, 1)) * rng.integers(-1, 2, 4)
        elif kind == 2:
            end = (0, 255)[(i >> 2) & 1]
            px = end + (1 if end == 0 else -1) * rng.integers(0, int(rng.integers(2, 90)), (16, 4)) * (rng.integers(0, 3, (16, 1)) == 0)
        else:
            lv = rng.integers(0, 256, (3, 4))
            px = lv[rng.integers(0, 3, 16)]
        px = np.clip(px, 0, 255)
        if (i >> 3) & 1:
            px[:, 3] = 255
        out.append(px)
    return np.array(out).astype(np.uint8)


def bc7_partition_blocks():
    rng = np.random.default_rng(0x9A47)
    out = []
    for p in range(64):
        m = E7.P2_MASKS[p]
        order = np.where(m, np.cumsum(m) - 1, np.cumsum(~m) - 1)
        count = np.where(m, m.sum(), (~m).sum())
        for size in (40, 120, 255):
            a = 0 if size == 255 else int(rng.integers(0, 256 - size))
            b = a + size
            w = min(size // 3, 50)
            for f0 in (False, True):
                for f1 in (False, True):
                    flip = np.where(m, f1, f0)
                    g = (np.where(flip, count - 1 - order, order) * w) // np.maximum(count - 1, 1)
                    x = np.empty((16, 4), np.int64)
                    x[:, 0] = np.where(m, b - g, a)
                    x[:, 1] = np.where(m, b, a + g)
                    x[:, 2] = np.where(m, b, a)
                    x[:, 3] = 255
                    out.append(x)
    return np.array(out).astype(np.uint8)


def bc7_wave_picture():
    """opaque blocks as the quiet lanes and blocks with alpha as the loud ones, then the other way round"""
    parts = bc7_partition_blocks()[::7][:16]
    alpha = low_entropy()[:64]
    alpha = alpha[(alpha[..., 3] != 255).any(1)][:16]
    a, _ = wave_layout(parts, alpha, rows=2)
    b, _ = wave_layout(alpha, parts, rows=2)
    return picture_of_blocks(np.concatenate([a, b]), row=WAVE_ROW)


BC7_FAMILIES = {"all_bytes": all_bytes, "repair_blocks": bc7_repair_blocks, "alpha_edges": alpha_edges, "low_entropy": low_entropy,
                "partition_blocks": bc7_partition_blocks}


def bc7_pictures():
    """name -> uint8 [h, w, 4]"""
    out = {name: picture_of_blocks(f(), row=ROW) for name, f in BC7_FAMILIES.items()}
    out["mode_waves"] = bc7_wave_picture()
    return out


# ------------------------------------------------------------------------------------------------------ measuring --
def trace(module, call):
    """(call(), the records the reference module noted meanwhile)"""
    assert module.TRACE is None
    module.TRACE = records = []
    try:
        out = call()
    finally:
        module.TRACE = None
    return out, records


def records_of(records, name):
    return [r[1:] for r in records if r[0] == name]


# ------------------------------------------------------------------------------------------- decode block sets --
# Blocks are handled as bit arrays uint8 [n, 128] (bit i of the block, least significant first).


def bits_of(blocks):
    return np.unpackbits(np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16), axis=1, bitorder="little")


def blocks_of_bits(bits):
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")


def _field(bits, pos, n):
    """the n-bit field at fixed bit position pos, int64 [N]"""
    return (bits[:, pos: pos + n].astype(np.int64) << np.arange(n)).sum(1) if n else np.zeros(len(bits), np.int64)


def _fields_at(bits, pos, width, maxw):
    """fields at per-block positions pos [N, T] of per-block widths width [N, T] (<= maxw) -> int64 [N, T]"""
    out = np.zeros(pos.shape, np.int64)
    rows = np.arange(len(bits))[:, None]
    for k in range(maxw):
        out |= np.where(k < width, bits[rows, np.minimum(pos + k, 127)].astype(np.int64), 0) << k
    return out


def _put(bits, pos, n, v):
    v = np.asarray(v, np.int64)
    for k in range(n):
        bits[:, pos + k] = (v >> k) & 1


def _index_layout(start, ib, anchors):
    """positions and widths [N, 16] of an index field starting at `start`: ib bits a texel, one fewer at texel 0 and at
    the texels in anchors (list of [N])"""
    n = len(anchors[0])
    width = np.full((n, 16), ib, np.int64)
    width[:, 0] -= 1
    for a in anchors:
        width[np.arange(n), a] -= (a != 0)
    pos = start + np.cumsum(width, 1) - width
    return pos, width


def _sext(v, bits):
    return np.where(v & (1 << (bits - 1)), v - (1 << bits), v)


def _unq6(c, prec, signed):
    """_bc6h._unquantize, elementwise"""
    if not signed:
        if prec >= 15:
            return c
        return np.where(c == 0, 0, np.where(c == (1 << prec) - 1, 0xFFFF, ((c << 16) + 0x8000) >> prec))
    if prec >= 16:
        return c
    mag = np.abs(c)
    u = np.where(mag == 0, 0, np.where(mag >= (1 << (prec - 1)) - 1, 0x7FFF, ((mag << 15) + 0x4000) >> (prec - 1)))
    return np.where(c < 0, -u, u)


_ANCH2 = np.array(H7.ANCHORS_2, np.int64)
_PART2 = np.array([[(m >> t) & 1 for t in range(16)] for m in H7.PARTITIONS_2], np.int64)
_PART3 = np.array([[(m >> (2 * t)) & 3 for t in range(16)] for m in H7.PARTITIONS_3], np.int64)
_ANCH3A, _ANCH3B = np.array(H7.ANCHORS_3A, np.int64), np.array(H7.ANCHORS_3B, np.int64)
_WT = {b: np.array(H7.WEIGHTS[b], np.int64) for b in (2, 3, 4)}


def bc6h_indices(bits, regions):
    """the index fields [N, 16] of BC6H blocks of one- or two-region modes (bit arrays)"""
    anchor = _ANCH2[_field(bits, 77, 5)] if regions == 2 else np.zeros(len(bits), np.int64)
    ipos, iw = _index_layout(82 if regions == 2 else 65, 3 if regions == 2 else 4, [anchor])
    return _fields_at(bits, ipos, iw, 4)


def decode_bc6h_blocks(blocks, signed):
    """_bc6h.decode_block restated over arrays: uint8 [N, 16] -> uint16 [N, 16, 4] half patterns"""
    bits = bits_of(blocks)
    n = len(bits)
    out = np.zeros((n, 16, 4), np.int64)
    out[..., 3] = 0x3C00
    low2, low5 = _field(bits, 0, 2), _field(bits, 0, 5)
    value = np.where(low2 < 2, low2, low5)
    for mi, (mv, regions, transformed, prec, deltas, _l) in enumerate(H6.MODES):
        sel = np.flatnonzero(value == mv)
        if not len(sel):
            continue
        b = bits[sel]
        pos = H6.mode_bits(mv)
        f = {name: np.zeros(len(sel), np.int64) for name in H6.FIELDS}
        for name, fb in H6.layout(mi):
            for bit in fb:
                f[name] |= b[:, pos].astype(np.int64) << bit
                pos += 1
        part = _field(b, 77, 5) if regions == 2 else np.zeros(len(sel), np.int64)
        ends = [[f[c + k] for c in "rgb"] for k in "wxyz"[: 2 * regions]]
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
        unq = np.stack([np.stack([_unq6(e, prec, signed) for e in end], -1) for end in ends], 1)     # [n, 2 regions, 3]
        ib = 3 if regions == 2 else 4
        idx = bc6h_indices(b, regions)
        w = _WT[ib][idx][..., None]
        s = _PART2[part] if regions == 2 else np.zeros((len(sel), 16), np.int64)
        rows = np.arange(len(sel))[:, None]
        a, e = unq[rows, 2 * s], unq[rows, 2 * s + 1]
        v = ((64 - w) * a + w * e + 32) >> 6
        if signed:
            px = np.where(v < 0, 0x8000 | ((-v * 31) >> 5), (v * 31) >> 5)
        else:
            px = (v * 31) >> 6
        out[sel, :, :3] = px
    return out.astype(np.uint16)


def decode_bc7_blocks(blocks):
    """_bptc.decode_block restated over arrays: uint8 [N, 16] -> uint8 [N, 16, 4]"""
    bits = bits_of(blocks)
    n = len(bits)
    out = np.zeros((n, 16, 4), np.int64)
    first = np.where(bits[:, :8].any(1), bits[:, :8].argmax(1), 8)
    for mode in range(8):
        sel = np.flatnonzero(first == mode)
        if not len(sel):
            continue
        b = bits[sel]
        m = len(sel)
        ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = H7.MODES[mode]
        pos = mode + 1
        part = _field(b, pos, pb); pos += pb
        rot = _field(b, pos, rb); pos += rb
        isel = _field(b, pos, isb); pos += isb
        ends = np.zeros((m, 2 * ns, 4), np.int64)
        for c in range(3):
            for e in range(2 * ns):
                ends[:, e, c] = _field(b, pos, cb); pos += cb
        for e in range(2 * ns):
            ends[:, e, 3] = _field(b, pos, ab); pos += ab
        if epb:
            p = np.stack([_field(b, pos + e, 1) for e in range(2 * ns)], 1); pos += 2 * ns
        elif spb:
            sh = np.stack([_field(b, pos + e, 1) for e in range(ns)], 1); pos += ns
            p = np.repeat(sh, 2, 1)
        else:
            p = None
        for c in range(4):
            width = cb if c < 3 else ab
            if c == 3 and ab == 0:
                ends[..., 3] = 255
                continue
            v = ends[..., c]
            if p is not None:
                v, width = (v << 1) | p, width + 1
            v = v << (8 - width)
            ends[..., c] = v | (v >> width)
        if ns == 1:
            anchors, subset = [], np.zeros((m, 16), np.int64)
        elif ns == 2:
            anchors, subset = [_ANCH2[part]], _PART2[part]
        else:
            anchors, subset = [_ANCH3A[part], _ANCH3B[part]], _PART3[part]
        ipos, iw = _index_layout(pos, ib, anchors if anchors else [np.zeros(m, np.int64)])
        prim = _fields_at(b, ipos, iw, ib)
        pos += 16 * ib - ns
        if ib2:
            spos, sw = _index_layout(pos, ib2, [np.zeros(m, np.int64)])
            sec = _fields_at(b, spos, sw, ib2)
            pos += 16 * ib2 - 1
            swap = (isel == 1)[:, None]
            cw = np.where(swap, _WT[ib2][sec], _WT[ib][prim])
            aw = np.where(swap, _WT[ib][prim], _WT[ib2][sec])
        else:
            cw = aw = _WT[ib][prim]
        assert pos == 128, (mode, pos)
        rows = np.arange(m)[:, None]
        e0, e1 = ends[rows, 2 * subset], ends[rows, 2 * subset + 1]
        w = np.concatenate([np.repeat(cw[..., None], 3, -1), aw[..., None]], -1)
        px = ((64 - w) * e0 + w * e1 + 32) >> 6
        for r in (1, 2, 3):
            rr = (rot == r)[:, None]
            ch, al = px[..., r - 1].copy(), px[..., 3].copy()
            px[..., r - 1] = np.where(rr, al, ch)
            px[..., 3] = np.where(rr, ch, al)
        out[sel] = px
    return out.astype(np.uint8)


_ODD = (1, 40503, 25117, 12347, 48611, 9973, 30011, 17, 52361, 7919, 60013, 33331)


def bc6h_decode_sets():
    """name -> uint8 [n, 16] blocks, per mode (all 14): block i carries code i in the base field of R (2^prec blocks, every
    code; G and B take every code too, through odd multipliers), every other endpoint field cycles through all its values
    at its own odd stride (all deltas against all bases: the sums wrap through the mask, and in the signed format through
    the sign bit), the partition is i % 32, texel t carries index (i + 5 (t + 1)) mod 2^b (anchors lose their top bit), so that the
    lowest and the highest code meet every weight too.
    "pairs": mode 0x03 blocks of endpoints 0 <-> all ones and (10-bit two's complement) -511 <-> 511, which unquantise
    to 0 <-> 0xFFFF and -0x7FFF <-> 0x7FFF, every weight at every texel.  The sets are format-blind: each decodes under
    both formats."""
    sets = {}
    for mi, (mv, regions, _t, prec, _d, _l) in enumerate(H6.MODES):
        n = 1 << prec
        i = np.arange(n, dtype=np.int64)
        bits = np.zeros((n, 128), np.uint8)
        _put(bits, 0, H6.mode_bits(mv), np.full(n, mv))
        width = dict.fromkeys(H6.FIELDS, 0)
        for name, fb in H6.layout(mi):
            width[name] = max(width[name], max(fb) + 1)
        vals = {}
        for j, name in enumerate(H6.FIELDS):
            if width[name]:
                vals[name] = (i * _ODD[j] + (0 if j == 0 else 3 * j)) & ((1 << width[name]) - 1)
        pos = H6.mode_bits(mv)
        for name, fb in H6.layout(mi):
            for bit in fb:
                bits[:, pos] = (vals[name] >> bit) & 1
                pos += 1
        ib = 4
        if regions == 2:
            _put(bits, 77, 5, i % 32)
            pos, ib = 82, 3
        idx = (i[:, None] + 5 * np.arange(1, 17)[None, :]) & ((1 << ib) - 1)         # (from 1: texel 0 loses its top bit)
        ipos, iw = _index_layout(pos, ib, [_ANCH2[i % 32]] if regions == 2 else [np.zeros(n, np.int64)])
        for t in range(16):
            for k in range(ib):
                live = k < iw[:, t]
                bits[np.flatnonzero(live), (ipos[:, t] + k)[live]] = ((idx[:, t] >> k) & 1)[live]
        sets["mode%02x" % mv] = blocks_of_bits(bits)
    pairs = []
    for a, b in ((0, 1023), (1023, 0), (0x201, 511), (511, 0x201)):
        for rot in range(16):
            v = 0x03 | sum(a << (5 + 10 * c) for c in range(3)) | sum(b << (35 + 10 * c) for c in range(3))
            pos = 65
            for t in range(16):
                ix = (t + rot) % 16
                nb = 3 if t == 0 else 4
                v |= (ix & ((1 << nb) - 1)) << pos
                pos += nb
            pairs.append(np.frombuffer(v.to_bytes(16, "little"), np.uint8))
    sets["pairs"] = np.array(pairs)
    return sets


def bc7_decode_sets():
    """name -> uint8 [n, 16], per mode 0..7: 4 * 2^(widest endpoint field) blocks; endpoint field j of block i carries
    (i * odd_j + j) mod 2^width (every code in every field), the p-bits run through all four pairs, rotation i % 4,
    index selection (i >> 2) & 1, partition i mod 2^pb, texel t index (i + 5 t) mod 2^b."""
    sets = {}
    for mode, (ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2) in enumerate(H7.MODES):
        top = max(cb, ab)
        n = 4 << top
        i = np.arange(n, dtype=np.int64)
        bits = np.zeros((n, 128), np.uint8)
        bits[:, mode] = 1
        pos = mode + 1
        part = i & ((1 << pb) - 1)
        _put(bits, pos, pb, part); pos += pb
        _put(bits, pos, rb, i % 4); pos += rb
        _put(bits, pos, isb, (i >> 2) & 1); pos += isb
        j = 0
        for wd, count in ((cb, 6 * ns), (ab, 2 * ns if ab else 0)):
            for _ in range(count):
                _put(bits, pos, wd, (i * _ODD[j % 12] + j) & ((1 << wd) - 1)); pos += wd
                j += 1
        for e in range(2 * ns if epb else ns if spb else 0):
            bits[:, pos] = ((i >> top) >> (e % 2)) & 1
            pos += 1
        if ns == 1:
            anchors = [np.zeros(n, np.int64)]
        elif ns == 2:
            anchors = [_ANCH2[part]]
        else:
            anchors = [_ANCH3A[part], _ANCH3B[part]]
        for b, anch in ((ib, anchors), (ib2, [np.zeros(n, np.int64)])):
            if not b:
                continue
            idx = (i[:, None] + 5 * np.arange(16)[None, :] + b) & ((1 << b) - 1)
            ipos, iw = _index_layout(pos, b, anch)
            for t in range(16):
                for k in range(b):
                    live = k < iw[:, t]
                    bits[np.flatnonzero(live), (ipos[:, t] + k)[live]] = ((idx[:, t] >> k) & 1)[live]
            pos += int(iw[0].sum())
        assert pos == 128, (mode, pos)
        sets["mode%d" % mode] = blocks_of_bits(bits)
    return sets


def texture_of_sets(sets, row=ROW):
    """(blocks [n, 16] of all sets in name order, padded by repetition to whole rows of `row` blocks; w, h)"""
    blocks = np.concatenate([sets[k] for k in sorted(sets)])
    blocks = cycle_to(blocks, -(-len(blocks) // row) * row)
    return np.ascontiguousarray(blocks), 4 * row, 4 * len(blocks) // row

"""BC6H (RGB_BPTC_UNSIGNED_FLOAT / RGB_BPTC_SIGNED_FLOAT, Hap HDR) encoder: the definition the GPU kernel
hap_amd/csrc/bc6h_encode.hip reproduces bit for bit.

numpy, vectorised over blocks, integer arithmetic only.  Every rounding rule and tie-break below is part of the
definition.  A block is 16 texels in row-major order of four half-float bit patterns (uint16); alpha is ignored.
">> s" is an arithmetic shift (floor), bitlen(v) the number of bits of v >= 0 (bitlen(0) = 0).

Normalisation (per channel, before anything else), to a signed integer h:
  unsigned format: a set sign bit (-0 included) or a NaN (pattern & 0x7FFF > 0x7C00) gives 0; +Inf gives 0x7BFF.
  signed format:   a NaN gives 0; the magnitude is clamped to 0x7BFF; h = -magnitude when the sign bit is set (-0 is 0).
Error of a candidate: the exact sum over 16 texels and R, G, B of (D - h)^2, D being what _bc6h.decode_block gives
for the candidate's bytes, read as sign and magnitude like h.  Lowest error wins; on a tie the earlier candidate in
  0x03, 0x07, 0x0B, 0x0F, 0x1E, 0x01, 0x00
wins.  A candidate whose deltas do not fit is left out.

Working domain: the 16-bit values before the decoder's finish, u = ceil(64 h / 31) (unsigned), sign(h) ceil(32 |h| / 31)
(signed); top = 0xFFFF / 0x7FFF is the largest magnitude there.

Fitting a set of texels (a region, or the whole block) with b-bit indices, first precision P0, final precisions P:
  1. lo_c, hi_c: the bounding box of the set.
  2. pivot: the channel of widest range hi - lo (on a tie the lowest channel, R < G < B); cs = max(0, bitlen(its
     range) - 11).
  3. every other channel c: cov_c = sum over the set of ((2 x_c - lo_c - hi_c) >> cs) ((2 x_pivot - lo_pivot -
     hi_pivot) >> cs).  Endpoint 0 takes lo_pivot, and lo_c when cov_c >= 0, else hi_c; endpoint 1 the others.
  4. quantise both endpoints at P0 bits (below) to unquantised 16-bit endpoints D0, D1.
  5. indices: d_c = D1_c - D0_c, M = max over c of |d_c|, |lo_c - D0_c|, |hi_c - D0_c|, s = max(0, bitlen(M) - 10),
     ds_c = d_c >> s, den = ds.ds, num_t = sum_c ((x_tc - D0_c) >> s) ds_c; the index of texel t is the number of k in
     1 .. 2^b - 1 with 128 num_t > (W[k-1] + W[k]) den (W: the BPTC weight table of b bits).  (Every product of a
     texel of the set fits 32 bits.)
  6. refit: with w_t = W[index_t], A = sum (64 - w)^2, B = sum (64 - w) w, Cc = sum w^2, X_c = sum (64 - w) x_c,
     Y_c = sum w x_c and det = A Cc - B^2.  If det = 0 the endpoints of step 3 stay.  Otherwise
     E0_c = rdiv(64 (Cc X_c - B Y_c), det), E1_c = rdiv(64 (A Y_c - B X_c), det),
     rdiv(n, d) = sign(n) min(top, floor((|n| + floor(d / 2)) / d)), and 0 for n < 0 in the unsigned format.
  7. for every final precision: quantise E0, E1 at it and index again (step 5).  The first pass (steps 4-6) is done
     once and shared by the modes of a family.
  8. anchor rule: where the index of texel 0, or of region 1's anchor texel, has its top bit set, the region's two
     endpoints are swapped and its indices inverted (2^b - 1 - index).  Transformed modes then store endpoint 0 of
     region 0 as the base and every other endpoint as code - base code; the candidate is kept only if each delta lies
     in [-2^(d-1), 2^(d-1) - 1] for its channel's d bits (no reliance on the decoder's wrap-around; the swap comes first).

Quantiser at prec bits (inverse of _bc6h._unquantize; U is that function):
  unsigned: prec >= 15: the code is the value.  Else the q among (v >> (16 - prec)) - 1, + 0, + 1, clamped to
  0 .. 2^prec - 1, with the smallest |U(q) - v|, ties to the lower q.
  signed: prec >= 16: the code is the value.  Else the magnitude is quantised: the q among (|v| >> (16 - prec)) - 1, + 0,
  + 1, clamped to 0 .. 2^(prec-1) - 1, with the smallest |U(q) - |v||, ties to the lower q; code and U(q) take v's sign.

Candidates.
  One region, 4-bit indices, P0 = 10: mode 0x03 (10 bits, raw; always there), 0x07 (11 bits, deltas 9), 0x0B (12, 8),
  0x0F (16, 4).
  Two regions, 3-bit indices, P0 = 6, tried only for blocks whose best one-region error exceeds TWO_REGION_ERROR (a block
  the one-region modes already bring to the 10-bit quantiser's noise has nothing to gain from them; the kernel skips the
  family when no block of a wave asks for it, which is the same thing): mode 0x1E (6 bits, raw), 0x01 (7, deltas 6 6 6),
  0x00 (10, deltas 5 5 5).  The partition: y_c = (x_c - blo_c) >> ps with blo / bhi the block's bounding box and
  ps = max(0, bitlen(max_c (bhi_c - blo_c)) - 10); for each of the 32 partitions, with S_s the per-channel sums of y
  over region s, n_s its texel count, score = |S_0|^2 n_1 + |S_1|^2 n_0 over den = n_0 n_1; the largest score / den
  wins, compared by cross-multiplication, ties to the lower partition.  Only that partition is fitted.
"""
import numpy as np

import _bc6h as H
import _bptc as B

W = {b: np.array(B.WEIGHTS[b], dtype=np.int64) for b in (3, 4)}
P2_MASKS = np.array([[(m >> t) & 1 for t in range(16)] for m in B.PARTITIONS_2[:32]], dtype=bool)   # [32, 16]: region 1
ANCHOR2 = np.array(B.ANCHORS_2[:32], dtype=np.int64)
ONE_REGION = (0x03, 0x07, 0x0B, 0x0F)
TWO_REGION = (0x1E, 0x01, 0x00)
MODES_USED = ONE_REGION + TWO_REGION
TWO_REGION_ERROR = 48 * 16 * 16          # 16 half patterns (1/64 stop) a texel and channel
ONE = 0x3C00
_MODE = {H.MODES[i][0]: i for i in range(len(H.MODES))}

# Measurements (tests/_bptc_value_space.py): a list here receives (name, values...) of the intermediates below while an
# encode runs; None (the default) records nothing.  No result depends on it.
TRACE = None


def _note(*record):
    if TRACE is not None:
        TRACE.append(record)


def _bitlen(v):
    """bits of v >= 0, elementwise"""
    n = np.zeros(v.shape, np.int64)
    v = v.copy()
    while (v > 0).any():
        n += v > 0
        v >>= 1
    return n


def normalise(texels, signed):
    """uint16 [..., 4] -> signed integers h [..., 3]"""
    p = np.asarray(texels)[..., :3].astype(np.int64)
    mag = p & 0x7FFF
    nan = mag > 0x7C00
    mag = np.minimum(mag, 0x7BFF)
    neg = (p & 0x8000) != 0
    if signed:
        return np.where(nan, 0, np.where(neg, -mag, mag))
    return np.where(nan | neg, 0, mag)


def to_working(h, signed):
    if signed:
        return np.sign(h) * ((32 * np.abs(h) + 30) // 31)
    return (64 * h + 30) // 31


def finish(v, signed):
    """interpolated 16-bit values -> signed integers of the half pattern the decoder writes"""
    if signed:
        return np.sign(v) * ((np.abs(v) * 31) >> 5)
    return (v * 31) >> 6


def to_pattern(h):
    return np.where(h < 0, 0x8000 | -h, h)


def finish_pattern(v, signed):
    """interpolated 16-bit values -> the half patterns the decoder writes (signed: -1 finishes to -0, 0x8000)"""
    mag = np.abs(finish(v, signed))
    return np.where(v < 0, 0x8000 | mag, mag)


def _unq(q, prec, signed):
    """_bc6h._unquantize of codes q >= 0 (signed: of magnitudes)"""
    if not signed:
        if prec >= 15:
            return q
        return np.where(q == 0, 0, np.where(q == (1 << prec) - 1, 0xFFFF, ((q << 16) + 0x8000) >> prec))
    if prec >= 16:
        return q
    return np.where(q == 0, 0, np.where(q >= (1 << (prec - 1)) - 1, 0x7FFF, ((q << 15) + 0x4000) >> (prec - 1)))


def quantise(v, prec, signed):
    """v [...] -> (codes, unquantised values)"""
    if prec >= (16 if signed else 15):
        return v, v
    mag = np.abs(v)
    top = (1 << (prec - 1 if signed else prec)) - 1
    base = mag >> (16 - prec)
    best_q = best_u = best_e = None
    for dq in (-1, 0, 1):
        q = np.clip(base + dq, 0, top)
        u = _unq(q, prec, signed)
        e = np.abs(u - mag)
        if best_q is None:
            best_q, best_u, best_e = q, u, e
        else:
            _note("quant_tie", (e == best_e) & (q != best_q))
            take = (e < best_e) | ((e == best_e) & (q < best_q))
            best_q, best_u, best_e = np.where(take, q, best_q), np.where(take, u, best_u), np.where(take, e, best_e)
    sg = np.where(v < 0, -1, 1)
    return sg * best_q, sg * best_u


def _box(x, m):
    big = np.int64(1 << 40)
    mm = m[..., None]
    return np.where(mm, x, big).min(1), np.where(mm, x, -big).max(1)


def _box_endpoints(x, m):
    """steps 1-3 -> e0, e1 [N, 3], lo, hi"""
    lo, hi = _box(x, m)
    rng = hi - lo
    pivot = np.argmax(rng, axis=1)
    ar = np.arange(x.shape[0])
    cs = np.maximum(0, _bitlen(rng[ar, pivot]) - 11)
    _note("cs", rng, pivot, cs)
    px = (2 * x[ar, :, pivot] - (lo[ar, pivot] + hi[ar, pivot])[:, None]) >> cs[:, None]
    cx = (2 * x - (lo + hi)[:, None, :]) >> cs[:, None, None]
    cov = (np.where(m[..., None], cx, 0) * px[..., None]).sum(1)
    flip = cov < 0
    flip[ar, pivot] = False
    return np.where(flip, hi, lo), np.where(flip, lo, hi), lo, hi


def _indices(x, lo, hi, d0, d1, b):
    d = d1 - d0
    big = np.maximum(np.maximum(np.abs(d), np.abs(lo - d0)), np.abs(hi - d0)).max(-1)
    s = np.maximum(0, _bitlen(big) - 10)
    ds = d >> s[:, None]
    den = (ds * ds).sum(-1)
    num = (((x - d0[:, None, :]) >> s[:, None, None]) * ds[:, None, :]).sum(-1)
    _note("s", big, s, num, den, b)
    w = W[b]
    idx = np.zeros(num.shape, np.int64)
    for k in range(1, len(w)):
        idx += (128 * num > ((w[k - 1] + w[k]) * den)[:, None]).astype(np.int64)
    return idx


def _rdiv(n, d, signed):
    top = 0x7FFF if signed else 0xFFFF
    safe = np.where(d > 0, d, 1)
    q = np.minimum(top, (np.abs(n) + safe // 2) // safe)
    _note("rdiv", n, d)
    if signed:
        return np.sign(n) * q
    return np.where(n < 0, 0, q)


def _refit(x, m, idx, b, e0, e1, signed):
    w = W[b][idx] * m
    v = (64 - W[b][idx]) * m
    a = (v * v).sum(1)
    bb = (v * w).sum(1)
    c = (w * w).sum(1)
    X = (v[..., None] * x).sum(1)
    Y = (w[..., None] * x).sum(1)
    det = a * c - bb * bb
    n0 = 64 * (c[:, None] * X - bb[:, None] * Y)
    n1 = 64 * (a[:, None] * Y - bb[:, None] * X)
    dd = det[:, None]
    ok = dd > 0
    return np.where(ok, _rdiv(n0, dd, signed), e0), np.where(ok, _rdiv(n1, dd, signed), e1)


def _first_pass(x, m, b, p0, signed):
    """steps 1-6 -> refitted endpoints E0, E1 and the set's box"""
    e0, e1, lo, hi = _box_endpoints(x, m)
    _q0, d0 = quantise(e0, p0, signed)
    _q1, d1 = quantise(e1, p0, signed)
    idx = _indices(x, lo, hi, d0, d1, b)
    e0, e1 = _refit(x, m, idx, b, e0, e1, signed)
    return e0, e1, lo, hi


def _final(x, m, b, fp, prec, signed, anchor):
    """steps 7-8 for one precision -> codes q0, q1, unquantised d0, d1 (after the anchor rule), indices"""
    e0, e1, lo, hi = fp
    q0, d0 = quantise(e0, prec, signed)
    q1, d1 = quantise(e1, prec, signed)
    idx = _indices(x, lo, hi, d0, d1, b)
    ar = np.arange(idx.shape[0])
    swap = (idx[ar, anchor] >> (b - 1)) != 0
    idx = np.where(swap[:, None], (1 << b) - 1 - idx, idx)
    _note("swap", prec, anchor, swap)
    s = swap[:, None]
    return np.where(s, q1, q0), np.where(s, q0, q1), np.where(s, d1, d0), np.where(s, d0, d1), idx


def _interp(d0, d1, idx, b):
    w = W[b][idx][..., None]
    return ((64 - w) * d0[:, None, :] + w * d1[:, None, :] + 32) >> 6


def _pack(mode, ends, part, idx, anchors, b):
    """mode value, ends: the endpoint codes [N, 3] of w, x(, y, z) as stored (deltas already taken), indices -> [N, 4]
    uint32 words"""
    n = idx.shape[0]
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)

    def put(v, pos):
        nonlocal lo, hi
        v = np.asarray(v, np.int64).astype(np.uint64) & np.uint64(1)
        if pos < 64:
            lo |= v << np.uint64(pos)
        else:
            hi |= v << np.uint64(pos - 64)

    mi = _MODE[mode]
    nb = H.mode_bits(mode)
    for i in range(nb):
        put(np.full(n, (mode >> i) & 1), i)
    pos = nb
    field = {c + k: ends[ki][:, ci] for ki, k in enumerate("wxyz"[: len(ends)]) for ci, c in enumerate("rgb")}
    for name, bits in H.layout(mi):
        for bit in bits:
            put(field[name] >> bit, pos)
            pos += 1
    if len(ends) == 4:
        for i in range(5):
            put(part >> i, pos)
            pos += 1
    is_anchor = np.zeros((n, 16), bool)
    ar = np.arange(n)
    for a in anchors:
        is_anchor[ar, a] = True
    # the index field: b bits a texel, one fewer at the anchors (their top bit is 0 after the anchor rule)
    acc = np.zeros(n, np.uint64)
    width = np.zeros(n, np.uint64)
    for t in range(16):
        acc |= idx[:, t].astype(np.uint64) << width
        width += np.where(is_anchor[:, t], b - 1, b).astype(np.uint64)
    assert pos >= 64 and (width + np.uint64(pos) == 128).all()
    hi |= acc << np.uint64(pos - 64)
    m32 = np.uint64(0xFFFFFFFF)
    return np.stack([lo & m32, lo >> np.uint64(32), hi & m32, hi >> np.uint64(32)], -1)


def _deltas_fit(base, q, dbits):
    ok = np.ones(base.shape[0], bool)
    for c in range(3):
        d = q[:, c] - base[:, c]
        _note("delta", c, dbits[c], d)
        ok &= (d >= -(1 << (dbits[c] - 1))) & (d <= (1 << (dbits[c] - 1)) - 1)
    return ok


def _sse(dec, h):
    return ((dec - h) ** 2).sum((1, 2))


def _one_region(x, h, signed):
    """-> list of (mode, words, interpolated 16-bit texels, error, valid) in candidate order"""
    n = x.shape[0]
    m = np.ones((n, 16), bool)
    zero = np.zeros(n, np.int64)
    fp = _first_pass(x, m, 4, 10, signed)
    out = []
    for mode in ONE_REGION:
        _v, _r, transformed, prec, dbits, _l = H.MODES[_MODE[mode]]
        q0, q1, d0, d1, idx = _final(x, m, 4, fp, prec, signed, zero)
        raw = _interp(d0, d1, idx, 4)
        valid = _deltas_fit(q0, q1, dbits) if transformed else np.ones(n, bool)
        words = _pack(mode, [q0, q1 - q0 if transformed else q1], zero, idx, [zero], 4)
        out.append((mode, words, raw, _sse(finish(raw, signed), h), valid))
    return out


def best_partition(x):
    lo, hi = x.min(1), x.max(1)
    ps = np.maximum(0, _bitlen((hi - lo).max(-1)) - 10)
    _note("ps", (hi - lo).max(-1), ps)
    y = (x - lo[:, None, :]) >> ps[:, None, None]
    tot = y.sum(1)
    s1 = np.einsum("pt,ntc->npc", P2_MASKS.astype(np.int64), y)
    s0 = tot[:, None, :] - s1
    n1 = P2_MASKS.sum(1).astype(np.int64)
    n0 = 16 - n1
    score = (s0 * s0).sum(-1) * n1 + (s1 * s1).sum(-1) * n0
    den = n0 * n1
    best = np.zeros(x.shape[0], np.int64)
    bs, bd = score[:, 0], np.full(x.shape[0], den[0], np.int64)
    for p in range(1, 32):
        _note("score_tie", (score[:, p] * bd == bs * den[p]) & (score[:, p] > 0))
        better = score[:, p] * bd > bs * den[p]
        best = np.where(better, p, best)
        bs = np.where(better, score[:, p], bs)
        bd = np.where(better, den[p], bd)
    return best


def _two_regions(x, h, signed, modes=TWO_REGION):
    n = x.shape[0]
    part = best_partition(x)
    sub1 = P2_MASKS[part]
    anchor1 = ANCHOR2[part]
    zero = np.zeros(n, np.int64)
    sets = ((~sub1, zero), (sub1, anchor1))
    fps = [_first_pass(x, m, 3, 6, signed) for m, _a in sets]
    out = []
    for mode in modes:
        _v, _r, transformed, prec, dbits, _l = H.MODES[_MODE[mode]]
        idx = np.zeros((n, 16), np.int64)
        raw = np.zeros((n, 16, 3), np.int64)
        ends = []
        for (m, anchor), fp in zip(sets, fps):
            q0, q1, d0, d1, ix = _final(x, m, 3, fp, prec, signed, anchor)
            idx = np.where(m, ix, idx)
            raw = np.where(m[..., None], _interp(d0, d1, ix, 3), raw)
            ends += [q0, q1]
        valid = np.ones(n, bool)
        if transformed:
            for k in (1, 2, 3):
                valid &= _deltas_fit(ends[0], ends[k], dbits)
            ends = [ends[0]] + [e - ends[0] for e in ends[1:]]
        words = _pack(mode, ends, part, idx, [zero, anchor1], 3)
        out.append((mode, words, raw, _sse(finish(raw, signed), h), valid))
    return out


def encode_blocks(texels, signed, two_regions=True, two_region_modes=TWO_REGION, threshold=TWO_REGION_ERROR):
    """texels: uint16 [N, 16, 4] -> (blocks uint8 [N, 16], predicted decoded texels uint16 [N, 16, 4], mode values [N]).
    (two_regions False: the one-region modes alone; the other keywords are for measurements.)"""
    h = normalise(texels, signed)
    x = to_working(h, signed)
    n = x.shape[0]
    cands = _one_region(x, h, signed)
    _note("candidates", [(c[0], c[3], c[4]) for c in cands])
    mode0, words, dec, err, _valid = cands[0]
    modes = np.full(n, mode0, np.int64)
    for mode, w, d, e, valid in cands[1:]:
        take = valid & (e < err)
        words, dec, err, modes = np.where(take[:, None], w, words), np.where(take[:, None, None], d, dec), np.where(take, e, err), np.where(take, mode, modes)
    if two_regions:
        asked = err > threshold
        _note("asked", err, asked)
        for mode, w, d, e, valid in _two_regions(x, h, signed, two_region_modes):
            _note("candidates", [(mode, e, valid)])
            take = asked & valid & (e < err)
            words, dec, err, modes = np.where(take[:, None], w, words), np.where(take[:, None, None], d, dec), np.where(take, e, err), np.where(take, mode, modes)
    blocks = np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(n, 16)
    pred = np.concatenate([finish_pattern(dec, signed), np.full((n, 16, 1), ONE, np.int64)], -1).astype(np.uint16)
    return blocks, pred, modes


def wave_tries_two_regions(texels, signed):
    """The kernel's ballot: the two-region family runs for a wave (64 consecutive blocks of a block row) when any of its
    blocks asks for it.  It changes no byte: a block that does not ask ignores the family's result."""
    h = normalise(texels, signed)
    x = to_working(h, signed)
    err = None
    for _mode, _w, _d, e, valid in _one_region(x, h, signed):
        err = e if err is None else np.where(valid & (e < err), e, err)
    return bool((err > TWO_REGION_ERROR).any())


def to_blocks(pic):
    """uint16 [h, w, 4] -> texels [N, 16, 4] of its 4x4 blocks, row-major"""
    h, w = pic.shape[:2]
    return np.ascontiguousarray(pic.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4))


def from_blocks(texels, h, w):
    return np.ascontiguousarray(np.asarray(texels, np.uint16).reshape(h // 4, w // 4, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(h, w, 4))


def encode(pic, signed, chunk=1 << 14, **kw):
    """uint16 (or float16) [h, w, 4] (h, w multiples of 4) -> BC6H texture bytes, blocks row-major"""
    t = to_blocks(np.ascontiguousarray(pic).view(np.uint16))
    out = [encode_blocks(t[i:i + chunk], signed, **kw)[0] for i in range(0, t.shape[0], chunk)]
    return np.concatenate(out).tobytes()


def psnr_half(dec, pic, signed):
    """10 log10(0x7BFF^2 / mse) over the integer half patterns (normalised input against decoded), R, G, B"""
    a = normalise(dec, True).astype(np.float64)            # decoded patterns are never special
    b = normalise(pic, signed).astype(np.float64)
    mse = float(np.mean((a - b) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(float(0x7BFF) ** 2 / mse)

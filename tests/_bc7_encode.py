"""BC7 (RGBA_BPTC_UNORM, Hap R) encoder: the definition the GPU kernel hap_amd/csrc/bptc_encode.hip reproduces bit for bit.

numpy, vectorised over blocks, integer arithmetic only.  Every rounding rule and tie-break below is part of the
definition.  A block is 16 RGBA8 texels in row-major order.

Candidates.  A block is *opaque* when all 16 alpha values are 255.
  opaque:     mode 6 with both p-bits forced to 1 (alpha decodes to exactly 255), and mode 1 on one partition.
  with alpha: mode 6 with p-bits chosen per endpoint, and mode 5 (rotation 0).
The candidate with the lowest error wins; on a tie the lower mode number wins.  The error is the exact sum over the
16 texels and the four channels of (decoded - input)^2, the decoded texel being what _bptc.decode_block gives.

Mode 1's partition: for each of the 64 two-subset partitions, with S_s the per-channel RGB sums of subset s, n_s its
texel count and |S_s|^2 the sum of their squares, score = |S_0|^2 n_1 + |S_1|^2 n_0 over den = n_0 n_1.  The
subsets' squared error about their means is sum(x^2) - score / den, so the partition of the largest score / den wins,
compared exactly by cross-multiplication; on a tie the lower partition number wins.  Only that partition is fitted.

Fitting a set of texels (one subset, or the whole block) on channels C with b-bit indices:
  1. lo_c, hi_c: the bounding box of the set.
  2. pivot: the channel of widest range hi - lo (on a tie the lowest channel, R < G < B < A).
  3. every other channel c: cov_c = sum (2 x_c - lo_c - hi_c)(2 x_pivot - lo_pivot - hi_pivot) over the set (the rule
     of oracle/bc_oracle.c).  Endpoint 0 takes lo_pivot, and lo_c when cov_c >= 0, else hi_c; endpoint 1 the others.
  4. quantise both endpoints (below) to decoded 8-bit endpoints D0, D1.
  5. indices: d = D1 - D0, den = d.d, num_t = (x_t - D0).d; the index of texel t is the number of k in 1..2^b - 1
     with 128 num_t > (W[k-1] + W[k]) den (W: the BPTC weight table of b bits): the nearest weight to 64 num_t / den,
     ties to the lower index.
  6. refit: with w_t = W[index_t], A = sum (64 - w)^2, B = sum (64 - w) w, Cc = sum w^2, X_c = sum (64 - w) x_c,
     Y_c = sum w x_c and det = A Cc - B^2.  If det = 0 the endpoints of step 3 stay.  Otherwise
     E0_c = rdiv(64 (Cc X_c - B Y_c), det), E1_c = rdiv(64 (A Y_c - B X_c), det),
     rdiv(n, d) = 0 for n <= 0, else min(255, floor((n + floor(d / 2)) / d)).
  7. quantise E0, E1 again and index again (step 5): these are the candidate's endpoints and indices.
  8. anchor rule: where the index of texel 0, or of the subset's anchor texel, has its top bit set, the subset's two
     endpoints (with their p-bits) are swapped and its indices inverted (2^b - 1 - index); the texels decode the same.

Quantisers (a code q of cb bits, p-bit p when the mode has one; U(q) = _bptc's unquantize of (q << 1 | p) or q):
  each channel takes the q among floor(v / 2^(8 - cb)) - 1, + 0, + 1 (clamped to 0 .. 2^cb - 1) with the smallest
  |U(q) - v|, ties to the lower q.
  mode 6 (RGBA 7 + p): with alpha, each endpoint tries p = 0 and p = 1 and keeps the one of smaller sum over RGBA of
  (U - v)^2, ties to p = 0; opaque, p = 1.
  mode 1 (RGB 6 + one p per subset): p = 0 and p = 1 for both endpoints of the subset together, smaller summed error
  over both, ties to p = 0.
  mode 5: RGB 7 bits, alpha 8 bits (exact), no p-bits; colour (RGB, 2-bit indices) and alpha (A, 2-bit indices) are
  fitted separately, each by the steps above.
"""
import numpy as np

import _bptc as B

W = {b: np.array(B.WEIGHTS[b], dtype=np.int64) for b in (2, 3, 4)}
P2_MASKS = np.array([[(m >> t) & 1 for t in range(16)] for m in B.PARTITIONS_2], dtype=bool)   # [64, 16]: subset 1
ANCHOR2 = np.array(B.ANCHORS_2, dtype=np.int64)
MODES_USED = (1, 5, 6)

# Measurements (tests/_bptc_value_space.py): a list here receives (name, values...) of the intermediates below while an
# encode runs; None (the default) records nothing.  No result depends on it.
TRACE = None


def _note(*record):
    if TRACE is not None:
        TRACE.append(record)


def _unq(code, bits):
    v = code << (8 - bits)
    return v | (v >> bits)


def _quant_channel(v, cb, p, has_p):
    """v [...] int64 -> (q, U(q)) nearest, ties to the lower q."""
    top = (1 << cb) - 1
    base = v >> (8 - cb)
    best_q = best_u = best_e = None
    for dq in (-1, 0, 1):
        q = np.clip(base + dq, 0, top)
        u = _unq((q << 1) | p, cb + 1) if has_p else _unq(q, cb)
        e = np.abs(u - v)
        if best_q is None:
            best_q, best_u, best_e = q, u, e
        else:
            _note("quant_tie", (e == best_e) & (q != best_q))
            take = (e < best_e) | ((e == best_e) & (q < best_q))
            best_q, best_u, best_e = np.where(take, q, best_q), np.where(take, u, best_u), np.where(take, e, best_e)
    return best_q, best_u


def _quant_p(v, cb, p):
    """v [N, C] with p [N] -> codes, decoded, summed squared error [N]"""
    q, u = _quant_channel(v, cb, p[:, None], True)
    return q, u, ((u - v) ** 2).sum(-1)


def quantize_mode6(e0, e1, opaque):
    """e0, e1 [N, 4] -> (q0, q1, p0, p1, D0, D1)"""
    n = e0.shape[0]
    out = []
    for e in (e0, e1):
        zero, one = np.zeros(n, np.int64), np.ones(n, np.int64)
        qa, ua, ea = _quant_p(e, 7, zero)
        qb, ub, eb = _quant_p(e, 7, one)
        _note("p_tie", 6, (eb == ea) & ~opaque)
        use1 = opaque | (eb < ea)
        out.append((np.where(use1[:, None], qb, qa), np.where(use1, 1, 0), np.where(use1[:, None], ub, ua)))
    (q0, p0, d0), (q1, p1, d1) = out
    return q0, q1, p0, p1, d0, d1


def quantize_mode1(e0, e1):
    """e0, e1 [N, 3] -> (q0, q1, p, D0, D1), one p-bit for both endpoints"""
    n = e0.shape[0]
    zero, one = np.zeros(n, np.int64), np.ones(n, np.int64)
    q0a, u0a, r0a = _quant_p(e0, 6, zero)
    q1a, u1a, r1a = _quant_p(e1, 6, zero)
    q0b, u0b, r0b = _quant_p(e0, 6, one)
    q1b, u1b, r1b = _quant_p(e1, 6, one)
    _note("p_tie", 1, (r0b + r1b) == (r0a + r1a))
    use1 = (r0b + r1b) < (r0a + r1a)
    s = use1[:, None]
    return np.where(s, q0b, q0a), np.where(s, q1b, q1a), use1.astype(np.int64), np.where(s, u0b, u0a), np.where(s, u1b, u1a)


def quantize_plain(e0, e1, cb):
    q0, u0 = _quant_channel(e0, cb, 0, False)
    q1, u1 = _quant_channel(e1, cb, 0, False)
    return q0, q1, u0, u1


def _box_endpoints(x, m):
    """x [N, 16, C], m [N, 16] bool -> the bounding-box diagonal endpoints e0, e1 [N, C] (steps 1-3)"""
    big = np.int64(1 << 20)
    mm = m[..., None]
    lo = np.where(mm, x, big).min(1)
    hi = np.where(mm, x, -big).max(1)
    rng = hi - lo
    pivot = np.argmax(rng, axis=1)                       # first maximum: the lowest channel on a tie
    ar = np.arange(x.shape[0])
    px = 2 * x[ar, :, pivot] - (lo[ar, pivot] + hi[ar, pivot])[:, None]          # [N, 16]
    cov = (np.where(mm, (2 * x - (lo + hi)[:, None, :]), 0) * px[..., None]).sum(1)   # [N, C]
    flip = cov < 0
    flip[ar, pivot] = False
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def _indices(x, d0, d1, b):
    """nearest-weight indices [N, 16] of x [N, 16, C] on the segment D0 -> D1 (step 5)"""
    d = d1 - d0
    den = (d * d).sum(-1)                                 # [N]
    num = ((x - d0[:, None, :]) * d[:, None, :]).sum(-1)  # [N, 16]
    _note("index", num, den, b)
    w = W[b]
    idx = np.zeros(num.shape, np.int64)
    for k in range(1, len(w)):
        idx += (128 * num > ((w[k - 1] + w[k]) * den)[:, None]).astype(np.int64)
    return idx


def _rdiv(n, d):
    safe = np.where(d > 0, d, 1)
    _note("rdiv", n, d)
    return np.where(n <= 0, 0, np.minimum(255, (n + safe // 2) // safe))


def _refit(x, m, idx, b, e0, e1):
    """least-squares endpoints from the indices (step 6); e0 / e1 stay where det = 0"""
    w = W[b][idx] * m                                     # texels outside the set weigh nothing...
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
    return np.where(ok, _rdiv(n0, dd), e0), np.where(ok, _rdiv(n1, dd), e1)


def _interp(d0, d1, idx, b):
    """decoded texels [N, 16, C]"""
    w = W[b][idx][..., None]
    return ((64 - w) * d0[:, None, :] + w * d1[:, None, :] + 32) >> 6


def _fit(x, m, b, quant):
    """steps 1-7 -> (quantiser result of the final endpoints, indices [N, 16])"""
    e0, e1 = _box_endpoints(x, m)
    r = quant(e0, e1)
    idx = _indices(x, r[-2], r[-1], b)
    e0, e1 = _refit(x, m, idx, b, e0, e1)
    r = quant(e0, e1)
    return r, _indices(x, r[-2], r[-1], b)


class _Bits:
    """128-bit blocks [N] built as 4 uint32 words, fields appended least significant bit first"""

    def __init__(self, n):
        self.words = np.zeros((n, 4), np.uint64)
        self.pos = 0

    def put(self, v, nbits):
        v = np.asarray(v, np.int64).astype(np.uint64) & np.uint64((1 << nbits) - 1)
        if np.ndim(v) == 0:
            v = np.full(self.words.shape[0], v, np.uint64)
        pos = self.pos
        while nbits:
            wd, off = divmod(pos, 32)
            take = min(nbits, 32 - off)
            self.words[:, wd] |= (v & np.uint64((1 << take) - 1)) << np.uint64(off)
            v = v >> np.uint64(take)
            pos += take
            nbits -= take
        self.pos = pos

    def bytes(self):
        assert self.pos == 128
        return self.words.astype("<u4")


def _sse(dec, x):
    return ((dec - x) ** 2).sum((1, 2))


def _swap_for_anchor(idx, b, anchor_t, subset_m, pairs):
    """anchor rule for one subset: returns (idx, swapped[N]); pairs: list of (a, b) arrays to exchange where swapped"""
    ar = np.arange(idx.shape[0])
    top = 1 << (b - 1)
    swapped = (idx[ar, anchor_t] & top) != 0
    _note("swap", b, anchor_t, swapped)
    inv = (1 << b) - 1 - idx
    idx = np.where(swapped[:, None] & subset_m, inv, idx)
    out = []
    for a0, a1 in pairs:
        s = swapped.reshape((-1,) + (1,) * (a0.ndim - 1))
        out.append((np.where(s, a1, a0), np.where(s, a0, a1)))
    return idx, swapped, out


def _put_indices(bits, idx, b, anchors):
    """indices of 16 texels, b bits each, one bit less at the anchor texels (anchors: list of [N] texel numbers)"""
    n = idx.shape[0]
    ar = np.arange(n)
    is_anchor = np.zeros((n, 16), bool)
    for a in anchors:
        is_anchor[ar, a] = True
    # build the index field as a python-int-free 64-bit accumulator: at most 63 bits
    acc = np.zeros(n, np.uint64)
    width = np.zeros(n, np.uint64)
    for t in range(16):
        nb = np.where(is_anchor[:, t], b - 1, b).astype(np.uint64)
        acc |= idx[:, t].astype(np.uint64) << width
        width += nb
    total = 16 * b - len(anchors)
    assert (width == total).all()
    bits.put(acc & np.uint64(0xFFFFFFFF), min(32, total))
    if total > 32:
        bits.put(acc >> np.uint64(32), total - 32)


def _mode6(x, opaque):
    n = x.shape[0]
    m = np.ones((n, 16), bool)
    (q0, q1, p0, p1, d0, d1), idx = _fit(x, m, 4, lambda a, c: quantize_mode6(a, c, opaque))
    idx, _, ((q0, q1), (p0, p1), (d0, d1)) = _swap_for_anchor(idx, 4, np.zeros(n, np.int64), m, [(q0, q1), (p0, p1), (d0, d1)])
    dec = _interp(d0, d1, idx, 4)
    bits = _Bits(n)
    bits.put(1 << 6, 7)
    for c in range(4):
        bits.put(q0[:, c], 7)
        bits.put(q1[:, c], 7)
    bits.put(p0, 1)
    bits.put(p1, 1)
    _put_indices(bits, idx, 4, [np.zeros(n, np.int64)])
    return bits.bytes(), dec, _sse(dec, x)


def best_partition(x):
    """mode 1's partition [N] (RGB of x [N, 16, 4])"""
    rgb = x[..., :3]
    tot = rgb.sum(1)                                              # [N, 3]
    s1 = np.einsum("pt,ntc->npc", P2_MASKS.astype(np.int64), rgb)  # [N, 64, 3]
    s0 = tot[:, None, :] - s1
    n1 = P2_MASKS.sum(1).astype(np.int64)                           # [64]
    n0 = 16 - n1
    score = (s0 * s0).sum(-1) * n1 + (s1 * s1).sum(-1) * n0          # [N, 64]
    den = n0 * n1
    best = np.zeros(x.shape[0], np.int64)
    bs, bd = score[:, 0], np.full(x.shape[0], den[0], np.int64)
    for p in range(1, 64):
        _note("score_tie", (score[:, p] * bd == bs * den[p]) & (score[:, p] > 0))
        better = score[:, p] * bd > bs * den[p]
        best = np.where(better, p, best)
        bs = np.where(better, score[:, p], bs)
        bd = np.where(better, den[p], bd)
    return best


def _mode1(x):
    n = x.shape[0]
    rgb = x[..., :3]
    part = best_partition(x)
    sub1 = P2_MASKS[part]                                           # [N, 16] bool
    anchor1 = ANCHOR2[part]
    idx = np.zeros((n, 16), np.int64)
    ends = []
    dec = np.zeros((n, 16, 3), np.int64)
    for s, m in ((0, ~sub1), (1, sub1)):
        (q0, q1, p, d0, d1), ix = _fit(rgb, m, 3, quantize_mode1)
        anchor = np.zeros(n, np.int64) if s == 0 else anchor1
        ix, _, ((q0, q1), (d0, d1)) = _swap_for_anchor(ix, 3, anchor, m, [(q0, q1), (d0, d1)])
        idx = np.where(m, ix, idx)
        dec = np.where(m[..., None], _interp(d0, d1, ix, 3), dec)
        ends.append((q0, q1, p))
    bits = _Bits(n)
    bits.put(1 << 1, 2)
    bits.put(part, 6)
    for c in range(3):
        for q0, q1, _ in ends:
            bits.put(q0[:, c], 6)
            bits.put(q1[:, c], 6)
    bits.put(ends[0][2], 1)
    bits.put(ends[1][2], 1)
    _put_indices(bits, idx, 3, [np.zeros(n, np.int64), anchor1])
    dec = np.concatenate([dec, np.full((n, 16, 1), 255, np.int64)], -1)
    return bits.bytes(), dec, _sse(dec, x)


def _mode5(x):
    n = x.shape[0]
    m = np.ones((n, 16), bool)
    zero = np.zeros(n, np.int64)
    (cq0, cq1, cd0, cd1), ci = _fit(x[..., :3], m, 2, lambda a, c: quantize_plain(a, c, 7))
    ci, _, ((cq0, cq1), (cd0, cd1)) = _swap_for_anchor(ci, 2, zero, m, [(cq0, cq1), (cd0, cd1)])
    (aq0, aq1, ad0, ad1), ai = _fit(x[..., 3:], m, 2, lambda a, c: quantize_plain(a, c, 8))
    ai, _, ((aq0, aq1), (ad0, ad1)) = _swap_for_anchor(ai, 2, zero, m, [(aq0, aq1), (ad0, ad1)])
    dec = np.concatenate([_interp(cd0, cd1, ci, 2), _interp(ad0, ad1, ai, 2)], -1)
    bits = _Bits(n)
    bits.put(1 << 5, 6)
    bits.put(0, 2)                                                   # rotation 0
    for c in range(3):
        bits.put(cq0[:, c], 7)
        bits.put(cq1[:, c], 7)
    bits.put(aq0[:, 0], 8)
    bits.put(aq1[:, 0], 8)
    _put_indices(bits, ci, 2, [zero])
    _put_indices(bits, ai, 2, [zero])
    return bits.bytes(), dec, _sse(dec, x)


def encode_blocks(texels):
    """texels: uint8 [N, 16, 4] -> (blocks uint8 [N, 16], predicted decoded texels uint8 [N, 16, 4], modes [N])"""
    x = np.asarray(texels, np.int64)
    n = x.shape[0]
    opaque = (x[..., 3] == 255).all(1)
    b6, d6, e6 = _mode6(x, opaque)
    b1, d1, e1 = _mode1(x)
    b5, d5, e5 = _mode5(x)
    # opaque: mode 1 against mode 6 (mode 1 wins a tie); with alpha: mode 5 against mode 6 (mode 5 wins a tie)
    e_other = np.where(opaque, e1, e5)
    _note("errors", opaque, e6, e1, e5)
    take6 = e6 < e_other
    words = np.where(take6[:, None], b6, np.where(opaque[:, None], b1, b5))
    dec = np.where(take6[:, None, None], d6, np.where(opaque[:, None, None], d1, d5))
    modes = np.where(take6, 6, np.where(opaque, 1, 5))
    blocks = np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(n, 16)
    return blocks, dec.astype(np.uint8), modes


def to_blocks(img):
    """uint8 [h, w, 4] -> texels [N, 16, 4] of its 4x4 blocks, row-major"""
    h, w = img.shape[:2]
    return np.ascontiguousarray(img.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4))


def encode(img, chunk=1 << 15):
    """uint8 [h, w, 4] (h, w multiples of 4) -> BC7 texture bytes, blocks row-major"""
    t = to_blocks(np.asarray(img, np.uint8))
    out = [encode_blocks(t[i:i + chunk])[0] for i in range(0, t.shape[0], chunk)]
    return np.concatenate(out).tobytes()


def from_blocks(texels, h, w):
    """texels [N, 16, 4] -> uint8 [h, w, 4]"""
    return np.ascontiguousarray(np.asarray(texels, np.uint8).reshape(h // 4, w // 4, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(h, w, 4))

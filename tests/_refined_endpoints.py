"""The definition of HAPGPU_ENCODE_REFINE_ENDPOINTS (include/hap_gpu.h) in numpy, vectorised over blocks.

A colour block of RGB_DXT1, and of the colour half of RGBA_DXT5, starts as the default encoder's (oracle/bc_oracle.c,
colour_block, restated here as `default_block`) and goes through two rounds of least-squares refinement of its two
end points for the indices it has; a round's candidate replaces the block only where its squared error is strictly
smaller.  Everything is integer.  px: int64 [n, 16, 3] (pixel i = 4 * row + column of the block, channels R, G, B).
"""
import functools

import numpy as np

ROUNDS = 2
WEIGHT = np.array([3, 0, 2, 1])           # thirds of pal[0] in palette entry k


def blocks_of(img):
    """uint8 [h, w, >= 3] -> int64 [h/4 * w/4, 16, 3], blocks in texture order"""
    h, w = img.shape[:2]
    p = img[..., :3].astype(np.int64).reshape(h // 4, 4, w // 4, 4, 3).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(p.reshape(-1, 16, 3))


def quant5(v):
    t = v * 31 + 128
    return (t + (t >> 8)) >> 8


def quant6(v):
    t = v * 63 + 128
    return (t + (t >> 8)) >> 8


def pack565(rgb):
    """[n, 3] bytes -> the 5:6:5 word"""
    return quant5(rgb[:, 0]) << 11 | quant6(rgb[:, 1]) << 5 | quant5(rgb[:, 2])


def palette(c0, c1):
    """bc_oracle.c:decode_colour with c0 > c1 -> [n, 4, 3]"""
    def expand(c):
        r, g, b = c >> 11, (c >> 5) & 63, c & 31
        return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], -1)
    p0, p1 = expand(c0), expand(c1)
    return np.stack([p0, p1, (2 * p0 + p1) // 3, (p0 + 2 * p1) // 3], 1)


def pick_indices(px, c0, c1):
    """bc_oracle.c:pick_indices on the palette of c0, c1 -> [n, 16] indices; 0 where c0 == c1"""
    pal = palette(c0, c1)
    d = pal[:, 0] - pal[:, 1]
    len2 = (d * d).sum(1)
    base = (pal[:, 1] * d).sum(1)
    safe = np.maximum(len2, 1)
    m24 = 50331648 // safe
    top = len2 + len2 // 6
    t = (px * d[:, None, :]).sum(2) + (len2 // 6 - base)[:, None]
    t = np.clip(t, 0, top[:, None])
    pos = np.minimum(((t * m24[:, None]) & 0xFFFFFFFF) >> 24, 3)
    return np.where((c0 != c1)[:, None], np.array([1, 3, 2, 0])[pos], 0)


def default_block(px):
    """bc_oracle.c:colour_block -> c0, c1 [n], idx [n, 16]"""
    lo, hi = px.min(1), px.max(1)
    dev = 2 * px - (lo + hi)[:, None, :]
    cov_rg = (dev[..., 0] * dev[..., 1]).sum(1)
    cov_bg = (dev[..., 2] * dev[..., 1]).sum(1)
    inset = (hi - lo) >> 4
    lo, hi = lo + inset, hi - inset
    ea, eb = hi.copy(), lo.copy()
    for c, cov in ((0, cov_rg), (2, cov_bg)):
        ea[:, c] = np.where(cov < 0, lo[:, c], hi[:, c])
        eb[:, c] = np.where(cov < 0, hi[:, c], lo[:, c])
    qa, qb = pack565(ea), pack565(eb)
    c0, c1 = np.maximum(qa, qb), np.minimum(qa, qb)
    return c0, c1, pick_indices(px, c0, c1)


def err(px, c0, c1, idx):
    """sum over pixels and channels of (px - pal[idx])^2 -> [n]"""
    chosen = np.take_along_axis(palette(c0, c1), idx[:, :, None], 1)
    return ((px - chosen) ** 2).sum((1, 2))


def moments(idx):
    """A, B, C, det of a block's indices -> four [n]"""
    w = WEIGHT[idx]
    v = 3 - w
    A, B, C = (w * w).sum(1), (w * v).sum(1), (v * v).sum(1)
    return A, B, C, A * C - B * B


def numerators(px, idx):
    """C P - B Q and A Q - B P per channel -> two [n, 3], and det [n]"""
    w = WEIGHT[idx]
    v = 3 - w
    A, B, C, det = moments(idx)
    P, Q = (w[:, :, None] * px).sum(1), (v[:, :, None] * px).sum(1)
    return C[:, None] * P - B[:, None] * Q, A[:, None] * Q - B[:, None] * P, det


def rounded_quotient(num, det):
    """clamp((2 * 3 * num + det) div (2 det), 0, 255), det > 0"""
    return np.clip((6 * num + det) // (2 * det), 0, 255)


def candidate(px, idx):
    """a round's candidate for blocks with indices idx -> valid [n], c0', c1' [n] (0 where not valid)"""
    na, nb, det = numerators(px, idx)
    valid = det != 0
    safe = np.where(valid, det, 1)[:, None]
    qa = pack565(rounded_quotient(na, safe))
    qb = pack565(rounded_quotient(nb, safe))
    return valid, np.where(valid, np.maximum(qa, qb), 0), np.where(valid, np.minimum(qa, qb), 0)


def one_round(px, c0, c1, idx):
    valid, n0, n1 = candidate(px, idx)
    nidx = pick_indices(px, n0, n1)
    win = valid & (err(px, n0, n1, nidx) < err(px, c0, c1, idx))
    return np.where(win, n0, c0), np.where(win, n1, c1), np.where(win[:, None], nidx, idx)


def refined_block(px, rounds=ROUNDS):
    c0, c1, idx = default_block(px)
    for _ in range(rounds):
        c0, c1, idx = one_round(px, c0, c1, idx)
    return c0, c1, idx


def pack(c0, c1, idx):
    """-> uint8 [n, 8], the DXT1 block bytes"""
    word = (idx << (2 * np.arange(16))[None, :]).sum(1)
    out = np.empty((len(c0), 8), np.uint8)
    for k, v in enumerate((c0, c0 >> 8, c1, c1 >> 8, word, word >> 8, word >> 16, word >> 24)):
        out[:, k] = v & 255
    return out


def unpack(blocks):
    """uint8 [n, 8] -> c0, c1, idx"""
    b = blocks.astype(np.int64)
    word = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    return b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8, (word[:, None] >> (2 * np.arange(16))[None, :]) & 3


def encode_dxt1(img, refine=True):
    """uint8 [h, w, >= 3] -> uint8 [blocks, 8]"""
    px = blocks_of(img)
    return pack(*(refined_block(px) if refine else default_block(px)))


def encode_dxt5(img, default_dxt5):
    """the refined DXT5 texture: the default's alpha halves (bytes: the default DXT5 texture of img) with refined colour
    halves -> uint8 [blocks, 16]"""
    out = np.frombuffer(default_dxt5, np.uint8).reshape(-1, 16).copy()
    out[:, 8:] = encode_dxt1(img)
    return out


def changed(blocks, img):
    """which blocks (uint8 [n, 8] colour blocks of img) differ from the default's -> bool [n]"""
    return (np.asarray(blocks).reshape(-1, 8) != encode_dxt1(img, refine=False)).any(1)


# ------------------------------------------------------------------------------ the edges of the definition --
def first_round(px):
    """what the first round meets, per block: det, the unclamped rounded quotients a, b [n, 3], qa, qb"""
    c0, c1, idx = default_block(px)
    na, nb, det = numerators(px, idx)
    safe = np.where(det != 0, det, 1)[:, None]
    a, b = (6 * na + safe) // (2 * safe), (6 * nb + safe) // (2 * safe)
    return c0, c1, det, a, b, pack565(np.clip(a, 0, 255)), pack565(np.clip(b, 0, 255))


def classes(px):
    """the block classes the tests name -> bool [n] each"""
    c0, c1, det, a, b, qa, qb = first_round(px)
    packed = np.sort(px[..., 0] << 16 | px[..., 1] << 8 | px[..., 2], 1)
    colours = 1 + (packed[:, 1:] != packed[:, :-1]).sum(1)
    ok = det != 0
    return {"solid": colours == 1, "two_colour": colours == 2, "default_c0_equals_c1": c0 == c1,
            "clamped_at_0": ok & ((a < 0) | (b < 0)).any(1), "clamped_at_255": ok & ((a > 255) | (b > 255)).any(1),
            "qa_below_qb": ok & (qa < qb), "candidate_c0_equals_c1": ok & (qa == qb) & (c0 != c1)}


@functools.lru_cache(maxsize=None)
def edge_blocks(per_class=34):
    """272 blocks with up to `per_class` of every class of classes() (every class is there; solid: eight, they are all
    alike): solid and two-colour blocks, near-solid ones (whose default end points fall together), blocks of one outlier
    pixel beside fifteen near 0 or near 255 (whose least-squares end points leave 0..255), and blocks just below white
    (where both clamped end points can quantise to one word) -> int64 [272, 16, 3], read-only"""
    rng = np.random.default_rng(20250601)
    pool = []
    solid = rng.integers(0, 256, (40, 1, 3))
    solid[:3, 0] = ((0, 0, 0), (255, 255, 255), (255, 0, 128))
    pool.append(np.repeat(solid, 16, 1))
    two = rng.integers(0, 256, (400, 2, 3))
    pool.append(two[np.arange(400)[:, None], rng.integers(0, 2, (400, 16))])
    near = rng.integers(0, 256, (1500, 1, 3)) + rng.integers(-3, 4, (1500, 16, 3))
    pool.append(np.clip(near, 0, 255))
    for base in (0, 255):
        out = np.clip(base + rng.integers(-40, 41, (1500, 16, 3)), 0, 255)
        out[np.arange(1500), rng.integers(0, 16, 1500)] = rng.integers(0, 256, (1500, 3))
        pool.append(out)
    ramp = rng.integers(0, 256, (600, 1, 3)) + (rng.integers(-12, 13, (600, 1, 3)) * np.arange(16)[None, :, None]) // 2
    pool.append(np.clip(ramp + rng.integers(-6, 7, (600, 16, 3)), 0, 255))
    pool.append(np.clip(255 + rng.integers(-6, 7, (60000, 16, 3)), 0, 255))
    pool = np.concatenate(pool).astype(np.int64)
    cls = classes(pool)
    chosen = []
    for name, mask in cls.items():
        chosen.extend(np.flatnonzero(mask)[:8 if name == "solid" else per_class].tolist())
    chosen = list(dict.fromkeys(chosen))
    rest = [i for i in range(len(pool)) if i not in set(chosen)]
    chosen.extend(rest[:272 - len(chosen)])
    assert len(chosen) == 272
    out = pool[chosen]
    out.setflags(write=False)
    return out


def picture_of(px, blocks_x):
    """int64 [n, 16, 3] -> the uint8 RGBA picture [4 n / blocks_x, 4 blocks_x, 4] of those blocks, alpha a ramp"""
    n = len(px)
    rows = n // blocks_x
    img = np.zeros((rows * 4, blocks_x * 4, 4), np.uint8)
    img[..., :3] = px.reshape(rows, blocks_x, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(rows * 4, blocks_x * 4, 3)
    y, x = np.mgrid[0:rows * 4, 0:blocks_x * 4]
    img[..., 3] = (x * 7 + y * 13) & 255
    return img

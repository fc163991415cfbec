"""The block encoders' index selection (clamp t, one multiply, positions gathered from the top) and the centred Y / Co /
Cg of the Hap Q encoder on the GPU, against oracle/bc_oracle.c byte for byte, on two small pictures whose blocks are
chosen for what can go wrong there:

  * pixels that project below 0 and above top = len2 + len2 / 6 (end points inset by the box rule and moved by their
    5:6:5 rounding, two outlier pixels beyond them) -- the clamp now works on t, not on the position;
  * blocks whose sixteen positions use all four values and read differently backwards -- a gather that runs from the
    wrong end shows; the same for the eight ramp codes of each half of the alpha-style blocks;
  * chroma ranges that select the scales 1, 2 and 4; channel values 0, 127, 128, 255 in every channel; alpha 0, 0x7F,
    0x80, 0xFF; flat blocks (c0 == c1).

The blocks are picked from a seeded pool with the numpy restatement of tests/test_index_selection_identity.py, and the
pictures are asserted to hold every case before anything runs.  256 x 8 is two rows of 64 blocks (one full wavefront
step each way), 260 x 12 three rows of 65 (a block row longer than a wavefront, a last step that is partly empty).

Roads: Hap Q and DXT5 through encode_frames_rgba in batches of 8 (fragments placed) and 7 (slots and a gather pass) --
the fused kernels --, the same and Hap Q Alpha through a context made under HAP_AMD_NO_FUSION -- the batch kernels --,
DXT1 and RGTC1 (and the other two) through compress_rgba.  The kernel class that ran is asserted from the context's
profile, as in tests/test_fused_encode_shapes_gpu.py."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V
import test_fused_encode_shapes_gpu as F
import test_gpu_parity as P
import test_index_selection_identity as I

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
SIZES = [(256, 8), (260, 12)]
SPECIAL = np.array([0, 127, 128, 255])


def _pool(seed=0x1D5E1):
    """Seeded candidate blocks, uint8 [n, 16, 4]."""
    rng = np.random.default_rng(seed)
    n = 4096
    # a segment between two colours, the pixels at sixteen different places along it in a shuffled order, the first two
    # moved beyond the ends; spans from a few units (where the 5:6:5 rounding moves an end point by a good part of the
    # segment) to the whole range, little noise across
    a = rng.integers(0, 256, (n, 1, 4))
    span = rng.choice([6, 10, 16, 24, 40, 90, 255], (n, 1, 1))
    b = np.clip(a + rng.integers(-1, 2, (n, 1, 4)) * span, 0, 255)
    w = np.stack([rng.permutation(16) for _ in range(n)])[..., None] / 15.0 * 0.7 + 0.15
    w[:, 0], w[:, 1] = -0.1, 1.1
    seg = a + (b - a) * w + rng.integers(-2, 3, (n, 16, 4))
    # near grey with a small chroma: the scales 4 and 2
    grey = rng.integers(16, 240, (n // 2, 1, 1)) + rng.integers(-1, 2, (n // 2, 1, 4)) * rng.choice([3, 12, 40], (n // 2, 1, 1)) \
        + rng.integers(-6, 7, (n // 2, 16, 4))
    special = SPECIAL[rng.integers(0, 4, (256, 16, 4))]
    flat = np.repeat(rng.integers(0, 256, (64, 1, 4)), 16, axis=1)
    flat[:4] = SPECIAL[:, None, None]
    return np.concatenate([seg.round(), grey, special, flat]).clip(0, 255).astype(np.uint8)


def _not_a_palindrome(codes):
    return (codes != codes[:, ::-1]).any(axis=1)


def _cases(px):
    """{case name: bool [n]} of blocks uint8 [n, 16, 4]."""
    p = px.astype(np.int64)
    rgb = I.colour_block_new(p[..., :3], raw=True)
    y, co, cg = I.centred_transform(p[..., 0], p[..., 1], p[..., 2])
    hq = I.ycocg_colour_block_new(co, cg, raw=True)
    out = {}
    for name, m in (("rgb", rgb), ("hapq", hq)):
        live = ~m["flat"]
        pos = I.new_position(m["t"], m["m24"][:, None], m["top"][:, None])
        out[name + " below 0"] = live & (m["t"] < 0).any(axis=1)
        out[name + " above top"] = live & (m["t"] > m["top"][:, None]).any(axis=1)
        out[name + " both ends beyond"] = out[name + " below 0"] & out[name + " above top"]
        out[name + " four positions, no palindrome"] = live & _not_a_palindrome(pos) & \
            np.all([(pos == k).any(axis=1) for k in range(4)], axis=0)
        out[name + " flat"] = m["flat"]
    for s in (1, 2, 4):
        out["hapq scale %d" % s] = ~hq["flat"] & (hq["scale"] == s)
    for ch, vals in ((3, p[..., 3]), (4, y + 128)):                       # the two alpha-style blocks: A and luma
        d = vals.max(axis=1) - vals.min(axis=1)
        what = "alpha" if ch == 3 else "luma"
        out[what + " ramp, no palindrome"] = (d >= 7) & _not_a_palindrome(vals[:, :8]) & _not_a_palindrome(vals[:, 8:])
        out[what + " flat"] = d == 0
    for c, cname in enumerate("RGBA"):
        for v in (SPECIAL if c < 3 else (0, 0x7F, 0x80, 0xFF)):
            out["%s %d" % (cname, v)] = (p[..., c] == v).any(axis=1)
    return out


_made = {}


def picture(w, h):
    """The picture of this size: for every case the first two blocks of the pool that show it, then the pool in order."""
    if (w, h) not in _made:
        pool = _pool()
        cases = _cases(pool)
        n = (w // 4) * (h // 4)
        # `distinct` different blocks, repeated: the frames are to take the field-stream road, which a picture of
        # unrelated blocks -- stored raw -- would not
        distinct = 32 if w == 256 else w // 4
        assert n % distinct == 0
        chosen = []
        for name, m in cases.items():
            hits = np.flatnonzero(m)
            assert len(hits) >= 1, "the pool has no block for: " + name
            if not any(m[i] for i in chosen):
                chosen.append(int(hits[0]))
        assert len(chosen) <= distinct, (len(chosen), distinct)
        rest = [i for i in range(0, len(pool), len(pool) // distinct) if i not in chosen]
        blocks = pool[(chosen + rest)[:distinct]]
        # dealt out so that the cases do not all sit in the first lanes
        # (each block n / distinct times in a row: the field matcher looks a few blocks back)
        blocks = np.repeat(blocks[np.random.default_rng(w * h).permutation(distinct)], n // distinct, axis=0)
        for name, m in _cases(blocks).items():
            assert m.any(), "picture %dx%d lost the case: %s" % (w, h, name)
        img = V.picture_of_blocks(blocks, row=w // 4)
        assert img.shape == (h, w, 4)
        _made[(w, h)] = (img, {f: D.oracle_bc_encode(img, f) for f in (L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1)})
    return _made[(w, h)]


@pytest.fixture(scope="module")
def hap():
    import hap_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hap_amd


@pytest.fixture(scope="module")
def ctx(hap):
    c = hap.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def unfused_ctx(hap):
    c = P._context_with(hap, HAP_AMD_NO_FUSION="1")
    yield c
    c.close()


def same_blocks(got, want, img, fmt, what):
    bb = D.BLOCK_BYTES[fmt]
    got = np.frombuffer(bytes(got), dtype=np.uint8).reshape(-1, bb)
    want = np.frombuffer(want, dtype=np.uint8).reshape(-1, bb)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d blocks differ; first: block %d\n  input  %s\n  kernel %s\n  oracle %s" % (
            what, len(bad), len(got), i, V.blocks_of_picture(img)[i].tolist(), got[i].tolist(), want[i].tolist()))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1], ids=["dxt1", "dxt5", "hapq", "rgtc1"])
def test_compress_rgba_writes_the_oracles_blocks(ctx, w, h, fmt):
    img, tex = picture(w, h)
    src = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    (r, got), launches = F.profiled(ctx, lambda: ctx.compress_rgba(src, w, h, w * 4, fmt))
    assert r == 0 and launches["block_encode"] >= 1 and launches["encode_fused"] == 0, (r, launches)
    same_blocks(got, tex[fmt], img, fmt, "compress_rgba %dx%d %#x" % (w, h, fmt))


def _frames(c, hap, img, w, h, fmts, batch):
    sizes = [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]
    T = len(fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [1] * T)
    src = torch.from_numpy(img).cuda()
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    (r, used, res), launches = F.profiled(c, lambda: c.encode_frames_rgba(
        [src] * batch, w, h, w * 4, fmts, [1] * T, [1] * T, outs, flags=hap.ENCODE_FRAGMENT_INDEX))
    assert r == 0 and res == [0] * batch, (w, h, fmts, batch)
    return [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)], launches, sizes


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", [L.FMT_YCOCG, L.FMT_DXT5], ids=["hapq", "dxt5"])
def test_fused_kernel_writes_the_oracles_frames(ctx, hap, w, h, fmt, batch):
    img, tex = picture(w, h)
    frames, launches, sizes = _frames(ctx, hap, img, w, h, [fmt], batch)
    assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    code, got, got_fmt = ORA.decode(frames[0], 0, sizes[0])
    assert code == 0 and got_fmt == fmt
    same_blocks(got, tex[fmt], img, fmt, "fused %dx%d %#x batch %d" % (w, h, fmt, batch))
    F.frame_against_oracle(frames[0], tex[fmt], fmt, 1, (w, h, fmt, batch))
    assert all(f == frames[0] for f in frames[1:]), (w, h, fmt, batch)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmts", [[L.FMT_YCOCG], [L.FMT_DXT5], [L.FMT_YCOCG, L.FMT_RGTC1]], ids=["hapq", "dxt5", "hapq_alpha"])
def test_batch_kernels_write_the_oracles_frames(unfused_ctx, hap, w, h, fmts):
    img, tex = picture(w, h)
    frames, launches, sizes = _frames(unfused_ctx, hap, img, w, h, fmts, 8)
    assert launches["block_encode"] >= 1 and launches["encode_fused"] == 0, launches
    for t, f in enumerate(fmts):
        code, got, got_fmt = ORA.decode(frames[0], t, sizes[t])
        assert code == 0 and got_fmt == f
        same_blocks(got, tex[f], img, f, "unfused %dx%d texture %d of %s" % (w, h, t, fmts))
    if len(fmts) == 1:
        F.frame_against_oracle(frames[0], tex[fmts[0]], fmts[0], 1, (w, h, fmts, "unfused"))
    assert all(f == frames[0] for f in frames[1:]), (w, h, fmts)


def test_the_pictures_hold_every_case():
    """(Runs with the GPU tests because they are what it guards; needs none itself.)"""
    for w, h in SIZES:
        picture(w, h)

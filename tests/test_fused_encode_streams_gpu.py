"""The fused RGBA -> blocks -> field stream kernel against the oracle, byte for byte, on pictures built so that the
element mixes of their streams reach the corners of the kernel's match, choose and emit stages -- the geometry tests
(tests/test_fused_encode_shapes_gpu.py) use natural pictures, whose streams are ordinary.  The comparison is theirs
(frame_against_oracle: every fragment's bytes, size and group table against oracle/field_stream_oracle.c, the blocks
against oracle/bc_oracle.c through the oracle's decoder).

Pictures are made of 4 x 4 tiles whose blocks are steered field by field: a tile has an alpha-role pattern (the luma
of Hap Q, the alpha channel of DXT5: fields 0 and 1, end points and indices) and a colour-role pattern (fields 2 and
3).  Two tiles with the same end points but another arrangement of the same values agree in the end-point field alone.

  flat      one colour: one chain of run copies, the fewest elements
  noise     per-pixel noise over six block rows (all literals, runs of more than 60 bytes with their length byte, no
            copy: a 2-byte field that happens to match stays a literal), two flat block rows below:
            frame_against_oracle asks for chunks that Snappy shrinks
  table     every block unlike its four predecessors in every field of more than two bytes but equal to a block
            5..400 back: candidates from the table only, copy-2 distances of 2048 bytes and more among them
  lone      tiles drawn from a small alphabet of end points and arrangements: single 4-byte fields that match between
            literal fields (`lone4`), 2-byte fields that match alone (`lone`), more than a thousand elements in the
            full fragment (seventeen passes of the tag walk and more)
  cut       runs of 2..8 equal blocks at every offset of a half-tile: copies that run across field 16 and are cut at
            64 bytes, and ones that just fit

Shapes: 260 x 32 (a full fragment and 8 blocks) and 264 x 32 (a full fragment and 16 blocks), one chunk, as batches of
8 (placed) and 7 (slots), both fused formats.  A picture of noise alone does not shrink and is stored, not Snappy; it
runs through the kernel all the same and is checked through the oracle's decoder
(test_noise_alone_is_stored_and_decodes)."""
import numpy as np
import pytest

import _data as D
import _libs as L
import test_gpu_parity as P
from test_fused_encode_shapes_gpu import ORA, frame_against_oracle, profiled

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20260817
SHAPES = [pytest.param(260, 32, id="w260-tail8"), pytest.param(264, 32, id="w264-tail16")]
FORMATS = [pytest.param(L.FMT_YCOCG, id="ycocg"), pytest.param(L.FMT_DXT5, id="dxt5")]
W_BASE = np.array([0, 7, 1, 6, 2, 5, 3, 4, 0, 7, 2, 5, 1, 6, 3, 4])        # alpha-role steps of a tile (both ends present)
U_BASE = np.array([0, 3, 1, 2, 0, 3, 1, 2, 3, 0, 2, 1, 0, 3, 1, 2])        # colour-role steps


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


def tile(fmt, le, lp, ce, cp):
    """A 4 x 4 RGBA tile: alpha-role end points `le` (lo, hi) in arrangement `lp`, colour-role end points `ce` in
    arrangement `cp` (arrangements: permutations of the sixteen positions)."""
    w = le[0] + (le[1] - le[0]) * W_BASE[lp] // 7
    u = U_BASE[cp]
    if fmt == L.FMT_YCOCG:
        (co0, cg0), (co1, cg1) = ce
        co, cg = co0 + (co1 - co0) * u // 3, cg0 + (cg1 - cg0) * u // 3
        px = np.stack([w + co - cg, w + cg, w - co - cg, np.full(16, 255)], axis=1)
    else:
        c0, c1 = np.array(ce[0]), np.array(ce[1])
        rgb = c0[None, :] + (c1 - c0)[None, :] * u[:, None] // 3
        px = np.concatenate([rgb, w[:, None]], axis=1)
    assert px.min() >= 0 and px.max() <= 255
    return px.astype(np.uint8).reshape(4, 4, 4)


def picture(tiles, w, h):
    """[h, w, 4] from (w / 4) (h / 4) tiles in block order."""
    bx, by = w // 4, h // 4
    t = np.asarray(tiles, dtype=np.uint8).reshape(by, bx, 4, 4, 4)
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3, 4).reshape(h, w, 4))


def noise_tiles(rng, n):
    t = rng.integers(0, 256, size=(n, 4, 4, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(0, 256, size=(n, 4, 4), dtype=np.uint8)
    return t


def alphabet(rng, fmt):
    """End points and arrangements to draw tiles from."""
    les = [(70, 200), (80, 180), (96, 150)]
    if fmt == L.FMT_YCOCG:
        ces = [((-30, -20), (30, 20)), ((-10, 25), (20, -25)), ((5, -30), (-25, 10))]
    else:
        ces = [((20, 40, 200), (220, 180, 30)), ((200, 10, 60), (40, 240, 90)), ((128, 128, 0), (100, 10, 250))]
    perms = [rng.permutation(16) for _ in range(4)]
    return les, ces, perms


def pic_flat(fmt, w, h, rng):
    return picture(np.tile(np.array([90, 140, 60, 200], dtype=np.uint8), (w * h // 16, 4, 4, 1)), w, h)


def pic_noise(fmt, w, h, rng):
    n, row = w * h // 16, w // 4
    t = noise_tiles(rng, n)
    t[6 * row:] = np.array([10, 20, 30, 40], dtype=np.uint8)
    return picture(t, w, h)


def pic_table(fmt, w, h, rng):
    n, fresh = w * h // 16, 200
    pool = noise_tiles(rng, fresh)
    ids = list(range(fresh))
    for i in range(fresh, n):
        while True:
            d = int(rng.integers(5, 41)) if rng.integers(0, 2) else int(rng.integers(128, min(i, 400) + 1))
            if ids[i - d] not in ids[i - 4: i]:
                break
        ids.append(ids[i - d])
    return picture(pool[ids], w, h)


def pic_lone(fmt, w, h, rng):
    les, ces, perms = alphabet(rng, fmt)
    n = w * h // 16
    pick = rng.integers(0, [len(les), len(perms), len(ces), len(perms)], size=(n, 4))
    return picture([tile(fmt, les[a], perms[b], ces[c], perms[d]) for a, b, c, d in pick], w, h)


def pic_cut(fmt, w, h, rng):
    les, ces, perms = alphabet(rng, fmt)
    n = w * h // 16
    t = noise_tiles(rng, n)
    for ht in range(0, n, 8):                 # a run per half-tile: blocks first .. first + length - 1 are equal
        first = (ht // 8) % 4
        length = 2 + (ht // 32) % 7
        run = tile(fmt, les[ht % 3], perms[ht % 4], ces[(ht // 8) % 3], perms[(ht // 16) % 4])
        t[ht + first: min(n, ht + first + length)] = run
    return picture(t, w, h)


PICTURES = {"flat": pic_flat, "noise": pic_noise, "table": pic_table, "lone": pic_lone, "cut": pic_cut}
_made = {}


def made(kind, fmt, w, h):
    """(picture, the oracle's texture), made once per case and shared by the batches."""
    key = (kind, fmt, w, h)
    if key not in _made:
        pic = PICTURES[kind](fmt, w, h, np.random.default_rng([SEED, sorted(PICTURES).index(kind), fmt & 0xFF, w]))
        _made[key] = (pic, D.oracle_bc_encode(pic, fmt))
    return _made[key]


def fields(tex):
    """The blocks' four fields as integers: [blocks, 4]."""
    b = np.frombuffer(tex, dtype=np.uint8).reshape(-1, 16).astype(np.uint64)
    le = lambda cols: sum(b[:, c] << np.uint64(8 * i) for i, c in enumerate(cols))
    return np.stack([le(range(0, 2)), le(range(2, 8)), le(range(8, 12)), le(range(12, 16))], axis=1)


def elements(tex, fragment=0):
    return P._unpack_groups(P._ofs_fragment(tex[8192 * fragment: 8192 * (fragment + 1)], 4, 0)[1])[2]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_pictures_are_what_their_names_say(fmt, w, h):
    """The oracle's textures and streams of the pictures have the properties the cases are there for (no GPU work:
    what is asserted comes from the oracle alone)."""
    f = {k: fields(made(k, fmt, w, h)[1]) for k in PICTURES}
    n = len(f["flat"])
    # flat: one block value; two elements per half-tile (the first block's literals aside)
    assert len(set(map(tuple, f["flat"]))) == 1 and elements(made("flat", fmt, w, h)[1]) <= 2 * 64 + 4
    # noise: in the noise rows no field of more than two bytes equals the same field 1..4 blocks back (a 2-byte field
    # that matches alone stays a literal)
    rows = 6 * (w // 4)
    for d in range(1, 5):
        assert not (f["noise"][d:rows, 1:] == f["noise"][:rows - d, 1:]).any()
    # table: no field of more than two bytes matches at the four fixed distances, every block from 200 on has occurred 5..400 blocks
    # before, at 128 blocks (2048 bytes) and more for some
    t = f["table"]
    for d in range(1, 5):
        assert not (t[d:, 1:] == t[:-d, 1:]).any()
    back = [min(d for d in range(5, min(i, 400) + 1) if (t[i] == t[i - d]).all()) for i in range(200, n)]
    assert min(back) >= 5 and sum(d >= 128 for d in back) >= 20
    # lone: blocks whose colour end points alone match the block before, blocks whose 2-byte field alone does;
    # more than a thousand elements in the full fragment (the natural 8K stream has 470)
    a = f["lone"]
    same = a[1:] == a[:-1]
    assert (same[:, 2] & ~same[:, 0] & ~same[:, 1] & ~same[:, 3]).sum() >= 10
    assert (same[:, 0] & ~same[:, 1] & ~same[:, 2] & ~same[:, 3]).sum() >= 10
    assert elements(made("lone", fmt, w, h)[1]) > 1000
    # cut: runs of equal blocks across the middle of a half-tile, longer than 64 bytes and not
    c = f["cut"]
    eq = (c[1:] == c[:-1]).all(axis=1)
    across = [sum(eq[ht + k] for k in range(7)) for ht in range(0, 512, 8) if eq[ht + 3]]
    assert any(r >= 5 for r in across) and any(r <= 4 for r in across)


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
@pytest.mark.parametrize("kind", sorted(PICTURES))
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_kernel_writes_the_oracles_streams(ctx, hap, fmt, w, h, kind, batch):
    pic, tex = made(kind, fmt, w, h)
    size = len(tex)
    cap = hap.HapMaxEncodedLength([size], [fmt], [1])
    dev = torch.from_numpy(pic).cuda()
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    t0, r0 = ctx.placement_timeouts(), ctx.placement_retries()
    (r, used, res), launches = profiled(ctx, lambda: ctx.encode_frames_rgba(
        [dev] * batch, w, h, w * 4, [fmt], [1], [1], outs, flags=hap.ENCODE_FRAGMENT_INDEX))
    assert r == 0 and res == [0] * batch, (kind, fmt, batch)
    assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    assert (ctx.placement_timeouts(), ctx.placement_retries()) == (t0, r0)
    frames = [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]
    frame_against_oracle(frames[0], tex, fmt, 1, (kind, w, h, fmt, batch))
    assert ORA.decode(frames[0], 0, size) == (0, tex, fmt)
    for i in range(1, batch):
        assert frames[i] == frames[0], (kind, fmt, batch, i)


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_noise_alone_is_stored_and_decodes(ctx, hap, fmt, batch):
    """All literals in every half-tile of both fragments: the stream is longer than the texture, so the chunk is
    stored; the frame still decodes to the oracle's blocks."""
    w, h = 260, 32
    pic = picture(noise_tiles(np.random.default_rng([SEED, 99, fmt & 0xFF]), w * h // 16), w, h)
    tex = D.oracle_bc_encode(pic, fmt)
    assert len(P._ofs_fragment(tex[:8192], 4, 0)[0]) > 8192
    cap = hap.HapMaxEncodedLength([len(tex)], [fmt], [1])
    dev = torch.from_numpy(pic).cuda()
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    r, used, res = ctx.encode_frames_rgba([dev] * batch, w, h, w * 4, [fmt], [1], [1], outs,
                                          flags=hap.ENCODE_FRAGMENT_INDEX)
    assert r == 0 and res == [0] * batch
    for i in range(batch):
        assert ORA.decode(outs[i][: used[i]].cpu().numpy().tobytes(), 0, len(tex)) == (0, tex, fmt)

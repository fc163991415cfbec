"""The matrix-pipe YCoCg transform (hap_amd/csrc/bc_encode_core.hpp) on the GPU, byte for byte against oracle/bc_oracle.c,
on the smallest pictures where a group of four lanes is partly inactive or a wave is nearly empty: the matrix
instruction reads the weight rows from lanes 0..2 of every group of four whether or not those lanes run, so a lane
whose group-mates have left the kernel is the case that can go wrong.

  widths 4, 8, 12, 20 (1, 2, 3, 5 blocks a row: groups of four with 1, 2, 3 and 4 + 1 lanes alive) by heights 4 and 8,
  and 260 x 4: 65 blocks, a second wave with one live lane.

Every road that runs the transform: compress_rgba (Hap Q), the two-texture frame call (Hap Q Alpha's block kernel: the
road by which that kernel is reached; it keeps the dot-product form and must write the same bytes), the fused kernel
through encode_frames_rgba in a batch of 8 (placed) and of 7 (slots), the planes encoder, one transcode to Hap Q.  The
pictures hold the eight corner colours (the saturated primaries among them: Co - 128 = +128 occurs only there) and
seeded noise; the CPU side of the same arithmetic is tests/test_ycocg_matrix_transform.py."""
import functools

import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as V
import test_fused_encode_shapes_gpu as F
import test_ycocg_matrix_transform as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
SIZES = [(4, 4), (8, 4), (12, 4), (20, 4), (4, 8), (8, 8), (12, 8), (20, 8), (260, 4)]


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


@functools.lru_cache(maxsize=None)
def picture(w, h):
    """(picture [h, w, 4], its Hap Q texture, its RGTC1 alpha plane): corner-colour blocks and noise blocks in turn"""
    pool = M.pinned_blocks(noise=256)
    n = (w // 4) * (h // 4)
    corner = (320 + np.arange(n) * 67) % (64 * 16)                           # from red / blue on, spread over pairs and positions
    noise = 64 * 16 + np.arange(n) * 5 % 512
    px = pool[np.where(np.arange(n) % 2 == 0, corner, noise)]
    img = np.ascontiguousarray(V.picture_of_blocks(px, row=w // 4))
    assert img.shape == (h, w, 4)
    img.setflags(write=False)
    return img, D.oracle_bc_encode(img, L.FMT_YCOCG), D.oracle_bc_encode(img, L.FMT_RGTC1)


def differing(got, want, bb=16):
    got, want = np.frombuffer(bytes(got), np.uint8), np.frombuffer(want, np.uint8)
    if got.shape != want.shape:
        return "lengths %d / %d" % (got.size, want.size)
    bad = np.flatnonzero((got.reshape(-1, bb) != want.reshape(-1, bb)).any(axis=1))
    return None if not len(bad) else "%d of %d blocks differ, first %d" % (len(bad), got.size // bb, int(bad[0]))


def test_the_pictures_hold_the_cases():
    for w, h in SIZES:
        y, co, cg = M.matrix_form(V.blocks_of_picture(picture(w, h)[0]))
        assert (co == 128).any() or (co == -127).any() or (cg == 128).any() or (cg == -127).any(), (w, h)
    y, co, cg = M.matrix_form(V.blocks_of_picture(picture(260, 4)[0]))
    assert (co == 128).any() and (co == -127).any() and (cg == 128).any() and (cg == -127).any()


def test_compress_rgba_hap_q(ctx):
    for w, h in SIZES:
        img, tex, _plane = picture(w, h)
        src = torch.from_numpy(img.copy()).cuda()
        torch.cuda.synchronize()
        (r, got), launches = F.profiled(ctx, lambda: ctx.compress_rgba(src, w, h, w * 4, L.FMT_YCOCG))
        assert r == 0 and launches["block_encode"] >= 1 and launches["encode_fused"] == 0, (w, h, r, launches)
        assert differing(got, tex) is None, (w, h, differing(got, tex))


def encoded(ctx, hap, img, w, h, fmts, batch):
    sizes = [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]
    T = len(fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [1] * T)
    src = torch.from_numpy(img.copy()).cuda()
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    (r, used, res), launches = F.profiled(ctx, lambda: ctx.encode_frames_rgba(
        [src] * batch, w, h, w * 4, fmts, [1] * T, [1] * T, outs, flags=hap.ENCODE_FRAGMENT_INDEX))
    assert r == 0 and res == [0] * batch, (w, h, fmts, batch, r, res)
    return [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)], launches, sizes


def test_hap_q_alpha_block_kernel(ctx, hap):
    for w, h in SIZES:
        img, tex, plane = picture(w, h)
        frames, launches, sizes = encoded(ctx, hap, img, w, h, [L.FMT_YCOCG, L.FMT_RGTC1], 8)
        assert launches["block_encode"] >= 1 and launches["encode_fused"] == 0, (w, h, launches)
        for t, (want, fmt) in enumerate(((tex, L.FMT_YCOCG), (plane, L.FMT_RGTC1))):
            code, got, got_fmt = ORA.decode(frames[0], t, sizes[t])
            assert code == 0 and got_fmt == fmt, (w, h, t)
            assert differing(got, want, D.BLOCK_BYTES[fmt]) is None, (w, h, t, differing(got, want, D.BLOCK_BYTES[fmt]))
        assert all(f == frames[0] for f in frames[1:]), (w, h)


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
def test_fused_kernel(ctx, hap, batch):
    for w, h in SIZES:
        img, tex, _plane = picture(w, h)
        frames, launches, sizes = encoded(ctx, hap, img, w, h, [L.FMT_YCOCG], batch)
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, (w, h, batch, launches)
        code, got, got_fmt = ORA.decode(frames[0], 0, sizes[0])
        assert code == 0 and got_fmt == L.FMT_YCOCG, (w, h, batch)
        assert differing(got, tex) is None, (w, h, batch, differing(got, tex))
        assert all(f == frames[0] for f in frames[1:]), (w, h, batch)


def test_planes_encoder(ctx):
    for w, h in SIZES:
        img, tex, _plane = picture(w, h)
        planes = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32)).cuda()   # element = byte
        torch.cuda.synchronize()
        r, got = ctx.compress_planes(planes, w, h, L.FMT_YCOCG, scale=(1.0,) * 4, bias=(0.0,) * 4)
        assert r == 0, (w, h, r)
        assert differing(got, tex) is None, (w, h, differing(got, tex))


def test_transcode_to_hap_q(ctx):
    for w, h in SIZES:
        img = picture(w, h)[0]
        src = D.oracle_bc_encode(img, L.FMT_DXT5)
        pic = np.ascontiguousarray(D.oracle_bc_decode(src, L.FMT_DXT5, w, h))
        want = D.oracle_bc_encode(pic, L.FMT_YCOCG)
        r, got = ctx.transcode_texture(src, L.FMT_DXT5, w, h, 0, [L.FMT_YCOCG])
        assert r == 0, (w, h, r)
        assert differing(got[0], want) is None, (w, h, differing(got[0], want))

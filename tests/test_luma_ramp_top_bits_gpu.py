"""The fused Hap Q kernel's luma half on the GPU, byte for byte against the scalar definition.  The kernel takes luma
from row 0 of the matrix product as 256 (255 - Y) + junk and makes the ramp field in the top bits of one unsigned
24-bit multiply-add (hap_amd/csrc/bc_encode_core.hpp, luma_block_negated), so what can go wrong is a range or an offset
at which the fixed point, the wrap-around or the junk byte moves a pixel to its neighbour's code, or the two end bytes
changing places.  tests/test_luma_row_identity.py holds the arithmetic on the CPU; this holds the instructions.

  blocks:  oracle/bc_oracle.c (the texture)
  stream:  oracle/field_stream_oracle.c (every fragment's bytes, size and group table)

Pictures (tests/_luma_ramp.py):
  ramp    256 x 256, 4096 blocks: every luma range 1..255 at sixteen offsets, pixels on both ends and in between, f = 0..3
          from unequal R, G, B of the same Y, chroma flat in the left half and busy in the right
  turned  the same turned by 180 degrees (the second picture of a batch)
  small   64 x 68, 272 blocks: no whole number of fragments

Roads: HapGpuEncodeFramesRGBA fused with the fragments placed (8 frames, the placing threshold) and a batch of two
frames, the kernel class asserted from the context's profile, the placement counters unchanged; and HapGpuCompressRGBA
(bc_encode.hip, the block-per-lane kernel, which keeps the centred form).  The oracle's textures are made once."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _luma_ramp as R
import test_fused_encode_shapes_gpu as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


_made = {}


def made():
    """{name: (picture, the oracle's texture)}: made once, shared, left unchanged."""
    if not _made:
        ramp = R.ramp_picture()
        turned = np.ascontiguousarray(ramp[::-1, ::-1])
        for name, img in (("ramp", ramp), ("turned", turned), ("small", R.small_picture(ramp)),
                          ("small-turned", R.small_picture(turned))):
            _made[name] = (img, D.oracle_bc_encode(img, L.FMT_YCOCG))
    return _made


def test_picture_set_is_what_it_says():
    img, tex = made()["ramp"]
    assert img.shape == (256, 256, 4) and made()["small"][0].shape == (68, 64, 4)
    assert (68 // 4) * (64 // 4) % S.FRAG_BLOCKS != 0
    luma = np.frombuffer(tex, dtype=np.uint8).reshape(64, 64, 16).astype(np.int64)
    d, a1 = luma[..., 0] - luma[..., 1], luma[..., 1]
    assert set(np.unique(d).tolist()) == set(range(1, 256))
    for rng in range(1, 256):                                                   # sixteen offsets a range, both ends of the scale
        offs = np.unique(a1[d == rng])
        assert len(offs) == min(16, 256 - rng) and offs[0] == 0 and offs[-1] == 255 - rng, rng
    s = img[..., 0].astype(np.int64) + 2 * img[..., 1].astype(np.int64) + img[..., 2].astype(np.int64) + 2
    assert [int(((s & 3) == f).sum()) > 10000 for f in range(4)] == [True] * 4   # every junk byte, often
    assert set(np.unique(R.row0(img) & 0xFF).tolist()) == {0, 64, 128, 192}
    assert (img[..., 0] != img[..., 1]).mean() > 0.5                             # unequal channels
    chroma = np.frombuffer(tex, dtype=np.uint8).reshape(64, 64, 16)[..., 8:]
    assert (chroma[:, :32] == chroma[0, 0]).all() and (chroma[:, 32:, 4:] != 0).any(axis=-1).mean() > 0.9
    codes = luma[..., 2:8]                                                       # pixels on the ends and in between
    assert (codes != 0).any(axis=-1).all()


def test_block_per_lane_kernel_writes_the_oracles_texture(ctx):
    for name, (img, tex) in made().items():
        h, w = img.shape[:2]
        r, got = ctx.compress_rgba(torch.from_numpy(img).cuda(), w, h, w * 4, L.FMT_YCOCG)
        assert r == 0, name
        if got != tex:
            a, b = np.frombuffer(got, dtype=np.uint8).reshape(-1, 16), np.frombuffer(tex, dtype=np.uint8).reshape(-1, 16)
            bad = np.flatnonzero((a != b).any(axis=1))
            raise AssertionError("%s: %d of %d blocks differ, first %d: %s against %s" %
                                 (name, len(bad), len(a), bad[0], a[bad[0]].tobytes().hex(), b[bad[0]].tobytes().hex()))


@pytest.mark.parametrize("names,batch", [(("ramp", "turned"), 8), (("small", "small-turned"), 8), (("ramp", "turned"), 2)],
                         ids=["ramp-placed", "small-placed", "ramp-two-frames"])
def test_fused_kernel_writes_the_oracles_bytes(ctx, hap, names, batch):
    fmt, chunks = L.FMT_YCOCG, 1
    h, w = made()[names[0]][0].shape[:2]
    tex = [made()[n][1] for n in names]
    dev = [torch.from_numpy(made()[n][0]).cuda() for n in names]
    size = len(tex[0])
    cap = hap.HapMaxEncodedLength([size], [fmt], [chunks])
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    t0, r0 = ctx.placement_timeouts(), ctx.placement_retries()
    (r, used, res), launches = S.profiled(ctx, lambda: ctx.encode_frames_rgba(
        [dev[i % len(dev)] for i in range(batch)], w, h, w * 4, [fmt], [1], [chunks], outs,
        flags=hap.ENCODE_FRAGMENT_INDEX))
    assert r == 0 and res == [0] * batch, (names, batch)
    assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    assert (ctx.placement_timeouts(), ctx.placement_retries()) == (t0, r0)
    frames = [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]
    for i, name in enumerate(names):
        got = S.ORA.decode(frames[i], 0, size)
        if got != (0, tex[i], fmt):
            a, b = np.frombuffer(got[1], dtype=np.uint8).reshape(-1, 16), np.frombuffer(tex[i], dtype=np.uint8).reshape(-1, 16)
            bad = np.flatnonzero((a != b).any(axis=1))
            raise AssertionError("%s: %d of %d blocks differ, first %d: %s against %s" %
                                 (name, len(bad), len(a), bad[0], a[bad[0]].tobytes().hex(), b[bad[0]].tobytes().hex()))
        S.frame_against_oracle(frames[i], tex[i], fmt, chunks, (name, batch))
    for i in range(len(names), batch):
        assert frames[i] == frames[i % len(names)], (names, batch, i)

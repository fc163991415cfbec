"""The Hap Q encoders at the ends of the chroma range, byte for byte against the scalar definition.  The fused kernel's
colour half keeps Co | Cg as NON-NEGATIVE halves 1..256 (hap_amd/csrc/bc_encode_core.hpp, BIASED: the transform's addend
tuple, the box by three-input packed half minima / maxima, the sums by 32-bit adds, the projection constant with the
bias folded in), so what can go wrong is at 1, 2, 255 and 256, in flat blocks, and where a channel spans the whole
range.  The block-per-lane kernel keeps the centred form and must write the same bytes from the same pictures.

  blocks:  oracle/bc_oracle.c (the texture)
  stream:  oracle/field_stream_oracle.c (every fragment's bytes, size and group table)

The picture set (tests/_biased_pairs.py; none larger than 256 x 64, one or two fragments):
  (a) every (R, B) that makes Co - 128 one of -127, -126, 0, 127, 128, with the G that make Cg - 128 one of them
  (b) flat blocks at those extremes (c0 == c1)        (c) the box 1..256 in one channel, flat in the other
  (d) 4 x 4 blocks of hap_amd.synth noise at each scale        (e) 256 x 60: the last fragment ragged

Roads: HapGpuEncodeFramesRGBA fused with the fragments placed (8 frames) and through slots (7), asserted from the
context's profile, and HapGpuCompressRGBA (bc_encode.hip).  The oracle's textures are made once and shared."""
import numpy as np
import pytest

import _biased_pairs as BP
import _data as D
import _libs as L
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
        for name, img in BP.pictures().items():
            img = np.ascontiguousarray(img)
            _made[name] = (img, D.oracle_bc_encode(img, L.FMT_YCOCG))
    return _made


def groups():
    """The pictures by geometry: one fused call a geometry."""
    by = {}
    for name, (img, _tex) in made().items():
        by.setdefault(img.shape[:2], []).append(name)
    return by


def test_picture_set_is_what_it_says():
    shapes = {name: img.shape for name, (img, _t) in made().items()}
    assert all(h <= 64 and w <= 256 and h % 4 == 0 and w % 4 == 0 for h, w, _c in shapes.values()), shapes
    assert shapes["e"] == (60, 256, 4) and (60 // 4) * (256 // 4) % S.FRAG_BLOCKS == 448
    assert sum(1 for n in shapes if n.startswith("a")) >= 1 and "bc" in shapes
    assert {n for n in shapes if n.startswith("d-")} == {"d-scale1", "d-scale2", "d-scale4"}
    assert all(shapes[n] == (16, 16, 4) for n in shapes if n.startswith("d-"))
    for scale in (1, 2, 4):                                   # the blue field of c0 carries s - 1
        tex = np.frombuffer(made()["d-scale%d" % scale][1], dtype=np.uint8).reshape(-1, 16)
        assert ((tex[:, 8] & 31) == scale - 1).mean() >= 0.5, scale


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


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
def test_fused_kernel_writes_the_oracles_bytes(ctx, hap, batch):
    fmt, chunks = L.FMT_YCOCG, 1
    for (h, w), names in sorted(groups().items(), reverse=True):        # (the 256-byte pictures last: see below)
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
        assert r == 0 and res == [0] * batch, (w, h, batch)
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
        frames = [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]
        stored = [S.P.find_fragment_table(frames[i], 0, 4000)[1] == 0 for i in range(len(names))]
        # only the 256-byte textures of (d) may be stored as they are (a call of such frames is encoded a second time
        # without placing, which is the library's rule for frames that do not shrink, not this test's subject)
        assert not any(stored) or size == 256, (names, stored)
        if not any(stored):
            assert (ctx.placement_timeouts(), ctx.placement_retries()) == (t0, r0)
        for i, name in enumerate(names):
            assert S.ORA.decode(frames[i], 0, size) == (0, tex[i], fmt), (name, batch)
            if stored[i]:
                # right only if the definition's stream for the one fragment is no shorter than the texture -- and then
                # the frame is its header and the texture
                assert len(S.P._varint(size) + S.P._ofs_fragment(tex[i], 4, 0)[0]) >= size, (name, batch)
                assert frames[i][-size:] == tex[i] and len(frames[i]) <= size + 8, (name, batch)
            else:
                S.frame_against_oracle(frames[i], tex[i], fmt, chunks, (name, batch))
        for i in range(len(names), batch):
            assert frames[i] == frames[i % len(names)], (w, h, batch, i)

"""The fused kernel's set-up (snappy_compress_blocks.hip): which frame and fragment a workgroup takes (the interleave
of a single-texture launch: workgroup number / frames and its remainder), the fragment's chunk, and the block row and
column of every lane's first block -- quotients the kernel takes with the host's reciprocals
(hapgpu_abi.h, HAPGPU_DIV_INV), a multiply-high and one correction each.

Fused calls of 8, 9, 11 and 13 frames (the interleave's divisor), on three picture widths:

  64 wide      16 blocks a row: a wavefront's 64 blocks span four block rows; two chunks of two fragments
  260 wide     65 blocks a row: one block more than a wavefront
  1920 wide    480 blocks a row

Every picture's last fragment is partly empty.  Hap Q and DXT5 (the two fused kernels), against the scalar definition
(oracle/bc_oracle.c, oracle/field_stream_oracle.c) byte for byte: a fragment that no workgroup took, or a lane that
read another block's pixels, shows in the frame's bytes."""
import pytest

import _data as D
import _libs as L
import test_fused_encode_shapes_gpu as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FRAG_BLOCKS = S.FRAG_BLOCKS


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


def pictures(w, h, fmt):
    """Two pictures of a geometry, their textures by the oracle and their device copies: made once, shared."""
    if (w, h, fmt) not in _made:
        pics = [D.rgba(w, h, frame=71 + i) for i in range(2)]
        _made[(w, h, fmt)] = ([D.oracle_bc_encode(p, fmt) for p in pics], [torch.from_numpy(p).cuda() for p in pics])
    return _made[(w, h, fmt)]


# (width, height, chunks, blocks in the last fragment of a chunk)
GEOMETRIES = [
    pytest.param(64, 320, 2, 128, id="16-blocks-a-row"),
    pytest.param(260, 36, 1, 73, id="65-blocks-a-row"),
    pytest.param(1920, 12, 1, 416, id="480-blocks-a-row"),
]


@pytest.mark.parametrize("batch", [8, 9, 11, 13])
@pytest.mark.parametrize("w,h,chunks,tail", GEOMETRIES)
def test_every_workgroup_finds_its_frame_fragment_and_blocks(ctx, hap, w, h, chunks, tail, batch):
    blocks = (w // 4) * (h // 4)
    assert blocks % chunks == 0 and (blocks // chunks) % FRAG_BLOCKS == tail and blocks // chunks > FRAG_BLOCKS
    for fmt in (L.FMT_YCOCG, L.FMT_DXT5):
        tex, dev = pictures(w, h, fmt)
        size = len(tex[0])
        cap = hap.HapMaxEncodedLength([size], [fmt], [chunks])
        # two pictures dealt out without a period (the oracle's work stays small)
        order = [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0][:batch]
        outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
        torch.cuda.synchronize()
        t0, r0 = ctx.placement_timeouts(), ctx.placement_retries()
        (r, used, res), launches = S.profiled(ctx, lambda: ctx.encode_frames_rgba(
            [dev[k] for k in order], w, h, w * 4, [fmt], [1], [chunks], outs, flags=hap.ENCODE_FRAGMENT_INDEX))
        assert r == 0 and res == [0] * batch, (w, h, fmt, batch)
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
        assert (ctx.placement_timeouts(), ctx.placement_retries()) == (t0, r0)
        frames = [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]
        for i in range(2):
            S.frame_against_oracle(frames[i], tex[i], fmt, chunks, (w, h, fmt, batch, i))
            assert S.ORA.decode(frames[i], 0, size) == (0, tex[i], fmt)
        assert frames[0] != frames[1]
        for i in range(2, batch):
            assert frames[i] == frames[order[i]], (w, h, fmt, batch, i)

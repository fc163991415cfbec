"""The fused RGBA -> blocks -> field stream kernel (snappy_compress_blocks_kernel<4, YCoCg / DXT5>) against the oracle,
byte for byte, on pictures whose fragment geometry reaches the corners of its step loop: a first step with fewer than
four blocks in front of a unit, full interior steps, a last step that is partly or wholly empty, block rows shorter
and longer than a wavefront's 64 blocks, fragments that wrap around several block rows.

  blocks:  oracle/bc_oracle.c (the texture the reference decodes from the frame)
  stream:  oracle/field_stream_oracle.c (every fragment's bytes, size and group table)

Each geometry runs as a batch of 8 frames (the placing threshold: the fragments are written straight into the frames)
and of 7 (below it: slots and a gather pass); the kernel class that ran is asserted from the context's profile, and the
placed road must neither time out nor encode a frame twice.

The value-space sweeps (tests/_value_space.py) already go through the fused kernel in
tests/test_value_space_gpu.py::test_encode_frames_rgba_sweeps (road "default", asserted there from the profile); they
are not repeated here."""
import numpy as np
import pytest

import _data as D
import _libs as L
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()
FRAG_BLOCKS = 8192 // 16


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


def frame_against_oracle(frame, tex, fmt, chunks, what):
    """Every section of a one-texture frame with the version-4 fragment table equals the scalar definition's."""
    limited = ORA.chunk_count(P._encode_with(ORA, tex, fmt, L.COMP_SNAPPY, chunks), 0)[1]
    codecs, sizes, frag_sizes, half, at = P._own_frame_sections(frame, limited)
    cb = len(tex) // limited
    fi = 0
    for c in range(limited):
        assert codecs[c] == 0x0B, (what, c)
        want = P._varint(cb)
        for o in range(0, cb, 8192):
            piece, halves = P._ofs_fragment(tex[c * cb + o: c * cb + min(cb, o + 8192)], 4, 0)
            assert frag_sizes[fi] == len(piece), (what, c, o)
            assert P._unpack_groups(half[fi].tobytes()) == P._unpack_groups(halves), (what, c, o)
            want += piece
            fi += 1
        assert sizes[c] == len(want), (what, c)
        got = frame[at: at + sizes[c]]
        if got != want:
            bad = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError("%s: chunk %d differs at stream byte %d of %d" % (what, c, bad, len(want)))
        at += sizes[c]
    assert fi == len(frag_sizes) and at == len(frame), what


def profiled(ctx, call):
    ctx.set_profiling(True)
    ctx.collect_profile()
    try:
        out = call()
        prof = ctx.collect_profile()
    finally:
        ctx.set_profiling(False)
    return out, {k: v[0] for k, v in prof.items()}


# (width, height, chunks): the last fragment of the one chunk holds `tail` blocks
#   widths 4 / 252 / 256 / 260 / 7680: 1, 63, 64, 65 and 1920 blocks per block row
GEOMETRIES = [
    pytest.param(4, 4 * (FRAG_BLOCKS + 1), 1, 1, id="w4-tail1"),
    pytest.param(252, 4 * 513, 1, 63, id="w252-tail63"),
    pytest.param(256, 4 * 9, 1, 64, id="w256-tail64"),
    pytest.param(260, 4 * 513, 1, 65, id="w260-tail65"),
    pytest.param(4, 4 * (2 * FRAG_BLOCKS - 1), 1, 511, id="w4-tail511"),
    pytest.param(7680, 8, 1, 256, id="w7680-tail256"),
    pytest.param(7680, 64, 4, 0, id="w7680-4chunks-full"),
    pytest.param(260, 4 * 16, 1, 16, id="w260-tail16"),
]


@pytest.mark.parametrize("batch", [8, 7], ids=["placed", "slots"])
@pytest.mark.parametrize("w,h,chunks,tail", GEOMETRIES)
def test_fused_kernel_writes_the_oracles_bytes(ctx, hap, w, h, chunks, tail, batch):
    blocks = (w // 4) * (h // 4)
    assert (blocks // chunks) % FRAG_BLOCKS == tail % FRAG_BLOCKS           # the geometry is what its name says
    for fmt in (L.FMT_YCOCG, L.FMT_DXT5):
        # two different pictures, dealt out over the batch (the oracle's work stays small)
        pics = [D.rgba(w, h, frame=31 + i) for i in range(2)]
        tex = [D.oracle_bc_encode(p, fmt) for p in pics]
        size = len(tex[0])
        cap = hap.HapMaxEncodedLength([size], [fmt], [chunks])
        dev = [torch.from_numpy(p).cuda() for p in pics]
        bufs = [dev[i & 1] for i in range(batch)]
        outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
        torch.cuda.synchronize()
        t0, r0 = ctx.placement_timeouts(), ctx.placement_retries()
        (r, used, res), launches = profiled(ctx, lambda: ctx.encode_frames_rgba(
            bufs, w, h, w * 4, [fmt], [1], [chunks], outs, flags=hap.ENCODE_FRAGMENT_INDEX))
        assert r == 0 and res == [0] * batch, (w, h, fmt, batch)
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
        assert (ctx.placement_timeouts(), ctx.placement_retries()) == (t0, r0)
        frames = [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]
        for i in range(2):
            frame_against_oracle(frames[i], tex[i], fmt, chunks, (w, h, fmt, batch, i))
            assert ORA.decode(frames[i], 0, size) == (0, tex[i], fmt)
        for i in range(2, batch):
            assert frames[i] == frames[i & 1], (w, h, fmt, batch, i)

"""The placed road's look-back (snappy_compress_blocks.hip, "placed streams"): a fragment finds its place in the frame
from the totals of the chunks before its own and the published sizes of the fragments before it in its chunk, both read
64 words a turn and added up across the wavefront -- in 32 bits, by DPP adds.  Pictures whose geometry makes the
in-chunk loop run one, two and three turns, and the chunk loop run over 63 chunks:

  1024 x 1040 Hap Q, one chunk     130 fragments: up to three turns over the fragments, no chunk before
  the same, two chunks             65 fragments a chunk: up to two turns, one chunk total
  1024 x 1280 Hap Q, 64 chunks     three fragments a chunk, the last one half empty: one turn, up to 63 chunk totals

Each runs as a placed batch of 8 frames, which must give the bytes of the 7-frame call (slots and a gather pass) and of
the scalar definition (oracle/bc_oracle.c, oracle/field_stream_oracle.c), without a time-out or a second encode; the
kernel class is asserted from the context's profile."""
import pytest

import _data as D
import _libs as L
import test_fused_encode_shapes_gpu as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = L.FMT_YCOCG


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


def picture(w, h):
    """The picture of a geometry, its texture by the oracle and its device copy: made once, shared, left unchanged."""
    if (w, h) not in _made:
        pic = D.rgba(w, h, frame=57)
        _made[(w, h)] = (D.oracle_bc_encode(pic, FMT), torch.from_numpy(pic).cuda())
    return _made[(w, h)]


def encode(ctx, hap, dev, w, h, chunks, size, batch):
    cap = hap.HapMaxEncodedLength([size], [FMT], [chunks])
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    (r, used, res), launches = S.profiled(ctx, lambda: ctx.encode_frames_rgba(
        [dev] * batch, w, h, w * 4, [FMT], [1], [chunks], outs, flags=hap.ENCODE_FRAGMENT_INDEX))
    assert r == 0 and res == [0] * batch, (w, h, chunks, batch)
    assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    return [outs[i][: used[i]].cpu().numpy().tobytes() for i in range(batch)]


# (width, height, chunks, fragments a chunk)
GEOMETRIES = [
    pytest.param(1024, 1040, 1, 130, id="1chunk-130frags"),
    pytest.param(1024, 1040, 2, 65, id="2chunks-65frags"),
    pytest.param(1024, 1280, 64, 3, id="64chunks-3frags"),
]


@pytest.mark.parametrize("w,h,chunks,fpc", GEOMETRIES)
def test_placed_fragments_lie_where_the_gather_puts_them(ctx, hap, w, h, chunks, fpc):
    tex, dev = picture(w, h)
    assert -(-(len(tex) // chunks) // 8192) == fpc and len(tex) % chunks == 0       # the geometry is what its name says
    placed = encode(ctx, hap, dev, w, h, chunks, len(tex), 8)
    slots = encode(ctx, hap, dev, w, h, chunks, len(tex), 7)
    assert (ctx.placement_timeouts(), ctx.placement_retries()) == (0, 0)
    S.frame_against_oracle(placed[0], tex, FMT, chunks, (w, h, chunks, "placed"))
    assert S.ORA.decode(placed[0], 0, len(tex)) == (0, tex, FMT)
    for i, frame in enumerate(placed[1:] + slots):
        assert frame == placed[0], (w, h, chunks, i)

"""GPU half of the pair form of the Hap Q colour half and of the ramp multiplier taken from v_rcp_f32 as it comes
(hap_amd/csrc/bc_encode_core.hpp: ycocg_colour_block, alpha_block): the smallest pictures at which a block can go
wrong, through the unfused block encoder (HapGpuCompressRGBA, Hap Q) and through the fused road
(HapGpuEncodeFramesRGBA, one frame, the frame decoded to its texture by the oracle), byte for byte against
oracle/bc_oracle.c.

  box grid      two-colour blocks whose Co / Cg box corners run over -127, 128 and the thresholds 31 / 32 and 63 / 64 of
                the scale rule, both covariance signs, both orders of the two 5:6:5 words (tests/_packed_endpoints.py;
                what the grid holds is asserted in tests/test_packed_endpoints_identity.py)
  luma ranges   every d = 1..255 at several minima, every position 0..d present: floor(2^19 / d) for every d; also as
                DXT5 and RGTC1 blocks (A = the grey), whose kernels share alpha_block
  shapes        the box grid in a picture of one full fragment (512 blocks) and in one whose last step is partial
                (65 blocks a row, 1040 blocks: two fragments and 16 blocks)

The kernel class that ran is asserted from the context's profile."""
import numpy as np
import pytest

import _data as D
import _libs as L
import _packed_endpoints as PE
import _value_space as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORA = L.oracle_api()


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


def profiled(ctx, call):
    ctx.set_profiling(True)
    ctx.collect_profile()
    try:
        out = call()
        prof = ctx.collect_profile()
    finally:
        ctx.set_profiling(False)
    return out, {k: v[0] for k, v in prof.items()}


_pictures, _oracle = {}, {}


def picture(name):
    """(picture, blocks per picture row)"""
    if name not in _pictures:
        if name == "box_grid":
            _pictures[name] = (V.picture_of_blocks(PE.box_grid_blocks()[0]), V.BLOCK_ROW)
        elif name == "luma_ranges":
            _pictures[name] = (V.picture_of_blocks(PE.luma_range_blocks()), V.BLOCK_ROW)
        elif name == "one_fragment":
            _pictures[name] = (V.picture_of_blocks(PE.box_grid_blocks()[0][:512], row=64), 64)
        else:
            assert name == "partial_last_step"
            _pictures[name] = (V.picture_of_blocks(PE.box_grid_blocks()[0][1000:1000 + 1040], row=65), 65)
    return _pictures[name]


def oracle_blocks(name, fmt):
    if (name, fmt) not in _oracle:
        _oracle[(name, fmt)] = D.oracle_bc_encode(picture(name)[0], fmt)
    return _oracle[(name, fmt)]


def check_blocks(got, name, fmt, what):
    bb = D.BLOCK_BYTES[fmt]
    want = np.frombuffer(oracle_blocks(name, fmt), dtype=np.uint8).reshape(-1, bb)
    got = np.frombuffer(bytes(got), dtype=np.uint8).reshape(-1, bb)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        i = int(bad[0])
        px = V.blocks_of_picture(picture(name)[0])[i]
        pytest.fail("%s %s %#x: %d of %d blocks differ; first: block %d\n  input  %s\n  kernel %s\n  oracle %s" % (
            what, name, fmt, len(bad), len(got), i, px.tolist(), got[i].tolist(), want[i].tolist()))


CASES = [("box_grid", L.FMT_YCOCG, 4), ("luma_ranges", L.FMT_YCOCG, 4), ("luma_ranges", L.FMT_DXT5, 4),
         ("luma_ranges", L.FMT_RGTC1, 4), ("one_fragment", L.FMT_YCOCG, 1), ("partial_last_step", L.FMT_YCOCG, 1)]
IDS = ["%s-%#x" % (n, f) for n, f, _c in CASES]


def test_the_shapes_are_what_their_names_say():
    img, row = picture("one_fragment")
    assert (img.shape[0] // 4) * row * 16 == 8192
    img, row = picture("partial_last_step")
    assert row == 65 and ((img.shape[0] // 4) * row) % 512 == 16


@pytest.mark.parametrize("name,fmt,chunks", CASES, ids=IDS)
def test_block_encoder_writes_the_oracles_blocks(ctx, name, fmt, chunks):
    img, _row = picture(name)
    h, w = img.shape[:2]
    src = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    (r, got), launches = profiled(ctx, lambda: ctx.compress_rgba(src, w, h, w * 4, fmt))
    assert r == 0 and launches["block_encode"] >= 1, (r, launches)
    check_blocks(got, name, fmt, "HapGpuCompressRGBA")


@pytest.mark.parametrize("name,fmt,chunks", CASES, ids=IDS)
def test_frame_encoder_writes_the_oracles_blocks(ctx, hap, name, fmt, chunks):
    img, _row = picture(name)
    h, w = img.shape[:2]
    size = (w // 4) * (h // 4) * D.BLOCK_BYTES[fmt]
    cap = hap.HapMaxEncodedLength([size], [fmt], [chunks])
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    (r, used, results), launches = profiled(ctx, lambda: ctx.encode_frames_rgba([src], w, h, w * 4, [fmt], [1], [chunks], [out]))
    assert r == 0 and results == [0], (r, results)
    if fmt == L.FMT_RGTC1:
        assert launches["block_encode"] >= 1 and launches["encode_fused"] == 0, launches
    else:
        assert launches["encode_fused"] >= 1 and launches["block_encode"] == 0, launches
    code, tex, got_fmt = ORA.decode_np(out[: used[0]].cpu().numpy(), 0, size)
    assert code == 0 and got_fmt == fmt and len(tex) == size, (code, got_fmt)
    check_blocks(tex.tobytes(), name, fmt, "HapGpuEncodeFramesRGBA")

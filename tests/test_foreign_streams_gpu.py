"""Other encoders' Snappy streams, swept over the element grammar (tests/_snappy_streams.py), through each of the three
roads hap_amd/csrc/snappy_decode.hip has for them:

  1. the whole stream by one wavefront with a 32 KiB ring            (HAPGPU_DECODE_NO_BLOCK_SCAN)
  2. a wavefront per 64 KiB block the block scan finds, 2 KiB ring   (a call of more than 256 scanned streams)
  3. a workgroup per 64 KiB block                                    (calls of at most 256 streams and 4 x CUs blocks)

The reference is the plain decoder of _snappy_streams, which tests/test_snappy_streams.py holds to libsnappy.  Road 3
returns without a word from whatever surprises it and road 2 then writes the block again, so bytes alone prove
nothing about it: HapGpuResolvedBlockCount must rise by exactly the number of blocks the generators say it takes."""
import numpy as np
import pytest

import _libs as L
import _snappy_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = S.K
MAX_STREAMS = 256                 # scanned streams of a call the workgroup-per-block kernel is launched for
SENTINEL = 0x5A
VARIANTS = {"host": ("host", 0), "device, odd address": ("device", 1)}


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


def _blocks_estimate(stream):
    """No less than the host's own estimate for a scanned stream (an eighth of its 8 KiB slots, which are bounded by
    the texture's 8 KiB pieces plus one per stream)"""
    return (len(S.decoded(stream)) + K - 1) // K + 1


def _calls(cases):
    """The sweep's cases in as few calls as keep each within what the workgroup-per-block kernel is launched for.
    The one stream that is not made of independent blocks has a call, and a test, of its own."""
    max_blocks = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    calls, blocks = [[]], 1
    for case in cases:
        need = _blocks_estimate(case[1])
        alone = case[0] == S.REACHING_STREAM
        if calls[-1] and (alone or calls[-1][-1][0] == S.REACHING_STREAM or len(calls[-1]) == MAX_STREAMS or blocks + need > max_blocks):
            calls.append([])
            blocks = 1
        calls[-1].append(case)
        blocks += need
    return calls


def _frame(streams):
    return S.frame_of_streams(list(streams))


def _decode(ctx, streams, flags=0, where="host", odd=0):
    """One frame with a chunk per stream, decoded into the middle of a sentinel-filled buffer.
    Returns ((r, used, results), bytes, whether the bytes around the output are untouched, the format)."""
    frame = _frame(streams)
    need = sum(len(S.decoded(s)) for s in streams)
    if where == "device":
        src = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda()
        backing = torch.full((need + 48,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = backing[16 + odd: 16 + odd + need]
        torch.cuda.synchronize()
    else:
        src = frame
        backing = np.full(need + 48, SENTINEL, dtype=np.uint8)
        out = backing[16 + odd: 16 + odd + need]
    r, used, fmts, res = ctx.decode_frames([src], [len(frame)], 0, [out], flags)
    whole = backing.cpu().numpy() if where == "device" else backing
    around = bytes(whole[: 16 + odd]) + bytes(whole[16 + odd + need:])
    return (r, used, res), bytes(whole[16 + odd: 16 + odd + need]), around == bytes([SENTINEL]) * 48, fmts[0]


def _want(streams):
    return b"".join(S.decoded(s) for s in streams)


def _first_difference(got, want):
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    return "first wrong byte %d (block %d, byte %d of it): %d for %d" % (at, at // K, at % K, a[at], b[at])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sweep", list(S.SWEEPS))
def test_a_workgroup_per_block_takes_every_block_it_is_meant_to(ctx, hap, sweep, variant):
    """Road 3.  Bytes, the bytes around the output, the result codes, no second pass -- and the counter: every block
    of sweeps a-f, and of sweep g all but the blocks of more than 1024 windows."""
    where, odd = VARIANTS[variant]
    for call in _calls([c for c in S.SWEEPS[sweep]() if c[0] != S.REACHING_STREAM]):
        streams = [s for _n, s, _e in call]
        want = _want(streams)
        n0, f0 = ctx.resolved_blocks(), ctx.table_fallbacks()
        status, got, untouched, fmt = _decode(ctx, streams, 0, where, odd)
        taken = ctx.resolved_blocks() - n0
        assert status == (0, [len(want)], [0]) and fmt == L.FMT_DXT5, (sweep, status)
        assert got == want, (sweep, _first_difference(got, want))
        assert untouched, sweep
        assert ctx.table_fallbacks() == f0, sweep
        expected = sum(e for _n, _s, e in call)
        print("%s, %s: %d streams, %d blocks expected, %d taken" % (sweep, variant, len(call), expected, taken))
        if taken != expected:
            # which stream is it?  each in a call of its own
            wrong = []
            for name, stream, e in call:
                n1 = ctx.resolved_blocks()
                _decode(ctx, [stream], 0, where, odd)
                if ctx.resolved_blocks() - n1 != e:
                    wrong.append("%s: %d of %d" % (name, ctx.resolved_blocks() - n1, e))
            assert taken == expected, "%s: %d blocks taken of %d; alone: %s" % (sweep, taken, expected, "; ".join(wrong[:12]) or "all as expected")


def test_a_stream_of_dependent_blocks_is_left_to_the_whole_stream_decoder(ctx, hap):
    """Sweep g's last case: the second block copies from the first.  The bytes are the plain decoder's; no block of
    the stream counts as taken by a workgroup, although one had taken the first, independent block before the second was
    found to reach back; and the frame is not decoded a second time: the workgroup that verified the second block's
    chain hands the stream to its whole-stream unit of the same call."""
    (name, stream, expected), = [c for c in S.sweep_declines() if c[0] == S.REACHING_STREAM]
    want = S.decoded(stream)
    for where, odd in VARIANTS.values():
        n0, f0 = ctx.resolved_blocks(), ctx.table_fallbacks()
        status, got, untouched, _fmt = _decode(ctx, [stream], 0, where, odd)
        taken, again = ctx.resolved_blocks() - n0, ctx.table_fallbacks() - f0
        print("%s, %s: %d blocks taken, %d frames decoded again" % (name, where, taken, again))
        assert status == (0, [len(want)], [0]) and got == want and untouched
        assert taken == expected == 0
        assert again == 0


@pytest.mark.parametrize("sweep", list(S.SWEEPS))
def test_a_wavefront_per_block_decodes_the_same(ctx, hap, sweep):
    """Road 2: the same streams, repeated until the call holds more than 256 scanned streams -- more than the
    workgroup-per-block kernel is launched for, so its counter stands still -- with the block scan running.  The library
    has no counter that tells a block decoded by its own wavefront from a stream that fell back to road 1 (the frame
    decoded again whole counts in table_fallbacks, a stream whose marks were not all found counts nowhere): the proof
    of the road is the shape of the call and the scan's launches."""
    streams = [s for _n, s, _e in S.SWEEPS[sweep]()]
    many = streams * -(-(MAX_STREAMS + 1) // len(streams))
    assert len(many) > MAX_STREAMS
    frame = _frame(many)
    want = _want(streams) * (len(many) // len(streams))
    src = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda()
    out = torch.full((len(want),), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n0 = ctx.resolved_blocks()
    ctx.set_profiling(True)
    ctx.collect_profile()
    r, used, fmts, res = ctx.decode_frames([src], [len(frame)], 0, [out])
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    got = out.cpu().numpy().tobytes()
    assert (r, used, res) == (0, [len(want)], [0]), sweep
    assert got == want, (sweep, _first_difference(got, want))
    assert ctx.resolved_blocks() == n0
    assert prof["block_scan"][0] > 0, prof


@pytest.mark.parametrize("sweep", list(S.SWEEPS))
def test_the_whole_stream_decoder_decodes_the_same(ctx, hap, sweep):
    """Road 1: no block scan, one wavefront per stream, sources older than its 32 KiB ring read back from memory"""
    streams = [s for _n, s, _e in S.SWEEPS[sweep]()]
    want = _want(streams)
    for where, odd in VARIANTS.values():
        n0 = ctx.resolved_blocks()
        status, got, untouched, _fmt = _decode(ctx, streams, hap.DECODE_NO_BLOCK_SCAN, where, odd)
        assert status == (0, [len(want)], [0]), (sweep, status)
        assert got == want, (sweep, _first_difference(got, want))
        assert untouched and ctx.resolved_blocks() == n0, sweep


@pytest.mark.parametrize("sweep", ["phase", "lengths"])
def test_plain_hapdecode_decodes_the_same(hap, sweep):
    """... and through hap.h's HapDecode, which has its own context"""
    for call in _calls(S.SWEEPS[sweep]()):
        streams = [s for _n, s, _e in call]
        want = _want(streams)
        assert hap.HapDecode(_frame(streams), 0, outputBufferBytes=len(want)) == (0, want, L.FMT_DXT5), sweep

"""The hand-built fragments of tests/_fragment_streams.py through snappy_decode_fragment_kernel<RING, false, GRAN, SLIDE>
(hap_amd/csrc/snappy_decode.hip): the fifteen decoders that decode_expand_kernel feeds from a version-1 fragment table
-- GRAN 1, 2 and 4 with rings of 8, 16, 32 and 64 KiB, and the three windowed ones with a ring of 4 KiB.

The expected bytes are the ones the fragment builders recorded (tests/test_fragment_streams.py holds them to the plain
decoder and to the checker libraries); every output lies in the middle of sentinel-filled memory.  For honest frames
table_fallbacks() must stand still: the fragment kernel of that GRAN, ring and SLIDE made the bytes, not a second pass
through the whole-stream kernel.  Every lie sits beside honest frames in one call and must raise the count by one: the
promise is looked at.  A launch takes one fragment size, so the families run one call per size."""
import collections
import time

import numpy as np
import pytest

import _fragment_streams as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x5A
GAP = 32                                  # sentinel bytes in front of and behind every output
GRANS = list(X.GRANS)


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


Built = collections.namedtuple("Built", "label frame want code size fragments starts")
# want: None where the frame is no Snappy (code: what it must return); size: bytes of its output buffer


def _build(label, chunks, frag_log2, gran, window256=0, version=1):
    b = X.frame_of_fragments(chunks, frag_log2, X.GRAN_LOG2[gran], window256, version=version)
    return Built("%s, table byte %d%s" % (label, window256, ", version 3" if version == 3 else ""), b.frame, b.want, 0,
                 len(b.want), b.fragments, b.starts)


def _family(gran, families, frag_log2=None, window256=0, version=1):
    return [_build(fr.label, fr.chunks, fr.frag_log2, gran, window256, version) for fam in families
            for fr in X.family_frames(fam, gran) if (frag_log2 is None or fr.frag_log2 == frag_log2) and (fr.window_ok or not window256)]


def _lie(lie):
    b = X.frame_of_lie(lie)
    return Built(lie.name, b.frame, b.want, 0 if lie.valid else X.RESULT_OF_INVALID, 16384, b.fragments, b.starts)


def _per_frame(value, n):
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def _run(ctx, built, where="device", src_off=0, dst_off=0, met=None):
    """One decode_frames call: every frame from its own buffer (at src_off bytes into it), every output in the middle of
    sentinel-filled memory, 16-byte aligned plus dst_off.  Asserts results, formats, used bytes, output bytes and
    sentinels; returns the rise of table_fallbacks().  met: {(frame label, fragment): phases}, to which the address
    modulo 16 of every fragment's first byte in device memory is added -- the pointers handed to the library."""
    n = len(built)
    src_off, dst_off = _per_frame(src_off, n), _per_frame(dst_off, n)
    starts, at = [], 0
    for b, d in zip(built, dst_off):
        starts.append(at + GAP + d)
        at = (at + GAP + d + b.size + GAP + 15) & ~15
    expect = np.full(at, SENTINEL, dtype=np.uint8)
    for b, s in zip(built, starts):
        if b.want is not None:
            expect[s: s + b.size] = np.frombuffer(b.want, dtype=np.uint8)
    if where == "device":
        srcs = [torch.from_numpy(np.frombuffer(bytes(o) + b.frame, dtype=np.uint8).copy()).cuda()[o:] for b, o in zip(built, src_off)]
        backing = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if met is not None:
            for b, t in zip(built, srcs):
                for k, start in enumerate(b.starts):
                    met[(b.label, k)].add((t.data_ptr() + start) & 15)
    else:
        srcs = [b.frame for b in built]
        backing = np.full(at, SENTINEL, dtype=np.uint8)
    outs = [backing[s: s + b.size] for b, s in zip(built, starts)]
    n0 = ctx.table_fallbacks()
    r, used, fmts, res = ctx.decode_frames(srcs, [len(b.frame) for b in built], 0, outs, 0)
    rise = ctx.table_fallbacks() - n0
    got = backing.cpu().numpy() if where == "device" else backing
    codes = [b.code for b in built]
    assert res == codes and r == next((c for c in codes if c), 0), (r, [(b.label, c) for b, c in zip(built, res) if c != b.code])
    wrong = []
    for i, (b, s) in enumerate(zip(built, starts)):
        if b.want is None:
            got[s: s + b.size] = SENTINEL                 # (no Snappy: what lies in its own output is nobody's business)
            continue
        assert used[i] == b.size and fmts[i] == X.FMT_DXT5, b.label
        lo, hi = s - GAP, s + b.size + GAP
        bad = np.flatnonzero(got[lo:hi] != expect[lo:hi])
        if len(bad):
            wrong.append("%s: %s" % (b.label, _where(b, int(bad[0]) - GAP, got[lo + int(bad[0])], expect[lo + int(bad[0])])))
    if wrong:
        pytest.fail("%d frames wrong; %s" % (len(wrong), "; ".join(wrong[:16])))
    assert np.array_equal(got, expect), "sentinel bytes overwritten"
    return rise


def _where(b, at, got, want):
    if at < 0 or at >= b.size:
        return "sentinel byte %d overwritten with %d" % (at, got)
    p = 0
    for i, f in enumerate(b.fragments):
        if at < p + f.made:
            return "byte %d of fragment %d (%s): %d for %d" % (at - p, i, f.name, got, want)
        p += f.made
    return "byte %d" % at


def _count(built):
    return sum(len(b.fragments) for b in built)


@pytest.mark.parametrize("gran", GRANS)
def test_every_family_through_the_kernel_of_its_ring(ctx, gran):
    """Honest families, one call per fragment size with table byte 0: the plain kernels with rings of 8 (log2 10 and
    13), 16, 32 and 64 KiB.  At log2 13 the families whose offsets stay within 3072 again with table byte 12, and the
    window family with byte 1 as well: the windowed kernel.  No frame is decoded a second time -- and at every size a
    frame whose table is off by a byte is: the table, not a scan, is what these calls decode by."""
    t0 = time.time()
    decoded = frames = 0
    for frag_log2 in X.FRAG_LOG2S:
        calls = [_family(gran, X.FAMILIES, frag_log2)]
        if frag_log2 == 13:
            calls.append(_family(gran, X.FAMILIES, 13, X.WINDOW_BYTE))
            calls.append(_family(gran, ("window",), 13, 1))
            assert len(calls[2]) == 1
        for built in calls:
            assert built and _run(ctx, built) == 0, frag_log2
            decoded += _count(built)
            frames += len(built)
        # the table is what feeds the kernels at this size too: two of its entries moved by a byte send the frame round
        ring, = [fr for fr in X.family_frames("rings", gran) if fr.frag_log2 == frag_log2]
        (first, second), = ring.chunks
        moved = X.frame_of_fragments(ring.chunks, frag_log2, X.GRAN_LOG2[gran], 0, sizes=[first.total + 1, second.total - 1])
        lying = Built("table moved by a byte at log2 %d" % frag_log2, moved.frame, moved.want, 0, len(moved.want), moved.fragments, moved.starts)
        assert _run(ctx, calls[0][:1] + [lying] + calls[0][-1:]) == 1, frag_log2
    want = sum(len(c) for fam in X.FAMILIES for fr in X.family_frames(fam, gran) for c in fr.chunks)
    windowed = sum(len(c) for fam in X.FAMILIES for fr in X.family_frames(fam, gran) for c in fr.chunks if fr.window_ok and fr.frag_log2 == 13)
    assert decoded == want + windowed + len(X.fragments("window", gran))
    print("GRAN %d: %d honest fragments built, %d decoded in %d frames (%d again through the windowed kernel), %.2f s" % (
        gran, want, decoded, frames, windowed + len(X.fragments("window", gran)), time.time() - t0))


@pytest.mark.parametrize("gran", GRANS)
def test_every_lie_is_noticed_beside_its_honest_twin(ctx, gran):
    """The lies interleaved with their honest twins in one call: one fallback per lying frame, none more; every frame of
    the call right, the honest neighbours included; the lies that are no Snappy return the checkers' code."""
    t0 = time.time()
    lies = [_lie(lie) for lie in X.lies(gran)]
    twins = [_build("honest twin", [X.honest_twin(gran)], 13, gran, w) for w in (0, X.WINDOW_BYTE)]
    assert _run(ctx, twins) == 0
    batch = [x for i, lie in enumerate(lies) for x in (lie, twins[i % 2])]
    assert _run(ctx, batch) == len(lies)
    for lie in lies[:2] + lies[-3:]:
        assert _run(ctx, [twins[0], lie, twins[1]]) == 1, lie.label
    print("GRAN %d: %d lying frames (%d no Snappy) beside %d honest fragments, %.2f s" % (
        gran, len(lies), sum(1 for b in lies if b.code), _count(twins), time.time() - t0))


def test_all_six_kinds_in_one_launch(ctx):
    """Granularity 0, 1 and 2, each with and without a window promise, in one call at log2 13: six kernels, no fallback"""
    t0 = time.time()
    built = []
    for gran in GRANS:
        for window256 in (0, X.WINDOW_BYTE):
            built += _family(gran, ("passes", "chains", "window"), 13, window256)
    assert len(built) == 18 and _run(ctx, built) == 0
    assert _run(ctx, built[::-1]) == 0
    print("six kinds: %d fragments in %d frames, twice, %.2f s" % (_count(built), len(built), time.time() - t0))


@pytest.mark.parametrize("gran", GRANS)
def test_every_source_phase(ctx, gran):
    """The forms and staging families from device memory at sixteen consecutive byte addresses: a fragment's address
    modulo 16 is its buffer's plus its place in the frame, so every fragment meets every phase -- the one the staging
    family is built for among them.  The phases are read off the device pointers the library is handed.  Plain and
    windowed; then both once from host memory."""
    t0 = time.time()
    offs = list(range(16))
    for window256 in (0, X.WINDOW_BYTE):
        built = _family(gran, ("forms", "staging"), 13, window256)
        met = collections.defaultdict(set)
        batch = [b for b in built for _ in offs]
        assert _run(ctx, batch, src_off=offs * len(built), met=met) == 0
        assert len(met) == _count(built) and all(phases == set(range(16)) for phases in met.values())
        assert _run(ctx, built, where="host") == 0
    print("GRAN %d: %d fragments at 16 source phases, plain and windowed, %.2f s" % (gran, _count(built), time.time() - t0))


@pytest.mark.parametrize("gran", GRANS)
def test_output_addresses_off_the_sixteen_byte_line(ctx, gran):
    """Outputs at 16-byte alignment plus 0, 1, 2 and 3: the ring leaves through a head of single bytes"""
    t0 = time.time()
    calls = collections.defaultdict(list)
    for fam in ("passes", "chains", "window", "ends", "rings"):
        for fr in X.family_frames(fam, gran):
            calls[fr.frag_log2].append(_build(fr.label, fr.chunks, fr.frag_log2, gran))
            if fr.frag_log2 == 13 and fr.window_ok:
                calls[13].append(_build(fr.label, fr.chunks, 13, gran, X.WINDOW_BYTE))
    assert sorted(calls) == list(X.FRAG_LOG2S)
    for frag_log2, frames in sorted(calls.items()):
        for off in (0, 1, 2, 3):
            assert _run(ctx, frames, dst_off=off) == 0, (frag_log2, off)
        assert _run(ctx, frames, dst_off=[i % 4 for i in range(len(frames))], src_off=[(5 * i) % 16 for i in range(len(frames))]) == 0
    print("GRAN %d: %d fragments at four output offsets, %.2f s" % (gran, sum(_count(f) for f in calls.values()), time.time() - t0))


@pytest.mark.parametrize("gran", GRANS)
def test_two_fragment_sizes_in_one_call(ctx, gran):
    """Frames of log2 10 and of log2 13 together: a launch takes one size, the frames of the other go through
    whole-stream units (hap_batch.c, "one fragment size per launch").  Bytes right, no frame decoded a second time."""
    t0 = time.time()
    small = _family(gran, ("ends", "rings"), 10)
    large = _family(gran, ("chains", "window"), 13) + _family(gran, ("window",), 13, X.WINDOW_BYTE)
    assert len(small) >= 3 and len(large) >= 3
    assert _run(ctx, small + large) == 0
    assert _run(ctx, large + small) == 0
    mixed = [x for pair in zip(small, large) for x in pair]
    assert _run(ctx, mixed, src_off=[i % 16 for i in range(len(mixed))]) == 0
    print("GRAN %d: %d fragments of two sizes in one call, %.2f s" % (gran, _count(small + large), time.time() - t0))


@pytest.mark.parametrize("gran", GRANS)
def test_a_version_three_table_gives_its_sizes_and_nothing_else(ctx, gran):
    """[3][13][g][w], 4 + 96 bytes a fragment, on the same fragments: the sizes are used, one wavefront per fragment
    through these kernels; the 96-byte group tables hold 0xFF throughout and nobody reads them.  A lie under such a
    table is noticed as under version 1."""
    t0 = time.time()
    built = _family(gran, ("passes", "chains", "window", "staging"), 13, 0, 3) + _family(gran, ("window", "forms"), 13, X.WINDOW_BYTE, 3)
    assert _run(ctx, built) == 0
    lie = X.lies(gran)[0]
    b = X.frame_of_fragments([lie.chunk], 13, X.GRAN_LOG2[gran], lie.window256, version=3)
    lying = Built(lie.name + ", version 3", b.frame, b.want, 0, 16384, b.fragments, b.starts)
    assert lie.valid and _run(ctx, built[:1] + [lying] + built[1:2]) == 1
    print("GRAN %d: %d fragments under a version-3 table, %.2f s" % (gran, _count(built), time.time() - t0))

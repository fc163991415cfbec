"""The hand-built field streams of tests/_field_streams.py through hap_amd/csrc/snappy_decode_fields.hip, for each of
its four block layouts, on two roads:

  table road   the frame carries the version-4 fragment table (section 0x46) and decodes with flags 0;
  guess road   the same fragments as chunks of their own without a table: guess_group_tables_kernel writes the tables
               (DECODE_GUESS_FIELDS), with DECODE_NO_FIELD_GUESS and with no flag as the controls.  Layouts 4, 2, 6.

The expected bytes are the ones the fragment builders recorded (tests/test_field_streams.py holds them to the plain
decoder and to the checker libraries); every output lies in the middle of sentinel-filled memory.

On the table road table_fallbacks() must stand still for the honest families -- the field kernel, not a second pass,
made the bytes -- and every honest batch is followed by its lie twins, which must each raise it by one: the table is
looked at.  Bytes alone are asserted
  * on the guess road: nothing counts the units the pre-pass converts, and a unit it leaves alone is decoded by the
    generic kernel to the same bytes;
  * for the room family: it sits on a limit of the kernel (its input-room check) that the public header does not state,
    so a frame of it may or may not be decoded a second time.
A fragment whose records go to memory and, at an output address that is no multiple of four, no longer fit its own
output range is declined by the kernel as well (all-copy fragments of one element per field): which frames those are
follows from the kernel's text (_field_streams.records_fit), and they are expected to fall back exactly there.

What no stream can reach: the sixth round of pointer doubling.  After the four DPP hops a pending link spans three
lanes or more unless its lane is the first or second of a row of 16 (hops 1 and 2 replace every shorter link they may
take, hops 4 and 8 only lengthen), so a chain of one step holds at most 6 + 57 / 3 = 25 links and five rounds resolve
it.  The deepest chains here (one field copied from three blocks back: 21 links) need all five."""
import functools
import time

import numpy as np
import pytest

import _data as D
import _field_streams as F
import _libs as L
import _snappy_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x5A
GAP = 32                                  # sentinel bytes in front of and behind every output
GUESS_MAX_CHUNK = 64 * 130 + 64 + 5       # hap_batch.c: a longer chunk keeps its frame off the guess road
LAYOUT_FORMATS = [(layout, fmt) for layout, lay in F.LAYOUTS.items() for fmt in lay.formats]
IDS = ["layout %d, format %#x" % lf for lf in LAYOUT_FORMATS]


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


class Built:
    """A frame, what it decodes to, and what it is"""

    def __init__(self, label, frame, want, fmt, fragments):
        self.label, self.frame, self.want, self.fmt, self.fragments = label, frame, want, fmt, fragments


@functools.lru_cache(None)
def _family_frames(layout, fmt, families):
    """A frame with the table per family and chunk shape (one fragment a chunk; the case third of three)"""
    built = []
    for fam in families:
        for per in (1, 3):
            chunks = [F.chunk_of(c) for c in F.family(fam, layout) if c.fragments == per]
            if chunks:
                frame, want = F.frame_of_fragments(chunks, layout, fmt)
                built.append(Built("%s, layout %d, %d to a chunk" % (fam, layout, per), frame, want, fmt, [f for c in chunks for f in c]))
    return built


STRICT = tuple(name for name in F.FAMILIES if name not in F.BYTES_ONLY)


@functools.lru_cache(None)
def _lie_frames(layout, fmt):
    built = []
    for lie in F.lies(layout):
        frame, want = F.frame_of_fragments([lie.chunk], layout, fmt, True, lie.tables)
        built.append(Built(lie.name, frame, want, fmt, lie.chunk))
    return built


@functools.lru_cache(None)
def _tableless_frame(layout, fmt, families=tuple(F.FAMILIES)):
    """Every fragment of the families a chunk of its own, no table: what ENCODE_FINE_CHUNKS writes"""
    frags = [f for fam in families for c in F.family(fam, layout) for f in F.chunk_of(c)]
    frags = [f for f in frags if len(S.varint(f.made)) + f.total <= GUESS_MAX_CHUNK]
    assert len(frags) > 1
    frame, want = F.frame_of_fragments([[f] for f in frags], layout, fmt, table=False)
    return Built("no table, %s, layout %d" % (families[0] if len(families) == 1 else "%d families" % len(families), layout), frame, want, fmt, frags)


def _per_frame(value, n):
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def _run(ctx, built, flags=0, where="device", src_off=0, dst_off=0):
    """One decode_frames call: every frame from its own buffer (at src_off bytes into it), every output in the middle of
    sentinel-filled memory, 16-byte aligned plus dst_off.  Asserts results, formats, bytes and sentinels; returns the
    rise of table_fallbacks()."""
    n = len(built)
    src_off, dst_off = _per_frame(src_off, n), _per_frame(dst_off, n)
    starts, at = [], 0
    for b, d in zip(built, dst_off):
        starts.append(at + GAP + d)
        at = (at + GAP + d + len(b.want) + GAP + 15) & ~15
    expect = np.full(at, SENTINEL, dtype=np.uint8)
    for b, s in zip(built, starts):
        expect[s: s + len(b.want)] = np.frombuffer(b.want, dtype=np.uint8)
    if where == "device":
        srcs = [torch.from_numpy(np.frombuffer(bytes(o) + b.frame, dtype=np.uint8).copy()).cuda()[o:] for b, o in zip(built, src_off)]
        backing = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    else:
        srcs = [b.frame for b in built]
        backing = np.full(at, SENTINEL, dtype=np.uint8)
    outs = [backing[s: s + len(b.want)] for b, s in zip(built, starts)]
    n0 = ctx.table_fallbacks()
    r, used, fmts, res = ctx.decode_frames(srcs, [len(b.frame) for b in built], 0, outs, flags)
    rise = ctx.table_fallbacks() - n0
    got = backing.cpu().numpy() if where == "device" else backing
    assert r == 0 and res == [0] * n, (r, [(b.label, c) for b, c in zip(built, res) if c])
    assert used == [len(b.want) for b in built] and fmts == [b.fmt for b in built]
    if not np.array_equal(got, expect):
        wrong = []
        for b, s in zip(built, starts):
            lo, hi = s - GAP, s + len(b.want) + GAP
            bad = np.flatnonzero(got[lo:hi] != expect[lo:hi])
            if len(bad):
                wrong.append("%s: %s" % (b.label, _where(b, int(bad[0]) - GAP, got[lo + int(bad[0])], expect[lo + int(bad[0])])))
        pytest.fail("%d frames wrong; %s" % (len(wrong), "; ".join(wrong[:16])))
    return rise


def _where(b, at, got, want):
    if at < 0 or at >= len(b.want):
        return "sentinel byte %d overwritten with %d" % (at, got)
    p = 0
    for i, f in enumerate(b.fragments):
        if at < p + f.made:
            names = [c.name for fam in F.FAMILIES for c in F.family(fam, f.layout) if c.frag is f]
            return "byte %d of fragment %d (%s): %d for %d" % (at - p, i, ", ".join(names) or "filler", got, want)
        p += f.made
    return "byte %d" % at


@pytest.mark.parametrize("layout,fmt", LAYOUT_FORMATS, ids=IDS)
def test_the_table_road_decodes_every_family_and_notices_every_lie(ctx, hap, layout, fmt):
    """Honest families: right bytes, sentinels untouched, no frame decoded a second time.  The room family: bytes.
    Then the lie twins beside the honest frames, in one call: one fallback per lying frame, none more, and every frame
    of the call -- the honest neighbours included -- right."""
    t0 = time.time()
    honest = _family_frames(layout, fmt, STRICT)
    assert _run(ctx, honest) == 0
    room = _family_frames(layout, fmt, F.BYTES_ONLY)
    assert 0 <= _run(ctx, room) <= len(room)
    lies = _lie_frames(layout, fmt)
    batch = [x for pair in zip(lies, honest) for x in pair] + lies[len(honest):] + honest[len(lies):]
    assert _run(ctx, batch) == len(lies)
    print("layout %d, format %#x: %d honest fragments in %d frames, %d lying frames, %.2f s" % (
        layout, fmt, sum(len(b.fragments) for b in honest + room), len(honest + room), len(lies), time.time() - t0))


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_one_lying_fragment_of_eight_sends_its_frame_round_once(ctx, hap, layout):
    fmt = F.LAYOUTS[layout].formats[-1]
    fillers = [F.mixed(layout, 700 + i, F.FRAG, 150 + 111 * i) for i in range(8)]
    stream_lie, = [lie for lie in F.lies(layout) if lie.name.endswith("offset not a whole block")]
    table_lie, = [lie for lie in F.lies(layout) if lie.name.endswith("sums that do not add up")]
    built = []
    for lie in (stream_lie, table_lie):
        chunk = fillers[:5] + [lie.chunk[0]] + fillers[6:]
        frame, want = F.frame_of_fragments([chunk], layout, fmt, True, {5: lie.tables[0]} if lie.tables else None)
        built.append(Built(lie.name + ", fragment 5 of 8", frame, want, fmt, chunk))
    frame, want = F.frame_of_fragments([fillers], layout, fmt)
    built.append(Built("eight honest fragments", frame, want, fmt, fillers))
    assert _run(ctx, built[2:]) == 0
    assert _run(ctx, built[:1]) == 1
    assert _run(ctx, built) == 2


@pytest.mark.parametrize("layout,fmt", [lf for lf in LAYOUT_FORMATS if lf[0] in F.GUESS_LAYOUTS],
                         ids=[i for lf, i in zip(LAYOUT_FORMATS, IDS) if lf[0] in F.GUESS_LAYOUTS])
def test_the_guess_road_decodes_every_family(ctx, hap, layout, fmt):
    """Bytes and sentinels: nothing counts the units guess_group_tables_kernel converts.  What can be said beyond them is
    that no frame of honest fragments is decoded a second time -- a fragment the pre-pass hands to the field kernel is
    one the table road takes as well, and one it leaves alone is decoded by the generic kernel in the same pass.  The
    room family has a frame of its own (a fragment of it that the field kernel declines sends its whole frame round), and
    so have the stream lies, which the pre-pass must leave to the generic kernel."""
    t0 = time.time()
    honest = _tableless_frame(layout, fmt, STRICT)
    room = _tableless_frame(layout, fmt, F.BYTES_ONLY)
    liars = [lie.chunk[0] for lie in F.lies(layout) if lie.promise and len(lie.chunk) == 1]
    frame, want = F.frame_of_fragments([[f] for f in liars], layout, fmt, table=False)
    lying = Built("no table, stream lies, layout %d" % layout, frame, want, fmt, liars)
    for flags in (hap.DECODE_GUESS_FIELDS, hap.DECODE_NO_FIELD_GUESS, 0):
        assert _run(ctx, [honest], flags) == 0
        _run(ctx, [lying, honest, room], flags)
    _run(ctx, [honest, lying, room], hap.DECODE_GUESS_FIELDS, where="host")
    print("layout %d, format %#x: %d fragments without a table, %.2f s" % (layout, fmt, len(honest.fragments + room.fragments), time.time() - t0))


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_every_source_alignment(ctx, hap, layout):
    """The alignment family, the records ladder beside it, from device memory at sixteen consecutive byte addresses: a
    fragment's address modulo 16 is the frame's plus its place in the frame, so every residue comes up for each.  Every
    frame ends with its last fragment, and the frame with its buffer.  Then the same without a table."""
    fmt = F.LAYOUTS[layout].formats[0]
    ladder = tuple(c for c in F.family("records", layout) if c.name.split(": ")[1].startswith("records "))
    chunks = [F.chunk_of(F.family("alignment", layout)[0])] + [F.chunk_of(c) for c in ladder]
    frame, want = F.frame_of_fragments(chunks, layout, fmt)
    one = Built("alignment and the records ladder, layout %d" % layout, frame, want, fmt, [f for c in chunks for f in c])
    chunk = F.chunk_of(F.family("alignment", layout)[1])
    frame, want = F.frame_of_fragments([chunk], layout, fmt)
    three = Built("alignment, three to a chunk, layout %d" % layout, frame, want, fmt, chunk)
    offs = list(F.SOURCE_ALIGNMENTS)
    assert offs == list(range(16))
    assert _run(ctx, [one] * 16 + [three] * 16, src_off=offs + offs) == 0
    if layout in F.GUESS_LAYOUTS:
        frame, want = F.frame_of_fragments([[f] for f in one.fragments + three.fragments], layout, fmt, table=False)
        bare = Built("alignment without a table, layout %d" % layout, frame, want, fmt, one.fragments + three.fragments)
        assert _run(ctx, [bare] * 16, hap.DECODE_GUESS_FIELDS, src_off=offs) == 0


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_output_addresses_that_are_no_multiple_of_the_block(ctx, hap, layout):
    """Outputs at 0, 1, 4 and 8 bytes past a 16-byte boundary: the bytes-at-a-time stores, also for fragments whose
    records are in memory (the upper rungs of the records ladder).  The all-copy fragments of one element per field keep
    their records in memory too, and those fill the whole output range: at an address that is no multiple of four the
    kernel declines them (records_fit), and exactly their frames are decoded a second time."""
    fmt = F.LAYOUTS[layout].formats[-1]
    records = F.family("records", layout)
    groups = [("records ladder", [[c.frag] for c in records[:-2]]), ("all copies", [[c.frag] for c in records[-2:]]),
              ("alignment", [F.chunk_of(F.family("alignment", layout)[0])]),
              ("short fragments", [F.chunk_of(c) for c in F.family("short fragments", layout) if c.fragments == 3])]
    built = []
    for label, chunks in groups:
        frame, want = F.frame_of_fragments(chunks, layout, fmt)
        built.append(Built("%s, layout %d" % (label, layout), frame, want, fmt, [f for c in chunks for f in c]))
    assert any(not F.records_in_lds(f, s) for f in built[0].fragments for s in F.SOURCE_ALIGNMENTS)
    assert list(F.OUTPUT_OFFSETS) == [0, 1, 4, 8]
    for off in F.OUTPUT_OFFSETS:
        declined = 0
        for b in built:
            fits = [{F.records_fit(f, s, off) for s in F.SOURCE_ALIGNMENTS} for f in b.fragments]
            assert all(len(v) == 1 for v in fits), b.label              # (no case hangs on the source address)
            declined += any(v == {False} for v in fits)
        assert declined == (1 if off % 4 else 0)
        assert _run(ctx, built, dst_off=off) == declined, off


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_frames_in_host_memory(ctx, hap, layout):
    fmt = F.LAYOUTS[layout].formats[0]
    assert _run(ctx, _family_frames(layout, fmt, STRICT), where="host") == 0


def test_all_layouts_and_a_two_texture_frame_in_one_launch(ctx, hap):
    """One call with frames of all four layouts and a hand-made Hap Q Alpha frame (layouts 4 and 6 in one frame); again
    with DECODE_IGNORE_HALF_TILES (the generic fragment kernels on the table's sizes)."""
    singles = []
    for layout, lay in F.LAYOUTS.items():
        for fmt in lay.formats:
            singles += _family_frames(layout, fmt, ("counts", "forms", "chains, rows"))
    two, wants = F.frame_of_two_textures([F.chunk_of(c) for c in F.family("element splits", 4)],
                                         [F.chunk_of(c) for c in F.family("element splits", 6)])
    missing = L.oracle_api().decode(singles[0].frame, 1, 8192)[0]
    assert missing != 0
    frames = [b.frame for b in singles] + [two]
    want = [w for b in singles for w in (b.want, None)] + wants
    fmts = [v for b in singles for v in (b.fmt, None)] + [L.FMT_YCOCG, L.FMT_RGTC1]
    for flags in (0, hap.DECODE_IGNORE_HALF_TILES):
        # (an entry for the second texture of a one-texture frame: sixteen bytes nobody may write)
        backing = [torch.full(((16 if w is None else len(w)) + 2 * GAP,), SENTINEL, dtype=torch.uint8, device="cuda") for w in want]
        srcs = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in frames]
        torch.cuda.synchronize()
        n0 = ctx.table_fallbacks()
        r, used, got_fmts, res = ctx.decode_frame_textures(srcs, [len(f) for f in frames], 2,
                                                           [b[GAP: len(b) - GAP] for b in backing], flags)
        assert r == missing and res == [0 if w is not None else missing for w in want], (r, res)
        assert ctx.table_fallbacks() == n0
        for i, (w, b) in enumerate(zip(want, backing)):
            whole = b.cpu().numpy().tobytes()
            if w is not None:
                assert used[i] == len(w) and got_fmts[i] == fmts[i], i
                assert whole == bytes([SENTINEL]) * GAP + w + bytes([SENTINEL]) * GAP, (i, flags)
            else:
                assert whole == bytes([SENTINEL]) * (16 + 2 * GAP), i


def test_the_library_writes_the_header_the_builder_writes(ctx, hap):
    """[4][13][granularity | layout << 4][0] of section 0x46, read off a frame the library encodes for each format"""
    for layout, lay in F.LAYOUTS.items():
        for fmt in lay.formats:
            n = (2 << 20) + 8192 if fmt == L.FMT_RGTC1 else 4 * 8192               # (RGTC1 planes take layout 6 from 2 MiB on)
            tex = D.stream_bytes(n, "runs")
            out = np.zeros(hap.HapMaxEncodedLength([n], [fmt], [1]) + 65536, dtype=np.uint8)
            flags = hap.ENCODE_FRAGMENT_INDEX | (hap.ENCODE_COARSE_MATCHES if layout == 8 else 0)
            r, used, res = ctx.encode_frames([[tex]], [fmt], [1], [1], [out], flags=flags)
            assert r == 0 and res == [0]
            head = out[: min(used[0], 64)].tobytes()
            at = head.find(bytes([0x46, 4, 13]))
            assert at > 0, (layout, fmt)
            assert head[at + 3] == lay.gran | layout << 4 and head[at + 4] == 0, (layout, fmt, head[at + 3])

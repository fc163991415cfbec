"""The hand-built field streams of tests/_field_streams.py, without a GPU: every honest case keeps the promises of
include/hap_gpu.h (conforms), decodes with the plain Snappy decoder and -- in its frame -- with the checker libraries to
the bytes its builder recorded; every lie is still Snappy to the checkers and breaks exactly the promise it is named
after; and the families hold what they are meant to hold, read back from the built bytes.

Two things differ from a naive reading of the grammar, both consequences of the promises themselves:
  * an element that starts and ends on field boundaries has an even length (a multiple of four for the 4 + 4 layouts;
    2, 6 or 0 modulo 8 for the 2 + 6 layout): "every literal length" means every length the layout's boundaries allow;
  * a copy whose offset is the fragment's length less one block lies in the fragment's last block.

No golden frame carries a version-4 table (tests/golden holds none written with the fragment table), so group_table()
is held to the table the scalar definition of the library's own compressor writes (oracle/field_stream_oracle.c)."""
import ctypes as C

import numpy as np
import pytest

import _field_streams as F
import _libs as L
import _snappy_streams as S

LAYOUTS = list(F.LAYOUTS)
CHECKERS = [("oracle", L.oracle_api())] + ([("reference", L.ref_api())] if L.ref_api() is not None else [])


def _honest(layout):
    return [(name, case) for name in F.FAMILIES for case in F.family(name, layout)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_honest_case_keeps_the_promises_and_decodes_to_its_recorded_bytes(layout):
    cases = _honest(layout)
    assert len({case.name for _f, case in cases}) == len(cases)
    for fam, case in cases:
        f = case.frag
        assert F.conforms(f.stream(), layout, f.made) is None, case.name
        assert 1 <= f.made <= F.FRAG and f.total == len(f.stream()) <= F.MAX_COMPRESSED, case.name
        assert S.decode(S.varint(f.made) + f.stream()) == bytes(f.out), case.name
        assert F.unpack_groups(F.group_table(f.parts))[2] == len(f.parts)
        # what the kernel declines without a promise being broken happens in the room family alone
        if fam not in F.BYTES_ONLY:
            assert all(F.room_ok(f, s) for s in F.SOURCE_ALIGNMENTS), case.name
            assert all(F.records_fit(f, s, 0) for s in F.SOURCE_ALIGNMENTS), case.name


@pytest.mark.parametrize("table", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_of_honest_cases_decode_with_the_checkers(layout, table):
    for fmt in F.LAYOUTS[layout].formats:
        for fam in F.FAMILIES:
            for fragments in (1, 3):
                chunks = [F.chunk_of(c) for c in F.family(fam, layout) if c.fragments == fragments]
                if not chunks:
                    continue
                frame, want = F.frame_of_fragments(chunks, layout, fmt, table)
                for name, api in CHECKERS:
                    assert api.decode(frame, 0, len(want)) == (0, want, fmt), (name, fam, fragments)
                    assert api.chunk_count(frame, 0) == (0, len(chunks) * (1 if table else fragments)), fam


def test_the_two_texture_frame_decodes_with_the_checkers():
    for table in (True, False):
        frame, want = F.frame_of_two_textures([F.chunk_of(c) for c in F.family("counts", 4)],
                                              [F.chunk_of(c) for c in F.family("counts", 6)], table)
        for name, api in CHECKERS:
            assert api.texture_count(frame) == (0, 2), name
            assert api.decode(frame, 0, len(want[0])) == (0, want[0], L.FMT_YCOCG), name
            assert api.decode(frame, 1, len(want[1])) == (0, want[1], L.FMT_RGTC1), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_lie_is_snappy_to_the_checkers_and_breaks_one_promise(layout):
    lay = F.LAYOUTS[layout]
    lies = F.lies(layout)
    honest = F.honest_twin(layout)
    assert F.conforms(honest.stream(), layout, F.FRAG) is None and all(F.room_ok(honest, s) for s in F.SOURCE_ALIGNMENTS)
    stream_lies = {"offset not a whole block", "element across a half-tile", "copy-4", "literal with a two-byte length",
                   "copy from one block before the fragment"}
    stream_lies |= {"start on an even byte that is no field start", "start on an odd byte"} if layout in (4, 6) else \
        {"start off a multiple of four"}
    table_lies = {"table, N -1", "table, N +1", "table, N +64", "table, a boundary moved between two groups' compressed bytes",
                  "table, a boundary moved between two groups' output bytes", "table, sums that do not add up", "table, all zero"}
    assert {lie.name.split(": ", 1)[1] for lie in lies} == stream_lies | table_lies
    for lie in lies:
        frame, want = F.frame_of_fragments([lie.chunk], layout, lay.formats[0], True, lie.tables)
        assert len(want) == F.FRAG * len(lie.chunk)
        for name, api in CHECKERS:
            assert api.decode(frame, 0, len(want)) == (0, want, lay.formats[0]), (lie.name, name)
        assert S.decode(S.varint(len(want)) + b"".join(f.stream() for f in lie.chunk)) == want, lie.name
        f = lie.chunk[-1]
        if lie.promise is None:
            # a table lie: the stream is honest, the table is not the stream's
            assert F.conforms(f.stream(), layout, f.made) is None and len(lie.chunk) == 1, lie.name
            assert lie.tables[0] != F.group_table(f.parts) and len(lie.tables[0]) == F.GT, lie.name
        else:
            assert lie.promise in F.PROMISES and F.broken(f.stream(), layout, f.made) == [lie.promise], lie.name
            assert not lie.tables and all(F.conforms(g.stream(), layout, g.made) is None for g in lie.chunk[:-1]), lie.name
            # a twin: the honest fragment's elements but for those of one half-tile (two where an element lies across)
            same = sum(1 for x, y in zip(f.parts, honest.parts) if x == y) + sum(1 for x, y in zip(f.parts[::-1], honest.parts[::-1]) if x == y)
            assert f.parts != honest.parts and same >= len(honest.parts) - 8, lie.name
    # what the lies are about, said with the elements
    by_name = {lie.name.split(": ", 1)[1]: lie for lie in lies}
    els = [el for _p, el in F._walk(by_name["copy from one block before the fragment"].chunk[1])]
    made = 0
    reach = []
    for el in els:
        if el.form.startswith("copy") and el.off > made:
            reach.append(el.off - made)
        made += el.n
    assert reach == [lay.block]
    starts = lambda lie: [p for p, _el in F._walk(lie.chunk[0])]                        # noqa: E731
    if layout in (4, 6):
        assert any(p % 2 == 0 and not F.on_field(layout, p) for p in starts(by_name["start on an even byte that is no field start"]))
        assert not any(p % 2 for p in starts(by_name["start on an even byte that is no field start"]))
        assert any(p % 2 for p in starts(by_name["start on an odd byte"]))
    else:
        assert any(p % 4 for p in starts(by_name["start off a multiple of four"]))


def _ofs_fragment(data, layout):
    o = L.oracle_lib()
    o.ofs_compress_fragment.restype = C.c_uint
    out = (C.c_ubyte * (8192 + 512))()
    table = (C.c_ubyte * F.GT)()
    n = o.ofs_compress_fragment(bytes(data), C.c_uint(len(data)), C.c_uint(layout), C.c_uint(0), out, table)
    return bytes(out[:n]), bytes(table)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_group_table_rebuilds_the_tables_of_the_compressors_scalar_definition(layout):
    """tests/golden has no frame with a version-4 table to parse.  The scalar definition of the library's own
    compressor writes the table beside the elements: group_table() of the parsed elements is that table, byte for byte;
    and what that compressor writes keeps the promises as conforms() states them."""
    for seed, n in ((1, 8192), (2, 8192), (3, 8192 - 3 * F.LAYOUTS[layout].block), (4, 640)):
        frag = F.family("element splits", layout)[(7 * seed) % F.SPLITS].frag
        data = (bytes(frag.out) * (8192 // max(1, frag.made) + 1))[:n] if seed != 2 else F.mixed(layout, seed, n).out
        stream, table = _ofs_fragment(data, layout)
        assert S.decode(S.varint(n) + stream) == bytes(data)
        parts = [stream[el.pos - len(S.varint(n)): el.pos - len(S.varint(n)) + el.hdr + (el.n if el.form.startswith("lit") else 0)]
                 for el in S.elements(S.varint(n) + stream)]
        assert b"".join(parts) == stream
        assert F.group_table(parts) == table, (layout, seed)
        assert F.conforms(stream, layout, n) is None


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_families_hold_what_they_are_meant_to_hold(layout):
    lay = F.LAYOUTS[layout]
    d = F.describe(layout)
    step = F.step_bytes(layout)
    assert list(F.FAMILIES) == ["chains", "chains, mixed", "chains, long", "chains, rows", "chains, ring", "forms", "element splits",
                                "counts", "short fragments", "records", "room", "alignment"]
    # chains: every distance 1..63, once for each field
    assert dict(d["chain distances"]) == {k: set(range(1, 64)) for k in range(len(lay.fields))}
    assert d["chains, mixed"] == sorted((3, 17, 1, 40)[: len(lay.fields)])
    assert d["chains, long"] == [1] and d["chains, rows"] == [1, 2, 4, 8]
    assert set(d["chains, ring"]) >= {64, 65, 127, 128}
    # ... the long chain is 63 links long both ways; the row chains cross lanes 15 -> 16, 31 -> 32 and 47 -> 48
    for case in F.family("chains, long", layout):
        first = bytes(case.frag.out[: lay.block])
        assert bytes(case.frag.out) == first * 128 and len(set(first)) > 4
    for case, dist in zip(F.family("chains, rows", layout), (1, 2, 4, 8)):
        copied = {p // lay.block for p, el in F._walk(case.frag) if el.form.startswith("copy")}
        assert all(b + j in copied for b in (16, 32, 48, 64 + 16, 64 + 32, 64 + 48) for j in range(dist)), case.name   # sources: the row below
        assert 0 not in copied and min(copied) == 4 + dist                   # the chain's root is not the step's first block
    own = [(p, el.off) for p, el in F._walk(F.family("chains, ring", layout)[-1].frag) if el.form.startswith("copy")]
    assert own == [(2 * step + 32, 2 * step + 32), (F.FRAG - lay.block, F.FRAG - lay.block)]
    # forms: every literal length the boundaries allow, 1..60 in the tag and 1..128 with a length byte, at the start,
    # in the middle and at the end of a half-tile wherever it can lie there
    spans = F.literal_spans(layout)
    allowed = {n for n in range(1, 129) if any(F.on_field(layout, s) and F.on_field(layout, s + n) for s in range(lay.block))}
    assert set(spans) == allowed and {4: 64, 2: 32, 6: 48, 8: 32}[layout] == len(allowed)
    assert d["literals"]["lit1"] == allowed and d["literals"]["lit0"] >= {n for n in allowed if n <= 60}
    assert set(d["literals"]) == {"lit0", "lit1"}
    for n, starts in spans.items():
        places = {"start"} if 0 in starts else set()
        places |= {"end"} if F.HALF - n in starts else set()
        places |= {"middle"} if any(0 < s < F.HALF - n for s in starts) else set()
        assert d["literal places"][("lit1", n)] >= places, n
        if n <= 60:
            assert d["literal places"][("lit0", n)] >= places, n
    top1 = 2047 // lay.block * lay.block
    lens1 = [n for n in range(4, 12) if n in allowed]
    lens2 = [n for n in (1, 2, 4, 6, 64) if n in allowed]
    assert lens1 and 64 in lens2 and len(lens2) >= 2
    assert d["copy1"] >= {(n, off) for n in lens1 for off in (lay.block, top1)}
    assert d["copy2"] >= {(n, off) for n in lens2 for off in (lay.block, 2048)}
    assert d["copy2"] >= {(fn, F.FRAG - lay.block) for _fp, fn in lay.fields}
    ends = [p + el.n for p, el in F._walk(F.family("forms", layout)[-1].frag) if el.form == "copy2" and el.n == 64]
    assert any(e % F.HALF == 0 for e in ends) and any(e % F.HALF == 64 for e in ends)
    # counts, short fragments, element splits
    assert d["counts"] == [1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 1024, 2048]
    assert F.conforms(F.family("counts", layout)[-1].frag.stream() + S.copy2(lay.fields[0][1], lay.block), layout, F.FRAG + lay.fields[0][1]) \
        == "element count"                                                  # (there is no larger N)
    assert any(0 in F.unpack_groups(F.group_table(c.frag.parts))[0] for c in F.family("counts", layout))      # empty groups
    assert d["short lengths"] == sorted({lay.block, 2 * lay.block, 128 - lay.block, 128, 128 + lay.block, step - lay.block,
                                         step + lay.block, 8192 - lay.block})
    assert d["short chunks"] == [1, 3] and len(F.family("short fragments", layout)) == 16
    assert d["splits"] == 32
    sizes = sorted(len(c.frag.parts) / (c.frag.made // 4) for c in F.family("element splits", layout))
    assert sizes[0] < 0.15 and sizes[-1] == 1.0                             # from a handful to one element per field
    # records: a ladder at one compressed size, on both sides of the point where the records leave LDS, for every
    # source alignment (kBufBytes: SDF_BUF_BYTES, hap_amd/csrc/snappy_decode_fields.hip:66 and :74)
    ladder = [c for c in F.family("records", layout) if c.name.split(": ")[1].startswith("records ")]
    assert {c.frag.total for c in ladder} == {F.RECORDS_TOTAL} and [len(c.frag.parts) for c in ladder] == list(F.RECORDS_LADDER)
    assert F.K_BUF_BYTES == 9344 + 32
    for s in F.SOURCE_ALIGNMENTS:
        inside = [F.records_in_lds(c.frag, s) for c in ladder]
        assert inside[0] and not inside[-1] and inside == sorted(inside, reverse=True), s
        assert inside.count(True) >= 2 and inside.count(False) >= 2
    for c in F.family("records", layout)[-2:]:
        assert all(e[0] & 3 for e in c.frag.parts[len(lay.fields) * 5:]) and len(c.frag.parts) == F.FRAG // 4
        assert not any(F.records_in_lds(c.frag, s) for s in F.SOURCE_ALIGNMENTS)
    # room: both sides of the limit
    sides = {F.room_ok(c.frag, 0) for c in F.family("room", layout)}
    assert sides == {True, False}
    # alignment
    assert d["source alignments"] == list(range(16)) and d["output offsets"] == [0, 1, 4, 8]
    sizes = [f.total for f in F.chunk_of(F.family("alignment", layout)[1])]
    assert len({s % 16 for s in sizes[:2]}) == 2 and len(sizes) == 3


def test_the_frame_rules_are_kept():
    """The header of section 0x46 and the chunk rule, on one frame per layout"""
    for layout, lay in F.LAYOUTS.items():
        chunks = [F.chunk_of(c) for c in F.family("short fragments", layout) if c.fragments == 3]
        frame, want = F.frame_of_fragments(chunks, layout, lay.formats[0])
        at = frame.find(bytes([0x46, 4, 13, lay.gran | layout << 4, 0]))
        assert at > 0 and int.from_bytes(frame[at - 3: at], "little") == 4 + (4 + F.GT) * 3 * len(chunks)
        sizes = [int.from_bytes(frame[at + 5 + 4 * i: at + 9 + 4 * i], "little") for i in range(3 * len(chunks))]
        assert sizes == [f.total for c in chunks for f in c]

"""The hand-built Snappy streams of tests/_snappy_streams.py, without a GPU: the plain decoder that is the reference
of tests/test_foreign_streams_gpu.py gives what libsnappy and the oracle give on every one of them (so every
non-canonical form in them is Snappy to the library every Hap client uses), and the sweeps hold what they claim to
hold -- computed from the built bytes, not from the generators' intentions."""
import collections

import pytest

import _data as D
import _libs as L
import _snappy_streams as S

K = S.K


def _all_cases():
    return [(sweep, case) for sweep, make in S.SWEEPS.items() for case in make()]


def _forms_seen(stream):
    return collections.Counter((el.form, el.n) for el in S.elements(stream))


@pytest.mark.parametrize("sweep", list(S.SWEEPS))
def test_plain_decoder_gives_what_libsnappy_and_the_oracle_give(sweep):
    cases = S.SWEEPS[sweep]()
    assert cases and len({name for name, _s, _e in cases}) == len(cases)
    for name, stream, expected in cases:
        want = S.decoded(stream)
        assert len(want) > K, name                                  # (the host has shorter streams decoded whole)
        assert D.osnappy_uncompress(stream, len(want)) == (0, want), name
        if L.snappy_lib() is not None:
            assert D.ref_snappy_uncompress(stream, len(want)) == (0, want), name
        # the blocks begin on elements, and the stated road-3 count is what the two rules give for the bytes
        blocks = S.blocks_of(stream)
        assert blocks is not None and len(blocks) == (len(want) + K - 1) // K and len(blocks) >= 2, name
        assert [b[2] for b in blocks[:-1]] == [K] * (len(blocks) - 1) and blocks[-1][2] == len(want) - K * (len(blocks) - 1), name
        assert S.expected_blocks(stream) == expected, name
        if sweep != "declines":
            assert expected == len(blocks), name                    # nothing but sweep g may count a decline


def test_plain_decoder_refuses_what_is_not_snappy():
    good = S.varint(12) + S.lit(b"0123") + S.copy2(8, 4)
    assert S.decode(good) == b"0123" * 3
    for what, stream in [("offset zero", S.varint(12) + S.lit(b"0123") + S.copy2(8, 0)),
                         ("offset beyond the start", S.varint(12) + S.lit(b"0123") + S.copy2(8, 5)),
                         ("truncated literal", S.varint(12) + S.lit(b"0123") + S.lit(b"01234567")[:-1]),
                         ("output longer than the prefix", good + S.lit(b"x")),
                         ("output shorter than the prefix", S.varint(13) + good[1:]),
                         ("truncated copy", good[:-1])]:
        with pytest.raises(ValueError):
            S.decode(stream)
        assert D.osnappy_uncompress(stream, 64)[0] != 0, what
        if L.snappy_lib() is not None:
            assert D.ref_snappy_uncompress(stream, 64)[0] != 0, what


def test_element_writers_cover_the_non_canonical_forms():
    # every length form of a literal holds every length it can, and reads back as written
    for extra in range(5):
        for n in (1, 5, 60, 61, 256, 257, 300):
            if n > 60 and extra == 0 or n > 256 and extra == 1:
                continue
            data = bytes(range(256)) * 2
            stream = S.varint(n) + S.lit(data[:n], extra)
            assert [tuple(el) for el in S.elements(stream)] == [(1 if n < 128 else 2, "lit%d" % extra, 1 + extra, n, 0)]
            assert S.decode(stream) == data[:n]
    seen = collections.Counter()
    for _sweep, (_name, stream, _e) in _all_cases():
        for el in S.elements(stream):
            if el.form == "lit1" and el.n <= 60:
                seen["short literal with a length byte"] += 1
            if el.form == "lit4" and el.n == 5:
                seen["five bytes with four length bytes"] += 1
            if el.form in ("copy2", "copy4") and el.off < 2048 and 4 <= el.n <= 11:
                seen[el.form + " a copy1 could hold"] += 1
    assert set(seen) == {"short literal with a length byte", "five bytes with four length bytes",
                         "copy2 a copy1 could hold", "copy4 a copy1 could hold"}, seen


def test_overlap_table_is_complete():
    (_name, stream, _e), = S.sweep_overlap()
    found = collections.defaultdict(set)
    prev = None
    for el in S.elements(stream):
        if el.form.startswith("copy") and el.off < el.n:
            assert prev is not None and prev.form in ("lit0", "lit1") and prev.n == el.off + 3     # the bytes it repeats are seeded ones
            found[el.form].add((el.off, el.n))
        prev = el
    pairs = {(off, n) for off in range(1, 64) for n in range(off + 1, 65)}
    assert found["copy2"] == pairs and len(pairs) == 2016
    assert found["copy1"] == {(off, n) for off, n in pairs if 4 <= n <= 11}
    assert found["copy4"] == {(off, n) for off, n in pairs if off in S.OVERLAP_COPY4_OFFSETS}
    # so every (offset, byte of the copy) pair the first-period arithmetic can meet is there
    assert {(off, rel) for off, n in found["copy2"] for rel in range(n)} == {(off, rel) for off in range(1, 64) for rel in range(64)}


def test_phase_sweep_puts_every_form_at_the_end_of_a_window_and_across_the_scan_segments():
    cases = S.sweep_phase()
    assert len(cases) == 64
    at_byte = collections.defaultdict(set)                     # (form, n) -> window bytes its tag was at, address phase 0
    straddles = {2048: collections.Counter(), 4096: collections.Counter()}
    for _name, stream, _e in cases:
        for el in S.elements(stream):
            if (el.form, el.n) in S.PHASE_FORMS:
                at_byte[(el.form, el.n)].add(el.pos & 63)
                for seg in straddles:
                    for s in S.ADDRESS_PHASES:
                        if (el.pos + s) // seg != (el.pos + s + el.hdr - 1) // seg:
                            straddles[seg][(el.form, el.n, s)] += 1
    for form in S.PHASE_FORMS:
        # every byte of a window at address phase 0, so every byte at any other phase too: 59..63 among them
        assert at_byte[form] == set(range(64)), form
    multi_byte = [f for f in S.PHASE_FORMS if f != ("lit0", 20)]
    for seg in (2048, 4096):
        # a header lies across a segment's end whatever the stream's address
        for s in S.ADDRESS_PHASES:
            assert sum(straddles[seg][(form, n, s)] for form, n in multi_byte) > 0, (seg, s)
    # every copy of the sequence reads seeded literal bytes of its block's first 64, at first or second hand
    for _name, stream, _e in cases[:2]:
        made = 0
        for el in S.elements(stream):
            if el.form.startswith("copy") and (el.form, el.n) in S.PHASE_FORMS and el.form != "copy1":
                assert made % K - el.off + el.n <= 64
            made += el.n


def _windows(stream, first, last, s):
    """{window: [elements that begin in it]} for compressed positions [first, last), address phase s"""
    found = collections.defaultdict(list)
    for el in S.elements(stream):
        if first <= el.pos < last:
            found[(el.pos + s) >> 6].append(el)
    return found


def test_field_width_sweep_holds_its_edges():
    cases = S.sweep_fields()
    name, stream, _e = cases[0]
    blocks = S.blocks_of(stream)
    for s in S.ADDRESS_PHASES:
        got = set()
        for els in _windows(stream, blocks[0][0], blocks[0][1], s).values():
            if (els[0].pos + s) & 63 or els[0].form != "copy2":
                continue
            run = 0
            for el in els[:-1]:                                # (one more tag follows in the same window)
                run += el.n
                if run in (511, 512, 513):
                    got.add((run, 513 if any(e.n == 1 for e in els) else 0))
        assert {(511, 0), (512, 0), (513, 513)} <= got, (s, got)
        # the 256-byte literal with one length byte, tag at the window's last byte
        assert any(el.form == "lit1" and el.n == 256 and (el.pos + s) & 63 == 63
                   for el in S.elements(stream) if blocks[1][0] <= el.pos < blocks[1][1]), s
    seen = {(el.form, el.off, el.n) for el in S.elements(stream) if blocks[2][0] <= el.pos < blocks[2][1]}
    for off in (510, 511, 512, 513):
        assert {("copy2", off, 1), ("copy2", off, 64), ("copy4", off, 1), ("copy4", off, 64), ("copy1", off, 4)} <= seen
    firsts = {el.pos: el for el in S.elements(stream)}
    assert [firsts[b[0]].form for b in blocks[3:]] == ["lit2", "lit3", "lit4", "lit2", "lit2"]
    # ... and the streams whose blocks end in each of the nine forms
    assert len(cases) == 1 + len(S.PHASE_FORMS)
    for (name, stream, _e), form in zip(cases[1:], S.PHASE_FORMS):
        ends = {b[1] for b in S.blocks_of(stream)}
        last = [(el.form, el.n) for el in S.elements(stream) if el.pos + el.hdr + (el.n if el.form.startswith("lit") else 0) in ends]
        assert last == [form, form], name


def test_length_sweep_ends_in_every_tail():
    tails = collections.defaultdict(list)
    for name, stream, _e in S.sweep_lengths():
        blocks = S.blocks_of(stream)
        tails[len(blocks)].append(blocks[-1][2])
        copies = [el for el in S.elements(stream) if el.pos >= blocks[-1][0] and el.form.startswith("copy")]
        assert bool(copies) == (blocks[-1][2] >= 5), name
    assert tails == {2: list(S.TAILS), 3: list(S.THREE_BLOCK_TAILS)}


def test_chain_sweep_is_as_deep_as_it_says():
    cases = dict((name, stream) for name, stream, _e in S.sweep_chains())
    assert len(cases) == 4
    forms = _forms_seen(cases["copy1(4, 4), 16383 deep"])
    assert forms[("copy1", 4)] == 16383
    forms = _forms_seen(cases["copy2(64, 1) run"])
    assert forms[("copy2", 64)] == 1023 and forms[("copy2", 63)] == 1
    first = S.decoded(cases["copy2(64, 1) run"])[:K]
    assert first == first[:1] * K
    kinds = [el.off < el.n for el in S.elements(cases["overlapping and plain copies in turn"]) if el.form == "copy2"][:3000]
    assert kinds[:2] == [True, False] and kinds == kinds[:2] * 1500


def test_ring_sweep_reaches_as_far_back_as_the_rings_are_long():
    (_name, stream, _e), = S.sweep_ring()
    placed = collections.Counter()
    made = 0
    for el in S.elements(stream):
        if el.form.startswith("copy"):
            assert el.off <= made % K                                        # inside its block, every one
            placed[(el.off, el.n)] += 1
        made += el.n
    for ring in S.RINGS:
        for off, n in S.ring_cases(ring):
            assert placed[(off, n)] >= 2, (ring, off, n)
        assert all(placed[(off, 48 if ring == 2048 else 24)] >= 1 for off in range(ring - 1152, ring + 65)), ring


def test_decline_sweep_spans_the_windows_it_says():
    cases = dict((name, (stream, e)) for name, stream, e in S.sweep_declines())
    assert len(cases) == 4
    stream, e = cases["one literal of 64 KiB"]
    (a0, a1, _n, _ok), _tail = S.blocks_of(stream)
    assert e == 1 and all(S.windows_spanned(a0, a1, s) >= 1025 for s in S.ADDRESS_PHASES)
    for name, span, want in (("1024 windows", 1024, 3), ("1025 windows", 1025, 2)):
        stream, e = cases[name]
        blocks = S.blocks_of(stream)
        assert e == want and blocks[1][1] - blocks[1][0] == S.SPAN_BLOCK_COMPRESSED
        for s in S.ADDRESS_PHASES:
            assert S.windows_spanned(blocks[1][0], blocks[1][1], s) == span, (name, s)
            assert S.windows_spanned(blocks[0][0], blocks[0][1], s) < 1024 and S.windows_spanned(blocks[2][0], blocks[2][1], s) < 1024
    a, b = cases["1024 windows"][0], cases["1025 windows"][0]
    assert a[S.blocks_of(a)[1][0]:] == b[S.blocks_of(b)[1][0]:]                 # the same second block, 48 bytes further on
    stream, e = cases[S.REACHING_STREAM]
    assert e == 0 and [b[3] for b in S.blocks_of(stream)] == [True, False]

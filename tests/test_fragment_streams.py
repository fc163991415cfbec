"""The hand-built fragments of tests/_fragment_streams.py, without a GPU: every honest fragment decodes with the plain
Snappy decoder to the bytes its builder recorded and keeps what its table announces; every frame -- and every lie that is
still Snappy -- decodes with the checker libraries to those bytes; the lies that are no Snappy make both checkers
return the code recorded with them; every lie breaks the promise it is named after and no other; and the families hold
what they are meant to hold, read back from the built bytes through the pass model.

What differs from a naive reading of the grammar:
  * lane 1 of a window holds no element: a pass begins with one, and none is a single byte long;
  * under GRAN 2 and 4 the pass totals around 512 are 512 - GRAN and 512 + GRAN, and the farthest copy-2 of a 64 KiB
    fragment lies at 65536 - GRAN;
  * the deepest chain of a step is 31 links (25 with single bytes): five rounds of pointer jumping, never six or seven."""
import pytest

import _fragment_streams as X
import _libs as L
import _snappy_streams as S

CHECKERS = [("oracle", L.oracle_api())] + ([("reference", L.ref_api())] if L.ref_api() is not None else [])
GRANS = list(X.GRANS)


def _all_frames(gran):
    return [fr for fam in X.FAMILIES for fr in X.family_frames(fam, gran)]


@pytest.mark.parametrize("gran", GRANS)
def test_every_honest_fragment_decodes_to_its_recorded_bytes_and_keeps_its_promises(gran):
    names = set()
    for fam in X.FAMILIES:
        for fr in X.family_frames(fam, gran):
            size = 1 << fr.frag_log2
            assert fr.frag_log2 in X.FRAG_LOG2S and len({len(c) for c in fr.chunks}) == 1, fr.label
            for c in fr.chunks:
                assert all(f.made == size for f in c[:-1]) and 1 <= c[-1].made <= size, fr.label
                for f in c:
                    names.add((fr.label, f.name))
                    assert f.gran == gran and f.claims is None and f.total == len(f.stream()), f.name
                    assert S.decode(S.varint(f.made) + f.stream()) == bytes(f.out), f.name
                    assert X.broken([f.stream()], [f.total], gran, fr.window_ok, fr.frag_log2, f.made) == [], f.name
                    assert (X.max_offset(f.stream()) <= X.WINDOW_REACH) or not fr.window_ok, f.name
                    # the model's own invariants hold at every source phase (asserted inside)
                    for phase in (0, 15):
                        X.staging(f.stream(), phase)
                    ps = X.passes(f.stream())
                    assert sum(p.N for p in ps) == f.made and sum(p.adv for p in ps) == f.total, f.name
    assert len(names) == sum(len(c) for fr in _all_frames(gran) for c in fr.chunks)
    # the families that keep the window are all but the rings and the frames of fragments that are no 8 KiB
    assert all(fr.window_ok for fam in ("overlap", "forms", "staging", "passes", "chains", "window") for fr in X.family_frames(fam, gran))


@pytest.mark.parametrize("gran", GRANS)
def test_frames_of_honest_fragments_decode_with_the_checkers(gran):
    for fr in _all_frames(gran):
        for window256, version in ((0, 1), (X.WINDOW_BYTE, 1), (0, 3)):
            if (window256 and not fr.window_ok) or (version == 3 and fr.frag_log2 != 13):
                continue
            built = X.frame_of_fragments(fr.chunks, fr.frag_log2, X.GRAN_LOG2[gran], window256, version=version)
            assert built.want == b"".join(bytes(f.out) for c in fr.chunks for f in c)
            for name, api in CHECKERS:
                assert api.decode(built.frame, 0, len(built.want)) == (0, built.want, X.FMT_DXT5), (name, fr.label)
                assert api.chunk_count(built.frame, 0) == (0, len(fr.chunks)), fr.label
            # where the fragments lie in the frame
            for f, at in zip(built.fragments, built.starts):
                assert built.frame[at: at + f.total] == f.stream(), f.name


def test_the_frame_is_the_hand_written_one():
    """tests/test_gpu_parity.py writes one such frame by hand (test_match_window_promise_is_checked_and_optional)"""
    f = X.Fragment(1, 1).lit(6144, 2, bytes(range(256)) * 24).lit(2048 - 64, 2, bytes(2048 - 64)).copy("copy2", 64, 6144 + 2048 - 64)
    chunk = bytes([0x80, 0x40]) + f.stream()
    tables = bytes([1, 0, 0, 2, 0x0B]) + bytes([4, 0, 0, 3]) + len(chunk).to_bytes(4, "little") + \
        bytes([8, 0, 0, 0x46, 1, 13, 0, 12]) + len(f.stream()).to_bytes(4, "little")
    body = len(tables).to_bytes(3, "little") + bytes([1]) + tables + chunk
    assert X.frame_of_fragments([[f]], 13, 0, 12).frame == len(body).to_bytes(3, "little") + bytes([0xCE]) + body


@pytest.mark.parametrize("gran", GRANS)
def test_every_lie_breaks_the_promise_it_names_and_no_other(gran):
    lies = X.lies(gran)
    honest = X.honest_twin(gran)
    assert X.broken([f.stream() for f in honest], [f.total for f in honest], gran, True, 13, 16384) == []
    built = X.frame_of_fragments([honest], 13, X.GRAN_LOG2[gran], X.WINDOW_BYTE)
    for name, api in CHECKERS:
        assert api.decode(built.frame, 0, 16384) == (0, built.want, X.FMT_DXT5), name
    want = {"offset %d under a window promise" % (3072 + gran), "offset 4096 under a window promise",
            "copy from one unit before the fragment", "an element across the fragment boundary",
            "two sizes of the table moved by one byte", "two sizes of the table moved back by one byte", "offset 0",
            "the last element cut short by the chunk size", "a fragment that makes fewer bytes than its share"}
    if gran >= 2:
        odd = 8 - gran // 2
        want |= {"literal length %d" % odd, "copy length %d" % odd, "copy offset %d" % odd, "serial literal of %d" % odd}
        want |= {"serial literal of 7"} if gran == 4 else set()         # (GRAN 4: a multiple of two and an odd one)
    assert {lie.name.split(": ", 1)[1] for lie in lies} == want
    for lie in lies:
        assert lie.promise in X.PROMISES and X.lie_breaks(lie) == [lie.promise], lie.name
        assert lie.valid == (lie.promise != "snappy"), lie.name
        built = X.frame_of_lie(lie)
        chunk = S.varint(16384) + b"".join(f.stream() for f in lie.chunk)
        chunk = chunk[: len(chunk) - lie.cut]
        if lie.valid:
            assert len(built.want) == 16384 and S.decode(chunk) == built.want, lie.name
            for name, api in CHECKERS:
                assert api.decode(built.frame, 0, 16384) == (0, built.want, X.FMT_DXT5), (lie.name, name)
        else:
            with pytest.raises(ValueError):
                S.decode(chunk)
            assert built.want is None
            for name, api in CHECKERS:
                assert api.decode(built.frame, 0, 16384)[0] == X.RESULT_OF_INVALID, (lie.name, name)
        # a twin: the honest chunk's elements but for a handful
        for f, h in zip(lie.chunk, honest):
            same = sum(1 for x, y in zip(f.parts, h.parts) if x == y) + sum(1 for x, y in zip(f.parts[::-1], h.parts[::-1]) if x == y)
            assert same >= len(h.parts) - 4, lie.name
    # what the lies are about, said with the elements
    by_name = {lie.name.split(": ", 1)[1]: lie for lie in lies}
    reach = by_name["copy from one unit before the fragment"].chunk[1]
    assert [e.off - out for _p, _l, e, out in X._walk(reach.stream()) if e.form.startswith("copy") and e.off > out] == [gran]
    far = [X.max_offset(f.stream()) for lie in lies if lie.promise == "window" for f in lie.chunk]
    assert sorted(far)[-2:] == [3072 + gran, 4096] and all(lie.window256 == X.WINDOW_BYTE for lie in lies if lie.promise == "window")
    assert [f.made for f in by_name["an element across the fragment boundary"].chunk] == [8192 + gran, 8192 - gran]


@pytest.mark.parametrize("gran", GRANS)
def test_the_families_hold_what_they_are_meant_to_hold(gran):
    g = gran
    d = X.describe(g)
    assert X.FAMILIES == ("overlap", "forms", "staging", "passes", "chains", "window", "rings", "ends")
    # overlap: every (offset, length) pair at multiples of GRAN, offsets GRAN..66 and 126..129, lengths up to 64: copy-2
    # and copy-4 for all, copy-1 for 4..11 -- below, at and above the length, on both sides of 127
    offs = [o for o in list(range(1, 67)) + [126, 127, 128, 129] if o % g == 0]
    pairs = {(form, n, off) for off in offs for n in range(g, 65, g) for form in ("copy2", "copy4")}
    pairs |= {("copy1", n, off) for off in offs for n in range(4, 12) if n % g == 0}
    assert d["overlap"] == pairs == set(X.overlap_cases(g))
    assert len(pairs) == {1: 70 * 136, 2: 35 * 68, 4: 17 * 34}[g]         # offsets x (2 x lengths + copy-1 lengths)
    assert 128 in offs and (g == 4 or 126 in offs) and (g > 1 or {127, 129} <= set(offs))   # (GRAN 4: 64 and 128 are the multiples near)
    # forms: every form at every lane a window has but lane 1
    assert X.LANES == (0,) + tuple(range(2, 64))
    assert len(X.form_list(g)) == 21 and set(d["forms"]) == {name for name, _f, _n, _a in X.form_list(g)}
    for name, lanes in d["forms"].items():
        assert lanes == set(X.LANES), name
    assert {form for _n, form, _b, _a in X.form_list(g)} == {"lit0", "lit1", "lit2", "lit3", "lit4", "copy1", "copy2", "copy4"}
    assert ("lit1 256", "lit1", 256, 1) in X.form_list(g)                   # (258 stream bytes at lane 63: the furthest read)
    # staging: every header form split at every byte, across a boundary in the middle of the staged ring and at its
    # wrap; serial literals that end around both; serial literals that leave the ring behind
    assert d["staging splits"] >= {(form, s, parity) for form, hdr in X.HEADER_FORMS for s in range(1, hdr) for parity in (0, 1)}
    assert len(X.staging_splits()) == 34
    assert d["staging serial ends"] == {(e, parity) for e in (-1, 0, 1) for parity in (0, 1)}
    assert d["staging skips"] == [1100, 1700, 2600] and d["staging events"]["restage"] >= 6 and d["staging events"]["advance"] > 50
    assert d["staging memory steps"] >= sum((n - 1024) // 64 for n in X.SKIPS)
    # passes
    assert d["pass totals"] >= {512 - g, 512, 512 + g, 1344} and d["pass totals with a 256-byte literal"] >= {512 - g, 512, 512 + g}
    assert d["passes that end at 512"] >= 2 and d["passes cut"] >= 3 and d["two-byte passes"] == 1
    assert d["most elements in a pass"] == 32
    # chains
    assert d["deepest chain"] == X.DEEPEST[g] and X.DEEPEST[g].bit_length() == 5
    assert d["chain depths"] >= set(range(0, 20))
    assert {(8, 8), (8, 4), (8, 2), (8, 1), (3, 3), (3, 1), (1, 1)} <= d["chain offsets"]
    # window
    w = d["window"]
    assert w["most"] == 3072 and w["at reach"] == {"first", "last"}
    assert w["flush copies"] == set(range(1, 8)) and w["flush serial"] == set(range(1, 8))
    assert w["source across wrap"] >= 1 and w["destination across wrap"] >= 1
    # rings: offsets that are everything made so far, at the start, the middle and the end; the farthest there are
    for k in X.FRAG_LOG2S:
        offs = {off for _form, off in d["rings"][k]}
        assert {64, 1 << (k - 1), (1 << k) - 64 - g, (1 << k) - g} <= offs, k
    assert ("copy2", 65536 - g) in d["rings"][16] and sum(1 for form, off in d["rings"][16] if form == "copy4" and off > 32767) >= 3
    # ends
    ends = dict((tuple(map(tuple, chunks)), log2) for log2, chunks in d["ends"])
    assert [c[-1] for c in d["ends"][0][1]] == [g, 2 * g, 60, 64, 68, 8192 - g]
    assert ((1024,),) in ends and ((g,),) in ends
    assert sorted(len(chunks[0]) for log2, chunks in d["ends"] if log2 == 10 and len(chunks[0]) > 1) == [65, 129]
    sizes = [sum(f.total for f in c) for c in X.family_frames("ends", g)[0].chunks]
    assert len(set(sizes)) == len(sizes)
    assert d["lies"] == {1: 9, 2: 13, 4: 14}[g]
    serial = [e.n for lie in X.lies(g) if "serial literal" in lie.name for f in lie.chunk for e in X.bare_elements(f.stream())
              if e.form in X.SPECIAL and e.n % g]
    assert sorted(serial) == {1: [], 2: [7], 4: [6, 7]}[g]                # an odd serial literal under both granularities

"""The scalar definition of the position-per-lane Snappy compressor (tests/_position_streams.py), without a GPU: what
it writes is Snappy to the plain decoder, to libsnappy and to the oracle; it keeps what the fragment table promises
the decoder; a few tiny streams are what one writes by hand from the rules; its sweeps reach what they are named for
(read from the definition's element lists, not from the generators' intentions); every texture's chunk shrinks, so
that a frame made of it holds Snappy and tests/test_position_streams_gpu.py compares something; and each of four rules
a subtly wrong kernel might break (table visible in the same round, the tie between fixed distances, the copy-1
threshold, the literal edge) decides bytes of the sweep that is there for it."""
import collections

import pytest

import _data as D
import _libs as L
import _position_streams as M
import _snappy_streams as S

SETTINGS = [pytest.param(s, id="g%d-p%d-f%d%s" % (s[0], s[1], s[2], "-w" if s[3] else "")) for s in M.SETTINGS + [M.BIG]]
EIGHT_K = [pytest.param(s, id="g%d-p%d%s" % (s[0], s[1], "-w" if s[3] else "")) for s in M.SETTINGS if s[2] == 13]


def textures(setting):
    """[(name, texture, chunks)] of a setting: the GPU tests' inputs"""
    gran, pitch, log2, window = setting
    if setting == M.BIG:
        return [("sweeps", M.texture(gran, pitch, log2, None, ("lengths", "offsets"))[0], 1)]
    found = [("sweeps", M.texture(gran, pitch, log2, window, total=(1 << 20) if window else None)[0], 1)]
    if not window:
        found += [(name, data, 1) for name, data in M.sweep_ends(gran, pitch, 1 << log2)]
        if pitch == 8:
            found.append(("unaligned", M.unaligned_texture(gran, pitch)[0], 2))
    return found


def case_fragments(setting):
    """[(name, fragment bytes)]: every fragment that holds a case"""
    gran, pitch, log2, window = setting
    size = 1 << log2
    sweeps = ("lengths", "offsets") if setting == M.BIG else tuple(M.FRAGMENT_SWEEPS)
    found = [(name, c) for sweep in sweeps for name, c in M.cases(sweep, gran, pitch, size, window)]
    if not window and setting != M.BIG:
        found += [(name, data[size:]) for name, data in M.sweep_ends(gran, pitch, size)]
    return found


@pytest.mark.parametrize("setting", SETTINGS)
def test_streams_are_snappy_to_every_decoder_and_every_chunk_shrinks(setting):
    gran, pitch, log2, window = setting
    for name, data, chunks in textures(setting):
        cb = len(data) // chunks
        for c in range(chunks):
            chunk = data[c * cb: (c + 1) * cb]
            stream, sizes = M.model_chunk(chunk, gran, pitch, log2, window)
            assert len(stream) < cb, (name, c, len(stream), cb)             # else the frame stores the chunk as it is
            assert len(sizes) == -(-cb // (1 << log2))
            assert S.decode(stream) == chunk, (name, c)
            assert D.osnappy_uncompress(stream, cb) == (0, chunk), (name, c)
            if L.snappy_lib() is not None:
                assert D.ref_snappy_uncompress(stream, cb) == (0, chunk), (name, c)


@pytest.mark.parametrize("setting", SETTINGS)
def test_streams_keep_what_the_fragment_table_promises(setting):
    gran, pitch, log2, window = setting
    sup = M.supertile_bytes(gran)
    for name, data in case_fragments(setting):
        els, stream = M.modelled(data, gran, pitch, window)
        parsed = list(M.stream_elements(stream))
        assert len(parsed) == len(els), name
        made = 0
        for el, p in zip(els, parsed):
            # the element list is what the stream says
            assert el.pos == made and el.n == p.n and el.off == p.off, (name, el, p)
            assert p.form == ("lit0" if el.n <= 60 else "lit1") if el.kind == "lit" else p.form == el.kind, (name, el, p)
            assert el.n % gran == 0 and el.off % gran == 0 and el.pos % gran == 0, (name, el)
            assert el.pos // sup == (el.pos + el.n - 1) // sup, (name, el)
            if el.kind != "lit":
                assert 4 <= el.n <= 64 and 0 < el.off <= el.pos, (name, el)
                assert (el.kind == "copy1") == (el.n < 12 and el.off < 2048), (name, el)
                if window and el.via == "hash":
                    assert el.off <= window, (name, el)
            else:
                assert el.pos // M.tile_bytes(gran) == (el.pos + el.n - 1) // M.tile_bytes(gran), (name, el)
            made += el.n
        assert made == len(data), name


# ------------------------------------------------------------------------------------------- written out by hand --
X = bytes(range(0x41, 0x51))                     # sixteen bytes, all different


def test_tiny_streams_written_out_by_hand():
    # 1. 64 equal bytes.  Position 0 is a literal granule (nothing lies in front of it).  At the next position the
    #    table's entry was never written and offers position 0: everything agrees, the room is what is left of the
    #    data (63 / 62 / 60 bytes); no fixed distance exists yet (the position is nearer than a pitch to the start).
    #    One literal of GRAN bytes, one copy-2 (12 bytes and more) at offset GRAN.
    run = bytes([7]) * 64
    assert M.compress_fragment(run, 1, 16) == bytes([0 << 2, 7]) + bytes([2 | (62 << 2), 1, 0])
    assert M.compress_fragment(run, 2, 16) == bytes([1 << 2, 7, 7]) + bytes([2 | (61 << 2), 2, 0])
    assert M.compress_fragment(run, 4, 8) == bytes([3 << 2, 7, 7, 7, 7]) + bytes([2 | (59 << 2), 4, 0])
    assert M.compress_chunk(run, 2, 16) == bytes([64, 4, 7, 7, 0xF6, 2, 0])
    # 2. two equal blocks of sixteen different bytes.  Sixteen literal bytes (every entry looked up offers position 0,
    #    which does not agree); at 16 the block repeats one pitch back (two pitches at pitch 8) for the 16 bytes that
    #    are left.  The table offers position 0 as well, the same 16 bytes: a fixed distance wins at equal length, and
    #    the offset is the same.  Literal tag (16 - 1) << 2, copy-2 tag 2 | (16 - 1) << 2, offset 16.
    for gran in (1, 2, 4):
        for pitch in (8, 16):
            assert M.compress_fragment(X + X, gran, pitch) == bytes([0x3C]) + X + bytes([0x3E, 16, 0]), (gran, pitch)
            assert M.fragment_elements(X + X, gran, pitch)[1] == M.El(16, "copy2", 16, 16, "fixed", 16 // pitch)
    # 3. five bytes repeat one pitch back.  At GRAN 1 a copy of 5: copy-1, tag 1 | (5 - 4) << 2, offset byte 16, then
    #    3 literal bytes.  At GRAN 2 the third granule agrees in its first byte only: a copy of 4 (tag 1), and the
    #    fifth byte leaves as a literal with the three behind it.  GRAN 4 the same.
    tail = bytes([0xF1, 0xF2, 0xF3])
    data = X + X[:5] + tail
    assert M.compress_fragment(data, 1, 16) == bytes([0x3C]) + X + bytes([0x05, 16]) + bytes([2 << 2]) + tail
    for gran in (2, 4):
        assert M.compress_fragment(data, gran, 16) == bytes([0x3C]) + X + bytes([0x01, 16]) + bytes([3 << 2]) + X[4:5] + tail
    # 4. eleven and twelve bytes repeat: copy-1 (tag 1 | 7 << 2) up to 11, copy-2 (tag 2 | 11 << 2, two offset bytes) from 12
    assert M.compress_fragment(X + X[:11] + bytes([0xF1]), 1, 16) == bytes([0x3C]) + X + bytes([0x1D, 16]) + bytes([0, 0xF1])
    assert M.compress_fragment(X + X[:12] + bytes([0xF1, 0xF2, 0xF3, 0xF4]), 4, 16) == \
        bytes([0x3C]) + X + bytes([0x2E, 16, 0]) + bytes([3 << 2, 0xF1, 0xF2, 0xF3, 0xF4])
    # 5. 61 literal bytes at GRAN 1 (nothing repeats in 61 different bytes): tag 60 << 2 and a length byte 60; 60: the tag alone
    d61 = bytes(range(1, 62))
    assert M.compress_fragment(d61, 1, 16) == bytes([0xF0, 60]) + d61
    assert M.compress_fragment(d61[:60], 1, 16) == bytes([59 << 2]) + d61[:60]
    # 6. a literal ends with its tile: 64 different bytes and two more at GRAN 1 are a literal of 64 and one of 2
    d66 = bytes(range(1, 67))
    assert M.compress_fragment(d66, 1, 16) == bytes([0xF0, 63]) + d66[:64] + bytes([1 << 2]) + d66[64:]
    # 7. three 8-byte blocks that begin with the same 4 bytes, pitch 8.  The second takes its 4 from the first (one
    #    pitch; the table's unwritten entry offers the same place, the fixed distance wins).  The third finds them one
    #    and two pitches back, 4 bytes either way: the kernel's key is length << 3 | pitches and the larger key wins, so
    #    the FARTHER distance, offset 16 (its comment said the nearer until this test was written).
    h = bytes([0x61, 0x62, 0x63, 0x64])
    blocks = h + bytes([1, 2, 3, 4]) + h + bytes([5, 6, 7, 8]) + h + bytes([9, 10, 11, 12])
    for gran in (1, 2, 4):
        assert M.compress_fragment(blocks, gran, 8) == bytes([7 << 2]) + blocks[:8] + bytes([0x01, 8]) + \
            bytes([3 << 2, 5, 6, 7, 8]) + bytes([0x01, 16]) + bytes([3 << 2, 9, 10, 11, 12]), gran


# ------------------------------------------------------------------------------- the sweeps are what their names say --
def _copies(setting, sweep):
    """[{position: element} of the copies] per case fragment of a sweep"""
    gran, pitch, log2, window = setting
    return [{e.pos: e for e in M.modelled(c, gran, pitch, window)[0] if e.kind != "lit"}
            for _name, c in M.cases(sweep, gran, pitch, 1 << log2, window)]


@pytest.mark.parametrize("setting", SETTINGS)
def test_length_sweep_lands_on_every_length(setting):
    gran, pitch, log2, window = setting
    size, rnd = 1 << log2, M.round_bytes(gran)
    fixed, far = M.lengths_fixed_places(gran, size), M.lengths_hash_places(gran, size)
    copies = _copies(setting, "lengths")
    first_far = max(p[0] for p in fixed) + 1
    assert [n for _f, _at, n in fixed] == list(range(3, 71))
    assert [n for _f, _at, n in far] == (list(range(3, 71)) if size >= 2 * rnd else [])
    seen = collections.Counter()
    for places, via, off, base in ((fixed, "fixed", pitch, 0), (far, "hash", rnd, first_far)):
        for frag, at, n in places:
            got = copies[base + frag]
            whole = n - n % gran                              # what GRAN leaves of the repeat
            if whole < 4:
                assert at not in got, (via, n)
                seen[via, "no copy"] += 1
                continue
            first = min(whole, 64)
            e = got[at]
            assert (e.n, e.off, e.via) == (first, off, via), (via, n, e)
            assert e.kind == ("copy1" if first < 12 and off < 2048 else "copy2"), (via, n, e)
            seen[via, e.kind] += 1
            if whole != n:
                seen[via, "rounded down"] += 1
            if whole - 64 >= 4:
                e = got[at + 64]                              # the cap at 64 and a second copy behind it
                # (64 bytes into a repeat of period `pitch` all four distances agree for what is left: the farthest)
                assert (e.n, e.off, e.via) == (whole - 64, 4 * pitch if via == "fixed" else off, via), (via, n, e)
                seen[via, "second copy"] += 1
            else:
                assert at + 64 not in got
    for via in ("fixed", "hash") if far else ("fixed",):
        assert seen[via, "no copy"] >= 1 and seen[via, "copy2"] >= 50 and seen[via, "second copy"] >= 1
        assert seen[via, "copy1"] >= 2 or (via == "hash" and rnd >= 2048)       # (a round back is 2048 bytes at GRAN 4)
        assert gran == 1 or seen[via, "rounded down"] >= 30


@pytest.mark.parametrize("setting", SETTINGS)
def test_offset_sweep_holds_its_edges_and_its_ties(setting):
    gran, pitch, log2, window = setting
    size, rnd = 1 << log2, M.round_bytes(gran)
    cases = dict((name, c) for name, c in M.cases("offsets", gran, pitch, size, window))
    if size >= 8192:
        els = [e for e in M.modelled(cases["offsets"], gran, pitch, window)[0] if e.via == "hash" and e.n == 8]
        forms = {e.off: e.kind for e in els}
        for d in M.offsets_of(gran, size, window):
            if window and d > window:
                assert d not in forms                                       # the next granule behind the window: not taken
            else:
                assert forms[d] == ("copy1" if d < 2048 else "copy2"), d
        assert {2044, 2048} <= set(forms) and (window or size - 12 in forms)
        if window:
            assert window in forms and window - gran in forms
        else:
            last = M.modelled(cases["offset size - 4"], gran, pitch)[0][-1]
            assert (last.pos, last.n, last.off, last.via) == (size - 4, 4, size - 4, "hash")
        if size > 32768:
            assert forms[32768] == forms[32768 + gran] == forms[40000] == "copy2"
    by_pos = {e.pos: e for e in M.modelled(cases["ties"], gran, pitch, window)[0]}
    base = size - rnd if size >= 2 * rnd else 0
    t = base + 64
    # three blocks with the same first 4 bytes: the second takes them one pitch back, the third could take them one
    # or two pitches back and takes the farther
    assert (by_pos[t + pitch].n, by_pos[t + pitch].pitches) == (4, 1)
    assert (by_pos[t + 2 * pitch].n, by_pos[t + 2 * pitch].pitches, by_pos[t + 2 * pitch].off) == (4, 2, 2 * pitch)
    if size >= 2 * rnd:
        q, r = base + 192, base + 320
        assert (by_pos[q].via, by_pos[q].n) == ("hash", 8)
        assert (by_pos[q + pitch].via, by_pos[q + pitch].n, by_pos[q + pitch].off) == ("fixed", 8, pitch)      # equal: fixed
        assert (by_pos[r].via, by_pos[r].n) == ("hash", 8)
        e = by_pos[r + pitch]
        assert (e.via, e.n, e.off) == ("hash", 8 + gran, r + pitch - (base - rnd + 120))                       # longer by a granule: hash


@pytest.mark.parametrize("setting", SETTINGS[:-1])
def test_position_sweep_begins_a_repeat_at_every_position_of_a_supertile(setting):
    gran, pitch, log2, window = setting
    size, sup, tile = 1 << log2, M.supertile_bytes(gran), M.tile_bytes(gran)
    copies = _copies(setting, "positions")
    lits = [[e for e in M.modelled(c, gran, pitch, window)[0] if e.kind == "lit"]
            for _name, c in M.cases("positions", gran, pitch, size, window)]
    seen = collections.Counter()
    starts = {12: set(), 64: set()}
    for frag, at, n, j in M.positions_places(gran, size):
        assert at % sup == gran * j
        room = min(n, sup - gran * j, size - at)
        starts[n].add(j)
        if room < 4:
            assert at not in copies[frag], (n, j)              # too near the supertile's end for a copy
            seen["nearer than 4 bytes to the supertile's end"] += 1
            e = None
        else:
            e = copies[frag][at]
            assert (e.n, e.off, e.via) == (room, pitch, "fixed"), (n, j, e)
        if j >= 32 and e:
            seen["lanes from 32 on"] += 1
        if e and gran * j < tile < gran * j + e.n:
            seen["carried into the second tile"] += 1
            # literals begin right behind the carried copy
            assert any(l.pos == at + e.n for l in lits[frag]), (n, j)
        if room < n:
            seen["cut at the supertile's end"] += 1
            rest = n - room
            if rest - rest % gran >= 4 and at + room < size:
                again = copies[frag][at + room]                # what is left begins the next supertile
                # (the period began a pitch in front of the repeat: the farthest distance that lies inside it)
                assert (again.n, again.off) == (rest - rest % gran, min(4, room // pitch + 1) * pitch), (n, j, again)
                seen["and taken up behind it"] += 1
    assert starts[12] == starts[64] == set(range(128))
    for what in ("lanes from 32 on", "carried into the second tile", "cut at the supertile's end", "and taken up behind it"):
        assert seen[what] >= 4 or (what == "and taken up behind it" and size == 2 * sup), (what, seen)
    assert gran == 4 or seen["nearer than 4 bytes to the supertile's end"] >= 1


@pytest.mark.parametrize("setting", SETTINGS[:-1])
def test_literal_sweep_holds_the_lengths_it_is_there_for(setting):
    gran, pitch, log2, window = setting
    tile = M.tile_bytes(gran)
    lits, forms, between, carried = collections.Counter(), collections.Counter(), [], []
    for _name, data in M.cases("literals", gran, pitch, 1 << log2, window):
        els, stream = M.modelled(data, gran, pitch, window)
        lits.update(e.n for e in els if e.kind == "lit")
        forms.update((p.form, p.n) for p in M.stream_elements(stream))
        between += [b for a, b, c in zip(els, els[1:], els[2:])
                    if a.kind != "lit" and c.kind != "lit" and b.kind == "lit" and b.n == gran]
        # a literal that begins behind a copy carried into its tile
        carried += [b.n for a, b in zip(els, els[1:])
                    if a.kind != "lit" and b.kind == "lit" and a.pos // tile != (a.pos + a.n - 1) // tile and b.pos % tile]
    assert lits[60] >= 1 and lits[60 + gran] >= 1 and lits[tile] >= 1        # (a whole tile: 256 bytes at GRAN 4)
    assert between and set(carried) >= {60, 60 + gran}, carried
    assert forms[("lit0", 60)] >= 1 and forms[("lit1", 60 + gran)] >= 1 and forms[("lit1", tile)] >= 1


@pytest.mark.parametrize("setting", EIGHT_K)
def test_table_sweep_tells_its_cases_apart(setting):
    gran, pitch, log2, window = setting
    rnd, sup = M.round_bytes(gran), M.supertile_bytes(gran)
    (_name, data), = M.cases("table", gran, pitch, 1 << log2, window)
    stats = collections.Counter()
    by_pos = {e.pos: e for e in M.fragment_elements(data, gran, pitch, window, stats=stats)}
    hashed = lambda at: (by_pos[at].via, by_pos[at].off, by_pos[at].n) if at in by_pos and by_pos[at].kind != "lit" else None
    assert data[96: 104] == data[16: 24] and hashed(96) is None                                 # same round: not found
    assert hashed(sup + 16 + rnd) == ("hash", rnd, 8)                                           # the round before: found
    at = 2 * rnd + sup + 48
    assert data[at: at + 8] == data[sup + 48: sup + 56] == data[3 * sup + 16: 3 * sup + 24]
    assert hashed(3 * sup + 16) is None and hashed(at) == ("hash", at - (3 * sup + 16), 8)      # of two in a round the higher
    at = 3 * rnd + 2 * sup + 32
    assert hashed(rnd + 2 * sup + 32) == ("hash", rnd, 16)
    assert data[at: at + 8] == data[rnd + 2 * sup + 36: rnd + 2 * sup + 44]
    assert hashed(at) == ("hash", 3 * rnd - 4, 8)                                               # not what lay inside a copy
    assert hashed(2 * sup + 80) == ("hash", 2 * sup + 80, 8)                                    # an entry never written: position 0
    assert stats["hash candidates at position 0 from an entry never written"] >= 1
    assert stats["entries never written that fail the comparison"] >= 100 and stats["entries that fail the comparison"] >= 10


@pytest.mark.parametrize("setting", [s for s in SETTINGS[:-1] if not s.values[0][3]])
def test_end_sweep_ends_where_it_says(setting):
    gran, pitch, log2, window = setting
    size, tile, sup = 1 << log2, M.tile_bytes(gran), M.supertile_bytes(gran)
    sizes = []
    for name, data in M.sweep_ends(gran, pitch, size):
        n = len(data) - size
        els = M.modelled(data[size:], gran, pitch)[0]
        copies = [e for e in els if e.kind != "lit"]
        if "begins" in name:
            back = int(name.split()[2])
            assert data[-back:] == data[-back - pitch: -pitch] and data[-back - 1] != data[-back - pitch - 1]
            # four bytes left: a copy of them; fewer: literals to the end
            assert [(e.pos, e.n) for e in copies if e.pos >= n - 4] == ([(n - 4, 4)] if back == 4 else []), (name, els)
            continue
        sizes.append(n)
        assert copies and copies[-1].pos + copies[-1].n >= n - 3, (name, els)       # a copy runs to the data's end, or as near as 4 bytes allow
    assert sizes == [16, 48, tile - gran, tile + gran, sup - gran, sup + gran]
    assert sum(1 for n in sizes if n & 15) >= (2 if gran == 4 else 4)               # the 16-byte loads' ragged end
    if pitch == 8:
        data, chunk = M.unaligned_texture(gran, pitch)
        assert chunk % 16 == 8 and (chunk // 8) % 2 == 1 and len(data) == 2 * chunk


# -------------------------------------------------------------------------- every rule decides bytes of the sweeps --
# (lengths are multiples of GRAN: a threshold moved by less than a granule moves nothing, so the two length thresholds
# move by one granule -- 12 -> 11 and 60 -> 61 at GRAN 1)
PERTURBED = {
    "hash visible in the same round": (lambda gran: M.RULES._replace(same_round_visible=True), "table"),
    "tie to the nearer fixed distance": (lambda gran: M.RULES._replace(tie_farther=False), "offsets"),
    "copy-1 threshold a granule lower": (lambda gran: M.RULES._replace(copy1_below=12 - gran), "lengths"),
    "literal edge a granule higher": (lambda gran: M.RULES._replace(literal_tag_max=60 + gran), "literals"),
}


@pytest.mark.parametrize("what", sorted(PERTURBED))
@pytest.mark.parametrize("setting", EIGHT_K)
def test_a_definition_with_one_rule_moved_writes_other_bytes(setting, what):
    """A kernel that differed from the definition in one of these rules would fail the byte comparison on the sweep
    named beside the rule (and the hand-written streams pin which of the two is the definition)."""
    gran, pitch, log2, window = setting
    make, sweep = PERTURBED[what]
    rules = make(gran)
    differing = [name for name, c in M.cases(sweep, gran, pitch, 1 << log2, window)
                 if M.compress_fragment(c, gran, pitch, window, rules) != M.modelled(c, gran, pitch, window)[1]]
    assert differing, what
    if sweep == "offsets":
        assert "ties" in differing

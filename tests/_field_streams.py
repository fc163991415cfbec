"""Hand-built field streams for the block-per-lane decoder (hap_amd/csrc/snappy_decode_fields.hip), the promises of
include/hap_gpu.h (section 0x46, version 4) as a plain checker, and the frames around them.

A field stream is ordinary Snappy -- the element writers and the plain decoder are tests/_snappy_streams.py's -- cut into
fragments of at most 8 KiB of output whose elements keep extra promises.  Everything here is written from the format
description in include/hap_gpu.h and from the frame rules of hap_frame.c / decode_expand_kernel.  No GPU, no ctypes:
tests/test_field_streams.py holds every case to conforms(), to the plain decoder and to the checker libraries, and
tests/test_field_streams_gpu.py then runs them through the table road and the guess road of the kernel.

Every fragment builder records the bytes it produces, so the expected output of a case is known by construction.

Two limits of the kernel are not promises of the public header; they are restated here from the kernel's text so that
the generators can say on which side a case lies (K_BUF_BYTES names the constant):
  room_ok():         no element's bytes are reached by the output of the steps in front of its own (the "overrun" check);
  records_in_lds():  the 4-byte records of all elements fit below the parked input in LDS.
"""
import collections
import functools

import numpy as np

import _snappy_streams as S

FRAG = 8192                        # output bytes of a fragment
HALF = 128                         # output bytes of a half-tile
GT = 196                           # bytes of a group table: 64 x 24 bits, LE16 element count, LE16 zero
MAX_COMPRESSED = FRAG + 320        # kMaxFragCompressed
K_BUF_BYTES = 9344 + 32            # kBufBytes = SDF_BUF_BYTES, hap_amd/csrc/snappy_decode_fields.hip:66
SOURCE_ALIGNMENTS = tuple(range(16))
OUTPUT_OFFSETS = (0, 1, 4, 8)

FMT_DXT1, FMT_DXT5, FMT_YCOCG, FMT_RGTC1, FMT_BC7 = 0x83F0, 0x83F3, 0x01, 0x8DBB, 0x8E8C
FORMAT_NIBBLE = {FMT_DXT1: 0xB, FMT_DXT5: 0xE, FMT_YCOCG: 0xF, FMT_RGTC1: 0x1, FMT_BC7: 0xC}

Layout = collections.namedtuple("Layout", "code fields block unit gran formats")
# fields: (byte position in the block, bytes); unit: bytes per position of the start mask; gran: the granularity nibble
# the library writes beside the layout (tests/test_field_streams_gpu.py reads it off frames the library encodes)
LAYOUTS = collections.OrderedDict([
    (4, Layout(4, ((0, 2), (2, 6), (8, 4), (12, 4)), 16, 2, 1, (FMT_DXT5, FMT_YCOCG))),
    (2, Layout(2, ((0, 4), (4, 4)), 8, 4, 2, (FMT_DXT1,))),
    (6, Layout(6, ((0, 2), (2, 6)), 8, 2, 1, (FMT_RGTC1,))),
    (8, Layout(8, ((0, 4), (4, 4), (8, 4), (12, 4)), 16, 4, 2, (FMT_BC7,))),
])
GUESS_LAYOUTS = (4, 2, 6)          # field_layout_of_format knows none for BC7


def step_bytes(layout):
    return 64 * LAYOUTS[layout].block


def on_field(layout, p):
    lay = LAYOUTS[layout]
    return (p % lay.block) in {fp for fp, _n in lay.fields}


# ------------------------------------------------------------------------------------------------- group tables --
def unpack_groups(table):
    """(compressed bytes of the 64 groups, bytes they produce, element count)"""
    table = bytes(table)
    assert len(table) == GT and table[194:196] == bytes(2)
    entries = [int.from_bytes(table[3 * g: 3 * g + 3], "little") for g in range(64)]
    return [e & 0xFFF for e in entries], [e >> 12 for e in entries], int.from_bytes(table[192:194], "little")


def pack_groups(sizes, made, elements):
    assert len(sizes) == 64 and len(made) == 64 and all(0 <= v < 4096 for v in list(sizes) + list(made))
    return b"".join((c | (m << 12)).to_bytes(3, "little") for c, m in zip(sizes, made)) + elements.to_bytes(2, "little") + bytes(2)


def element_lengths(e):
    """(bytes of the element in the stream, bytes it produces) of one hand-made Snappy element"""
    tag = e[0]
    kind = tag & 3
    if kind == 0:
        code = tag >> 2
        return len(e), code + 1 if code < 60 else int.from_bytes(e[1: code - 58], "little") + 1
    return len(e), 4 + ((tag >> 2) & 7) if kind == 1 else (tag >> 2) + 1


def group_table(elements):
    """The group table of a fragment made of these elements (byte strings): 64 groups of ceil(N / 64) elements."""
    lens = [element_lengths(e) for e in elements]
    n = len(lens)
    per = (n + 63) // 64
    return pack_groups([sum(c for c, _m in lens[g * per: (g + 1) * per]) for g in range(64)],
                       [sum(m for _c, m in lens[g * per: (g + 1) * per]) for g in range(64)], n)


# ------------------------------------------------------------------------------------------------ the promises --
PROMISES = ("copy-4", "literal length", "field boundary", "half-tile", "copy offset", "compressed size", "element count")


def broken(stream, layout, out_len):
    """The promises of section 0x46 version 4 that the bare elements `stream` of one fragment break, in the order of
    the first offence.  Plain Python over the elements; out_len: what the fragment is to produce."""
    lay = LAYOUTS[layout]
    found = []

    def note(what):
        if what not in found:
            found.append(what)
    p = n = 0
    for el in S.elements(S.varint(out_len) + bytes(stream)):
        n += 1
        if el.form == "copy4":
            note("copy-4")
        if el.form in ("lit2", "lit3", "lit4"):
            note("literal length")
        if not on_field(layout, p) or not on_field(layout, p + el.n):
            note("field boundary")
        if p // HALF != (p + el.n - 1) // HALF:
            note("half-tile")
        if el.form.startswith("copy") and (el.off % lay.block or el.off < lay.block or el.off > p):
            note("copy offset")
        p += el.n
    assert p == out_len, "the elements produce %d bytes, not %d" % (p, out_len)
    if len(stream) > MAX_COMPRESSED:
        note("compressed size")
    if n == 0 or 4 * n > out_len or out_len % lay.block or out_len > FRAG:
        note("element count")
    return found


def conforms(stream, layout, out_len):
    """None where the fragment keeps every promise, else the name of the first one it breaks"""
    found = broken(stream, layout, out_len)
    return found[0] if found else None


# ------------------------------------------------------------------------------------------ the fragment builder --
class Fragment:
    """Elements of one fragment and the bytes they make.  before: the output in front of the fragment in its chunk, for
    the one lie that reaches into it."""

    def __init__(self, layout, seed, before=b""):
        self.layout = layout
        self.lay = LAYOUTS[layout]
        self.pool = np.random.default_rng(seed).integers(0, 256, FRAG + 512, dtype=np.uint8).tobytes()
        self.taken = 0
        self.before = bytes(before)
        self.parts = []
        self.out = bytearray()
        self.total = 0

    @property
    def made(self):
        return len(self.out)

    def stream(self):
        return b"".join(self.parts)

    def _add(self, part):
        self.parts.append(part)
        self.total += len(part)

    def lit(self, n, length_bytes=None):
        """n seeded bytes"""
        data = self.pool[self.taken: self.taken + n]
        assert len(data) == n
        self.taken += n
        self._add(S.lit(data, length_bytes))
        self.out += data
        return self

    def copy(self, n, off, form=None):
        if form is None:
            form = "copy1" if 4 <= n <= 11 and off < 2048 else "copy2"
        self._add(S.COPY_WRITERS[form](n, off))
        made = self.made
        if off > made:
            src = self.before + bytes(self.out)
            assert off <= len(src) and off >= n
            self.out += src[len(src) - off: len(src) - off + n]
        elif off >= n:
            self.out += self.out[made - off: made - off + n]
        else:
            self.out += (bytes(self.out[made - off:]) * (n // off + 1))[:n]
        return self

    def lits_to(self, q, most=60):
        """Literals of at most `most` bytes up to output position q, each ending on a field boundary inside its half-tile"""
        while self.made < q:
            p = self.made
            m = min(most, q - p, HALF - p % HALF)
            while not on_field(self.layout, p + m):
                m -= 1
            self.lit(m)
        assert self.made == q
        return self

    def field_lits(self, blocks=1):
        """every field of the next `blocks` blocks a literal of its own"""
        for _ in range(blocks):
            for _fp, fn in self.lay.fields:
                self.lit(fn)
        return self

    def field_copies_to(self, q, d):
        """every field up to q a copy of its own from d blocks back"""
        while self.made < q:
            for _fp, fn in self.lay.fields:
                self.copy(fn, d * self.lay.block)
        return self


def from_cuts(layout, seed, out_len, cuts, kind):
    """A fragment whose elements begin at the output positions `cuts`; kind(i, p, n) says what element i is:
    ("lit", length bytes or None) or ("copy", blocks back)"""
    f = Fragment(layout, seed)
    cuts = sorted(cuts)
    assert cuts[0] == 0 and cuts[-1] < out_len
    for i, p in enumerate(cuts):
        n = (cuts[i + 1] if i + 1 < len(cuts) else out_len) - p
        what = kind(i, p, n)
        if what[0] == "lit":
            f.lit(n, what[1])
        else:
            f.copy(n, what[1] * f.lay.block)
    return f


def field_starts(layout, out_len):
    lay = LAYOUTS[layout]
    return [b + fp for b in range(0, out_len, lay.block) for fp, _n in lay.fields]


def spread_cuts(layout, out_len, count):
    """`count` element starts: every half-tile's first byte (every 64th byte where the count allows: what a copy can
    span), the rest evenly over the field starts"""
    starts = field_starts(layout, out_len)
    must = set(range(0, out_len, HALF))
    if count >= len(range(0, out_len, 64)):
        must = set(range(0, out_len, 64))
    rest = [p for p in starts if p not in must]
    need = count - len(must)
    assert 0 <= need <= len(rest), (out_len, count)
    return sorted(must | {rest[j * len(rest) // need] for j in range(need)})


def _mixed_kind(lay, salt=0):
    def kind(i, p, n):
        near = p // lay.block
        if near == 0 or n > 64 or (i + salt) % 3 == 0:
            return ("lit", 1 if n > 60 or (i + salt) % 7 == 0 else None)
        return ("copy", 1 + (i * 7 + salt) % min(near, 67))
    return kind


def mixed(layout, seed, out_len=FRAG, count=None):
    """A compact mixed fragment: literals in both forms, copy-1 and copy-2 at assorted distances"""
    if count is None:
        count = max(-(-out_len // HALF), min(out_len // 20, len(field_starts(layout, out_len))))
    return from_cuts(layout, seed, out_len, spread_cuts(layout, out_len, count), _mixed_kind(LAYOUTS[layout], seed))


# -------------------------------------------------------------------------- the two limits the header does not state --
def parked_at(total, shift):
    """S of the kernel: where the fragment's first compressed byte lies in the LDS buffer"""
    return ((K_BUF_BYTES - 16 - total - shift) & ~15) + shift


def room_ok(frag, shift):
    step = step_bytes(frag.layout)
    s, p, c = parked_at(frag.total, shift), 0, 0
    for e in frag.parts:
        clen, n = element_lengths(e)
        if (p & ~(step - 1)) > s + c:
            return False
        p += n
        c += clen
    return True


def records_in_lds(frag, shift):
    return 4 * len(frag.parts) <= parked_at(frag.total, shift) - shift


def records_fit(frag, shift, dst_address):
    """False: the records would go to memory and, rounded up to a 4-byte address, not fit the fragment's own output"""
    return records_in_lds(frag, shift) or 4 * len(frag.parts) + (-dst_address) % 4 <= frag.made


# ------------------------------------------------------------------------------------------------------ families --
Case = collections.namedtuple("Case", "name layout frag fragments")     # fragments of the case's chunk: 1 or 3


def _case(name, frag, fragments=1):
    return Case("%d: %s" % (frag.layout, name), frag.layout, frag, fragments)


def chains(layout):
    """Block 0 of each step a literal; in every later block one field copies from d blocks back"""
    lay, cases = LAYOUTS[layout], []
    for k in range(len(lay.fields)):
        for d in range(1, 64):
            f = Fragment(layout, 1000 * layout + 64 * k + d)
            for b in range(128):
                for j, (_fp, fn) in enumerate(lay.fields):
                    if j == k and b % 64 and b >= d:
                        f.copy(fn, d * lay.block)
                    else:
                        f.lit(fn)
            cases.append(_case("chain field %d d %d" % (k, d), f))
    return cases


MIXED_DISTANCES = (3, 17, 1, 40)


def chains_mixed(layout):
    lay = LAYOUTS[layout]
    f = Fragment(layout, 2000 + layout)
    for b in range(192):
        for j, (_fp, fn) in enumerate(lay.fields):
            d = MIXED_DISTANCES[j]
            if b >= d:
                f.copy(fn, d * lay.block)
            else:
                f.lit(fn)
    return [_case("chains mixed", f)]


def chains_long(layout):
    lay = LAYOUTS[layout]
    a = Fragment(layout, 2100 + layout).lit(lay.block)
    while a.made < 2 * step_bytes(layout):
        a.copy(min(64, HALF - a.made % HALF), lay.block, "copy2")
    b = Fragment(layout, 2110 + layout).field_lits().field_copies_to(2 * step_bytes(layout), 1)
    return [_case("long chain, overlapping copies", a), _case("long chain, a copy per field", b)]


ROW_DISTANCES = (1, 2, 4, 8)


def chains_rows(layout):
    lay, step, cases = LAYOUTS[layout], step_bytes(layout), []
    for d in ROW_DISTANCES:
        f = Fragment(layout, 2200 + 10 * layout + d)
        f.field_lits(4 + d).field_copies_to(step, d)                  # roots in blocks 4 .. 4 + d - 1, not in block 0
        f.field_lits(d).field_copies_to(2 * step, d)
        cases.append(_case("rows d %d" % d, f))
    return cases


RING_DISTANCES = (64, 65, 127, 128)


def chains_ring(layout):
    lay, step, cases = LAYOUTS[layout], step_bytes(layout), []
    for d in RING_DISTANCES:
        f = Fragment(layout, 2300 + 10 * layout + d % 10 + d // 100)
        f.field_lits(d).field_copies_to(4 * step, d)
        cases.append(_case("ring d %d" % d, f))
    f = Fragment(layout, 2350 + layout).lits_to(2 * step + 32)
    f.copy(lay.block, f.made)                                           # the fragment's first block, from two steps on
    f.lits_to(FRAG - lay.block)
    f.copy(lay.block, f.made)                                           # ... and from its last block
    cases.append(_case("offset equals position", f))
    return cases


def literal_spans(layout):
    """{n: [starts]}: where in a half-tile a literal of n bytes lies between two field boundaries"""
    spans = collections.OrderedDict()
    for n in range(1, HALF + 1):
        starts = [s for s in range(0, HALF - n + 1) if on_field(layout, s) and on_field(layout, s + n)]
        if starts:
            spans[n] = starts
    return spans


def copy_lengths(layout, lengths):
    return [n for n in lengths if any(on_field(layout, s) and on_field(layout, s + n) for s in range(LAYOUTS[layout].block))]


COPY1_LENGTHS = tuple(range(4, 12))
COPY2_LENGTHS = (1, 2, 4, 6, 64)


def forms(layout):
    """Literals of every length a layout's field boundaries allow, 1..60 in the tag and 1..128 with a length byte, at the
    start, the middle and the end of a half-tile; copy-1 and copy-2 at the edges of their lengths and offsets"""
    lay, cases = LAYOUTS[layout], []
    halves = []                                                         # (start, n, length bytes)
    for n, starts in literal_spans(layout).items():
        for length_bytes in ((0, 1) if n <= 60 else (1,)):
            for s in sorted({starts[0], starts[len(starts) // 2], starts[-1]}):
                halves.append((s, n, length_bytes))
    for at in range(0, len(halves), 56):
        f = Fragment(layout, 3000 + 100 * layout + at // 56)
        for s, n, length_bytes in halves[at: at + 56]:
            base = f.made
            f.lits_to(base + s).lit(n, length_bytes).lits_to(base + HALF)
        cases.append(_case("literal forms %d" % (at // 56), f))
    # copies: 2048 + block bytes of literals in front, so that every offset has its source
    top1 = (2047 // lay.block) * lay.block
    f = Fragment(layout, 3900 + layout).lits_to(2048 + lay.block)

    def put(n, off, form):
        s = next(s for s in range(lay.block) if on_field(layout, s) and on_field(layout, s + n))
        p = f.made
        q = p - p % lay.block + s
        q = q if q >= p else q + lay.block
        if q // HALF != (q + n - 1) // HALF:
            q = (q // HALF + 1) * HALF + s
        f.lits_to(q).copy(n, off, form)
    for n in copy_lengths(layout, COPY1_LENGTHS):
        for off in (lay.block, 2 * lay.block, top1 - lay.block, top1):
            put(n, off, "copy1")
    for n in copy_lengths(layout, COPY2_LENGTHS):
        for off in (lay.block, 2048):
            put(n, off, "copy2")
    f.lits_to(f.made - f.made % HALF + HALF + 64).copy(64, 2048, "copy2")   # the longest that ends with its half-tile
    # offset out_len - block: only the fragment's last block can hold it, a copy per field
    f.lits_to(FRAG - 64)
    f.copy(64 - lay.block, FRAG - 64, "copy2")                              # reaches the fragment's first byte
    for _fp, fn in lay.fields:
        f.copy(fn, FRAG - lay.block, "copy2")
    cases.append(_case("copy forms", f))
    return cases


SPLITS = 32


def element_splits(layout):
    """Seeded random conformant fragments: the output cut at random field boundaries, each element a literal or a copy
    of a random whole-block distance inside the fragment; from a handful of elements to one per field"""
    lay, cases = LAYOUTS[layout], []
    for i in range(SPLITS):
        for attempt in range(50):
            rng = np.random.default_rng([4000 + layout, i, attempt])
            out_len = FRAG if i % 4 else int(rng.integers(1, FRAG // lay.block + 1)) * lay.block
            starts = field_starts(layout, out_len)
            density = (i + 1) / SPLITS
            cuts = set(range(0, out_len, HALF)) | {p for p in starts if rng.random() < density}
            if i == SPLITS - 1:
                cuts = set(starts)
            cuts = sorted(cuts)
            # a copy holds 64 bytes: longer spans become two elements
            cuts = sorted(set(cuts) | {p + 64 for p, q in zip(cuts, cuts[1:] + [out_len]) if q - p > 64})
            draws = rng.random((len(cuts), 3))
            p_lit = 0.15 + 0.5 * float(rng.random())

            def kind(j, p, n, draws=draws, p_lit=p_lit):
                near = p // lay.block
                if near == 0 or draws[j, 0] < p_lit:
                    return ("lit", 1 if n > 60 or draws[j, 1] < 0.2 else None)
                return ("copy", 1 + int(draws[j, 2] * near))
            f = from_cuts(layout, 4100 + 50 * i + attempt, out_len, cuts, kind)
            if conforms(f.stream(), layout, out_len) is None and all(room_ok(f, s) for s in SOURCE_ALIGNMENTS):
                break
        else:
            raise AssertionError("no conformant split for seed %d" % i)
        cases.append(_case("split %d" % i, f))
    return cases


COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 1024, FRAG // 4)


def counts(layout):
    cases = []
    for n in COUNTS:
        out_len = FRAG if n >= 64 else n * HALF
        f = from_cuts(layout, 5000 + layout, out_len, spread_cuts(layout, out_len, n), _mixed_kind(LAYOUTS[layout], n))
        assert len(f.parts) == n
        cases.append(_case("count %d" % n, f))
    return cases


def short_lengths(layout):
    block, step = LAYOUTS[layout].block, step_bytes(layout)
    return (block, 2 * block, HALF - block, HALF, HALF + block, step - block, step + block, FRAG - block)


@functools.lru_cache(None)
def filler(layout, which):
    return mixed(layout, 5500 + 10 * layout + which, FRAG, 409 + 92 * which)


def short_fragments(layout):
    cases = []
    for out_len in short_lengths(layout):
        for fragments in (1, 3):
            cases.append(_case("short %d of %d" % (out_len, fragments), mixed(layout, 5600 + out_len + fragments, out_len), fragments))
    return cases


RECORDS_TOTAL = 4608               # compressed bytes of every fragment of the ladder
RECORDS_LADDER = tuple(range(1180, 1193))


def records(layout):
    cases = []
    for n in RECORDS_LADDER:
        lay = LAYOUTS[layout]
        cuts = spread_cuts(layout, FRAG, n)
        lens = [(cuts[i + 1] if i + 1 < n else FRAG) - p for i, p in enumerate(cuts)]
        lits = {i for i, p in enumerate(cuts) if p < lay.block}
        cost = lambda i: 2 if 4 <= lens[i] <= 11 else 3              # noqa: E731  (copy-1 / copy-2: every offset is below 2048)
        size = sum(lens[i] + 1 if i in lits else cost(i) for i in range(n))
        for i in sorted(range(n), key=lambda i: (i * 389) % n):
            if i not in lits and size + lens[i] + 1 - cost(i) <= RECORDS_TOTAL:
                lits.add(i)
                size += lens[i] + 1 - cost(i)
        padded = set(sorted(lits)[: RECORDS_TOTAL - size])
        assert len(padded) == RECORDS_TOTAL - size, (n, size)
        f = from_cuts(layout, 6000 + layout, FRAG, cuts,
                      lambda i, p, m: ("lit", 1 if i in padded else None) if i in lits else ("copy", 1 + i % min(p // lay.block, 5)))
        assert f.total == RECORDS_TOTAL and len(f.parts) == n, (f.total, len(f.parts))
        cases.append(_case("records %d" % n, f))
    f = Fragment(layout, 6100 + layout).field_lits().field_copies_to(FRAG, 1)
    cases.append(_case("all copies, an element per field", f))
    f = Fragment(layout, 6110 + layout).field_lits(5)
    while f.made < FRAG:
        for j, (_fp, fn) in enumerate(LAYOUTS[layout].fields):
            f.copy(fn, (1 + (f.made // 16 + j) % 5) * LAYOUTS[layout].block)
    cases.append(_case("all copies at five distances", f))
    return cases


ROOM_SPARSE = (8, 11, 15)          # half-tiles of two copies in front of the dense ones


def room(layout):
    """Input-sparse half-tiles, then input-dense ones: the parked input's last rows lie close to the output of the
    first steps.  On a limit the public header does not state: bytes only."""
    lay, cases = LAYOUTS[layout], []
    for sparse in ROOM_SPARSE:
        for dense in ("blocks", "fields"):
            f = Fragment(layout, 7000 + 100 * layout + sparse).lit(lay.block)
            f.copy(64, lay.block, "copy2").copy(HALF - 64 - lay.block, lay.block, "copy2")
            for _ in range(sparse):
                f.copy(64, HALF, "copy2").copy(64, HALF, "copy2")
            while f.made < FRAG:
                rest = FRAG - f.made - lay.block
                if dense == "fields" and f.total + lay.block + len(lay.fields) + rest + rest // lay.block <= MAX_COMPRESSED:
                    f.field_lits()
                else:
                    f.lit(lay.block)
            if f.total <= MAX_COMPRESSED:
                cases.append(_case("room: %d sparse half-tiles, then literal %s" % (sparse, dense), f))
    return cases


def alignment(layout):
    """One compact mixed fragment for every source address; a chunk of fragments of different compressed sizes (its
    case is the third); the frame ends with its last fragment"""
    return [_case("alignment", mixed(layout, 8000 + layout, FRAG, 400)),
            _case("alignment, third of a chunk", mixed(layout, 8010 + layout, FRAG - 3 * LAYOUTS[layout].block, 777), 3)]


FAMILIES = collections.OrderedDict([
    ("chains", chains), ("chains, mixed", chains_mixed), ("chains, long", chains_long), ("chains, rows", chains_rows),
    ("chains, ring", chains_ring), ("forms", forms), ("element splits", element_splits), ("counts", counts),
    ("short fragments", short_fragments), ("records", records), ("room", room), ("alignment", alignment)])
BYTES_ONLY = ("room",)


@functools.lru_cache(None)
def family(name, layout):
    return tuple(FAMILIES[name](layout))


def chunk_of(case):
    """The fragments of the case's chunk: fillers of different compressed sizes in front of a third one"""
    return [case.frag] if case.fragments == 1 else [filler(case.layout, 0), filler(case.layout, 1), case.frag]


# ---------------------------------------------------------------------------------------------------------- lies --
Lie = collections.namedtuple("Lie", "name layout chunk tables promise")   # tables: {fragment of the chunk: its table}


def _halves(layout, seed):
    """An honest fragment as 64 half-tiles of elements each, so that a twin can replace one"""
    lay = LAYOUTS[layout]
    halves = []
    for h in range(64):
        f = Fragment(layout, seed + h)
        f.out += bytes(HALF * h)                                       # (positions only: the twins are built again below)
        if h == 0:
            f.lits_to(HALF * h + 96, 48).copy(16, 96).lits_to(HALF * h + 120).copy(8, lay.block)
        else:
            f.copy(64, HALF, "copy2").lits_to(HALF * h + 64 + lay.block).copy(HALF - 64 - lay.block, lay.block * (1 + h % 4), "copy2")
        halves.append(f.parts)
    return halves


def _replay(layout, seed, element_lists, before=b""):
    """A fragment from ready elements: the output is the plain decoder's"""
    f = Fragment(layout, seed, before)
    f.parts = [e for els in element_lists for e in els]
    f.total = sum(len(e) for e in f.parts)
    stream = f.stream()
    made = sum(element_lengths(e)[1] for e in f.parts)
    whole = S.decode(S.varint(len(before) + made) + (S.lit(before, 4) if before else b"") + stream)
    f.out = bytearray(whole[len(before):])
    return f


@functools.lru_cache(None)
def honest_twin(layout):
    return _replay(layout, 9000 + layout, _halves(layout, 9000 + 100 * layout))


@functools.lru_cache(None)
def lies(layout):
    lay = LAYOUTS[layout]
    base = _halves(layout, 9000 + 100 * layout)
    block = lay.block
    found = []

    def twin(name, promise, h, els, fragments=1):
        v = list(base)
        v[h] = els
        if fragments == 1:
            found.append(Lie("%d: %s" % (layout, name), layout, [_replay(layout, 9100, v)], {}, promise))
        else:
            first = honest_twin(layout)
            found.append(Lie("%d: %s" % (layout, name), layout, [first, _replay(layout, 9100, v, first.out)], {}, promise))

    def half(h, build):
        f = Fragment(layout, 9200 + h, before=bytes(block))
        f.out += bytes(HALF * h)
        build(f)
        f.lits_to(HALF * (h + 1))
        return f.parts
    twin("offset not a whole block", "copy offset", 5, half(5, lambda f: f.copy(64, HALF + lay.fields[1][0], "copy2")))
    if layout in (4, 6):
        twin("start on an even byte that is no field start", "field boundary", 6,
             half(6, lambda f: f.copy(62, HALF, "copy2").lit(4)))
        twin("start on an odd byte", "field boundary", 7, half(7, lambda f: f.copy(63, HALF, "copy2").lit(3)))
    else:
        twin("start off a multiple of four", "field boundary", 7, half(7, lambda f: f.copy(62, HALF, "copy2").lit(2)))
    # an element across the end of half-tile 10: the sizes in the table still add up
    v = list(base)
    f = Fragment(layout, 9300)
    f.out += bytes(HALF * 10)
    f.lits_to(HALF * 10 + HALF - 2 * block).copy(4 * block, 3 * block, "copy2").lits_to(HALF * 12)
    v[10], v[11] = f.parts, []
    found.append(Lie("%d: element across a half-tile" % layout, layout, [_replay(layout, 9100, v)], {}, "half-tile"))
    twin("copy-4", "copy-4", 8, half(8, lambda f: f.copy(64, HALF, "copy4")))
    twin("literal with a two-byte length", "literal length", 9, half(9, lambda f: f.lit(64, 2)))
    twin("copy from one block before the fragment", "copy offset", 3,
         half(3, lambda f: f.copy(64, HALF, "copy2").copy(block, HALF * 3 + 64 + block, "copy2")), fragments=2)
    # table lies: the stream is the honest one
    honest = honest_twin(layout)
    sizes, made, n = unpack_groups(group_table(honest.parts))

    def table_lie(name, table):
        assert table != group_table(honest.parts)
        found.append(Lie("%d: table, %s" % (layout, name), layout, [honest], {0: table}, None))
    for wrong in (n - 1, n + 1, n + 64):
        table_lie("N %+d" % (wrong - n), pack_groups(sizes, made, wrong))
    k = 5
    first = element_lengths(honest.parts[k * ((n + 63) // 64)])           # the first element of group k
    moved = list(sizes)
    moved[k - 1] += first[0]
    moved[k] -= first[0]
    table_lie("a boundary moved between two groups' compressed bytes", pack_groups(moved, made, n))
    moved = list(made)
    moved[k - 1] += first[1]
    moved[k] -= first[1]
    table_lie("a boundary moved between two groups' output bytes", pack_groups(sizes, moved, n))
    off = list(sizes)
    off[k] += 3
    table_lie("sums that do not add up", pack_groups(off, made, n))
    table_lie("all zero", bytes(GT))
    return tuple(found)


# -------------------------------------------------------------------------------------------------------- frames --
def section(kind, body):
    n = len(body)
    if n < 1 << 24:
        return n.to_bytes(3, "little") + bytes([kind]) + body
    return bytes([0, 0, 0, kind]) + n.to_bytes(4, "little") + body


def texture_section(chunks, layout, fmt, table=True, tables=None):
    """One texture's section: every chunk a list of fragments, the same number P in each; its length prefix lies in
    ((P - 1) x 8192, P x 8192].  Header of section 0x46: [4][13][granularity | layout << 4][0], then the LE32 fragment
    sizes, then the group tables.  table=False: every fragment a chunk of its own, no private section."""
    lay = LAYOUTS[layout]
    assert fmt in lay.formats
    if not table:
        chunks = [[f] for c in chunks for f in c]
    per = len(chunks[0])
    streams = []
    for c in chunks:
        total = sum(f.made for f in c)
        assert len(c) == per and all(f.made == FRAG for f in c[:-1]) and (per - 1) * FRAG < total <= per * FRAG
        streams.append(S.varint(total) + b"".join(f.stream() for f in c))
    n = len(streams)
    secs = section(2, bytes([0x0B]) * n) + section(3, b"".join(len(s).to_bytes(4, "little") for s in streams))
    if table:
        frags = [f for c in chunks for f in c]
        tables = tables or {}
        secs += section(0x46, bytes([4, 13, lay.gran | layout << 4, 0]) + b"".join(f.total.to_bytes(4, "little") for f in frags) +
                        b"".join(tables.get(i) or group_table(f.parts) for i, f in enumerate(frags)))
    return section(0xC0 | FORMAT_NIBBLE[fmt], section(1, secs) + b"".join(streams))


def frame_of_fragments(chunks, layout, fmt, table=True, tables=None):
    """A whole Hap frame of one texture.  Returns (frame, the bytes it decodes to)."""
    return texture_section(chunks, layout, fmt, table, tables), b"".join(bytes(f.out) for c in chunks for f in c)


def frame_of_two_textures(chunks4, chunks6, table=True):
    """One Hap Q Alpha frame: a YCoCg-DXT5 texture (layout 4) and an RGTC1 one (layout 6).  Returns (frame, [bytes, bytes])"""
    frame = section(0x0D, texture_section(chunks4, 4, FMT_YCOCG, table) + texture_section(chunks6, 6, FMT_RGTC1, table))
    return frame, [b"".join(bytes(f.out) for c in chunks for f in c) for chunks in (chunks4, chunks6)]


# --------------------------------------------------------------------------------------------------- description --
def _walk(frag):
    p = 0
    for el in S.elements(S.varint(frag.made) + frag.stream()):
        yield p, el
        p += el.n


@functools.lru_cache(None)
def describe(layout):
    """What the families of a layout hold, read back from the built bytes"""
    lay = LAYOUTS[layout]
    field_at = {fp: k for k, (fp, _n) in enumerate(lay.fields)}
    d = {"chain distances": collections.defaultdict(set), "literals": collections.defaultdict(set),
         "literal places": collections.defaultdict(set), "copy1": set(), "copy2": set()}
    for case in family("chains", layout):
        for p, el in _walk(case.frag):
            if el.form.startswith("copy"):
                assert el.n == lay.fields[field_at[p % lay.block]][1]
                d["chain distances"][field_at[p % lay.block]].add(el.off // lay.block)
    for case in family("forms", layout):
        for p, el in _walk(case.frag):
            if el.form.startswith("lit"):
                d["literals"][el.form].add(el.n)
                where = {"start"} if p % HALF == 0 else set()
                where |= {"end"} if (p + el.n) % HALF == 0 else set()
                d["literal places"][(el.form, el.n)] |= where or {"middle"}
            else:
                d[el.form].add((el.n, el.off))
    for name in ("chains, mixed", "chains, long", "chains, rows", "chains, ring"):
        d[name] = sorted({el.off // lay.block for case in family(name, layout) for _p, el in _walk(case.frag) if el.form.startswith("copy")})
    d["counts"] = [len(case.frag.parts) for case in family("counts", layout)]
    d["short lengths"] = sorted({case.frag.made for case in family("short fragments", layout)})
    d["short chunks"] = sorted({case.fragments for case in family("short fragments", layout)})
    d["splits"] = len(family("element splits", layout))
    d["records"] = [(len(case.frag.parts), case.frag.total) for case in family("records", layout)]
    d["honest fragments"] = sum(len(family(name, layout)) for name in FAMILIES)
    d["lies"] = len(lies(layout))
    d["source alignments"] = list(SOURCE_ALIGNMENTS)
    d["output offsets"] = list(OUTPUT_OFFSETS)
    return d

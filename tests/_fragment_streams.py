"""Hand-built Snappy fragments for the table-driven fragment decoders (snappy_decode_fragment_kernel<RING, false, GRAN,
SLIDE>, hap_amd/csrc/snappy_decode.hip), the frames that carry them under a version-1 fragment table (section 0x46 of
include/hap_gpu.h: [1][log2 F][granularity log2][window / 256][LE32 size x fragments]) and a scalar model of how the
kernel walks a fragment.

A fragment is ordinary Snappy -- the element writers and the plain decoder are tests/_snappy_streams.py's -- that keeps
what its table announces: every length and every copy offset a multiple of the granularity (1, 2 or 4 bytes), no copy
from before the fragment, no element across its end, and, where the table says so, no offset above 3072.  Everything
else the grammar allows must decode: literals with up to four length bytes, over-long length forms, copy-4.  No GPU, no
ctypes: tests/test_fragment_streams.py holds every case to the plain decoder, to the checker libraries and to what its
family is meant to hold; tests/test_fragment_streams_gpu.py runs them through the kernels.

The pass model (passes(), coordinates(), staging(), chain_depths()) decides no byte.  It restates, from the kernel's text, how a
fragment is walked, so that what a family reaches can be asserted from the built bytes:

  coordinates  the kernel counts input from the 16-byte line of the fragment's first byte: coordinate = (address & 15) +
               stream position.  The staged input is a ring of two granules of 512 coordinates; granule g lies in half
               g & 1.  Granules 0 and 1 are staged at the start.
  staging      at the top of every pass, when ip + 384 > in_hi (the first coordinate not staged) and the input goes
               on: with g = ip / 512, granule next_g is stored when g + 1 == next_g ("advance"), and granules g and
               g + 1 are staged anew when g >= next_g ("restage": a serial literal jumped over whole granules).
  window pass  the 64 lanes parse the elements that would begin at ip .. ip + 63.  The pass takes the chain of elements
               from ip that begin there; it stops before a literal with 2 to 4 length bytes and before an element that
               does not fit the input.  Of these it keeps the elements with o_t + len <= 512 (o_t: output of the pass in
               front of the element).  N is their output, adv the input they span.
  serial pass  the element at ip is a literal with 2 to 4 length bytes: it is taken alone, 64 bytes a step; a step is
               read from the staged ring when it ends at or below in_hi, else from memory.
  production   a window pass produces its N / GRAN units 64 to a step.  A unit of a copy whose source unit lies in the
               same step waits for it; pointer jumping resolves a wait of depth d in bit_length(d) rounds.  Overlapping
               copies (offset < length) take source r = rel mod offset in front of the element: no unit of a copy waits
               for a unit of the same copy.

The deepest chain: a unit waits only for a unit of an earlier copy of the same pass, and the first copy of a pass that
heads a chain has its source in front of the step.  No element is shorter than two stream bytes, so at most 32 begin in a
window: depth 31 at the most (32 copy-1 of one unit each: GRAN 4, or of two units at offset one unit: GRAN 2), which
five rounds resolve.  With single bytes (GRAN 1) copy-1 spends four lanes and copy-2 three stream bytes: 14 copy-2 and
12 copy-1 make 26 copies in 62 lanes, depth 25.  Rounds six and seven of the kernel's loop are out of reach of any
stream; DEEPEST states the depths the chains family has to reach.

Lane 1 of a window is out of reach as well: the pass begins with an element, and none is one byte long.
"""
import collections
import functools

import numpy as np

import _snappy_streams as S
from _field_streams import FORMAT_NIBBLE, section

GRANS = (1, 2, 4)
GRAN_LOG2 = {1: 0, 2: 1, 4: 2}
FRAG_LOG2S = (10, 13, 14, 15, 16)
FMT_DXT5 = 0x83F3
WINDOW_BYTE = 12                   # HAP_FRAGMENT_WINDOW_256
WINDOW_REACH = 3072                # RING - 1024 of the windowed kernels
SLIDE_RING = 4096
FLUSH = 1024                       # the windowed ring gives output back in pieces of this size
GRANULE = 512                      # kV2InGranule
LOOKAHEAD = 384
OWNER = 512                        # kOwnerBytes: output of a window pass at the most
STEP = 64
LANES = tuple(lane for lane in range(64) if lane != 1)
DEEPEST = {1: 25, 2: 31, 4: 31}
SPECIAL = ("lit2", "lit3", "lit4")
V3_GROUP_TABLE = 96


# ----------------------------------------------------------------------------------------------- the pass model --
def bare_elements(stream):
    """The elements of a fragment's bare stream, positions from its first byte"""
    return [e._replace(pos=e.pos - 1) for e in S.elements(b"\0" + bytes(stream))]


Pass = collections.namedtuple("Pass", "kind ip first count adv N seen out stop")
# first, count: the elements taken; seen: output of the chain before the cut at 512; out: output in front of the pass;
# stop: lane of the element the chain stopped before (None: the window's end or the input's)


def passes(stream):
    els = bare_elements(stream)
    i = out = 0
    found = []
    while i < len(els):
        e = els[i]
        if e.form in SPECIAL:
            found.append(Pass("serial", e.pos, i, 1, e.hdr + e.n, e.n, e.n, out, None))
            i, out = i + 1, out + e.n
            continue
        j, seen = i, 0
        while j < len(els) and els[j].pos - e.pos < 64 and els[j].form not in SPECIAL:
            seen += els[j].n
            j += 1
        stop = els[j].pos - e.pos if j < len(els) and els[j].pos - e.pos < 64 else None
        k, n = i, 0
        while k < j and n + els[k].n <= OWNER:
            n += els[k].n
            k += 1
        if k < j:
            stop = els[k].pos - e.pos
        last = els[k - 1]
        size = last.hdr + (last.n if last.form.startswith("lit") else 0)
        found.append(Pass("window", e.pos, i, k - i, last.pos + size - e.pos, n, seen, out, stop))
        i, out = k, out + n
    return found


def staging(stream, phase):
    """[(pass, what the staging did at its top: None / "advance" / "restage", 64-byte steps of a serial literal read
    from memory)] for a fragment whose first byte lies at `phase` of its 16-byte line"""
    els = bare_elements(stream)
    in_end = phase + len(stream)
    granules = -(-in_end // GRANULE)
    next_g, in_hi = 2, 2 * GRANULE
    found = []
    for p in passes(stream):
        ip, event = phase + p.ip, None
        assert ip >= in_hi - 2 * GRANULE
        if ip + LOOKAHEAD > in_hi and in_hi < granules * GRANULE:
            g = ip // GRANULE
            if g + 1 == next_g:
                next_g, event = next_g + 1, "advance"
            elif g >= next_g:
                next_g, event = g + 2, "restage"
            in_hi = next_g * GRANULE
        # what a window pass reads (a 256-byte literal with its two header bytes at lane 63) is staged or past the input
        assert ip + LOOKAHEAD <= in_hi or in_hi >= in_end
        memory = 0
        if p.kind == "serial":
            e = els[p.first]
            at = ip + e.hdr
            memory = sum(1 for done in range(0, e.n, STEP) if at + done + min(STEP, e.n - done) > in_hi)
        found.append((p, event, memory))
    return found


def coordinates(stream, phase):
    """(element, staging coordinate of its tag, granule boundaries its header lies across) for a fragment whose first
    byte lies at `phase` of its 16-byte line"""
    for e in bare_elements(stream):
        at = phase + e.pos
        yield e, at, [k * GRANULE for k in range(at // GRANULE + 1, (at + e.hdr - 1) // GRANULE + 1)]


def chain_depths(stream, gran):
    """Per window pass, the depth of the deepest wait of a unit for units of its own 64-unit step"""
    els = bare_elements(stream)
    found = []
    for p in passes(stream):
        if p.kind != "window":
            continue
        depth, o_t = {}, 0
        for e in els[p.first: p.first + p.count]:
            first, elen = o_t // gran, e.n // gran
            for rel in range(elen):
                b = first + rel
                if e.form.startswith("lit"):
                    depth[b] = 0
                    continue
                offu = min(e.off, 127) // gran
                r = rel % offu if offu < elen else rel
                q = (o_t - e.off) // gran + r
                depth[b] = 0 if q < b - b % STEP else 1 + depth[q]
            o_t += e.n
        found.append(max(depth.values()))
    return found


# ----------------------------------------------------------------------------------------------- the builder --
class Fragment:
    """The bare elements of one fragment, the bytes they make, and a name.  before: the output in front of the fragment
    in its chunk, for the lies that reach into it.  claims: the output the chunk's length prefix counts for it."""

    def __init__(self, gran, seed, name="", before=b""):
        self.gran = gran
        self.name = name
        self.rng = np.random.default_rng(seed)
        self.before = bytes(before)
        self.parts = []
        self.out = bytearray()
        self.total = 0
        self.claims = None

    @property
    def made(self):
        return len(self.out)

    def stream(self):
        return b"".join(self.parts)

    def mark(self):
        return len(self.parts), len(self.out), self.total

    def back_to(self, mark):
        del self.parts[mark[0]:]
        del self.out[mark[1]:]
        self.total = mark[2]

    def _add(self, part):
        self.parts.append(part)
        self.total += len(part)

    def lit(self, n, length_bytes=None, data=None):
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes() if data is None else bytes(data)
        self._add(S.lit(data, length_bytes))
        self.out += data
        return self

    def head(self, n=64):
        """A literal of n <= 256 different bytes: nothing in it repeats at any period"""
        assert 1 <= n <= 256
        return self.lit(n, data=self.rng.permutation(256)[:n].astype(np.uint8).tobytes())

    def copy(self, form, n, off):
        self._add(S.COPY_WRITERS[form](n, off))
        made = self.made
        if off == 0:
            self.out += bytes(n)                                        # (invalid: nobody's output)
        elif off > made:
            src = self.before + bytes(self.out)
            assert off <= len(src) and off >= n
            self.out += src[len(src) - off: len(src) - off + n]
        elif off >= n:
            self.out += self.out[made - off: made - off + n]
        else:
            self.out += (bytes(self.out[made - off:]) * (n // off + 1))[:n]
        return self

    def opener(self):
        """A literal of two units with two length bytes: the serial path takes it alone, and the pass behind it begins
        with the element behind it"""
        return self.lit(2 * self.gran, 2)

    def advance(self, d):
        """Elements of exactly d stream bytes (none is one byte long): literals of 60, then copies of 2 and 3"""
        assert d == 0 or d >= 2, d
        while d > 64:
            self.lit(60)
            d -= 61
        if d % 2:
            self.copy("copy2", self.gran, 4 * self.gran)
            d -= 3
        for i in range(d // 2):
            self.copy("copy1", 4, 4 + 4 * (i % 8))
        return self

    def advance_to(self, at):
        if at - self.total == 1:
            raise AssertionError("no element is one byte long")
        return self.advance(at - self.total)

    def pad(self, total):
        """Literals up to `total` output bytes"""
        assert self.made <= total and (total - self.made) % self.gran == 0, (self.name, self.made, total)
        while self.made < total:
            self.lit(min(256, total - self.made))
        return self

    def tail(self):
        """Short elements that depend on the bytes staged behind what was just put"""
        return self.lit(8).copy("copy2", 8, 8).copy("copy1", 4, 12)


def mixed(gran, size, seed, name="mixed"):
    """An ordinary fragment of `size` bytes: short literals in all their forms, copies in the three forms near and far"""
    f = Fragment(gran, seed, name)
    f.head(min(64, size))
    rng = np.random.default_rng(seed + 77)
    while size - f.made >= 80:
        what = int(rng.integers(0, 6))
        n = gran * int(rng.integers(1, 64 // gran + 1))
        if what == 0:
            f.lit(n, int(rng.integers(0, 3)) if n <= 60 else int(rng.integers(1, 3)))
        elif what == 1 and 4 <= n <= 11:
            f.copy("copy1", n, gran * int(rng.integers(1, min(f.made, 2047) // gran + 1)))
        else:
            off = gran * int(rng.integers(1, min(f.made, WINDOW_REACH) // gran + 1))
            f.copy("copy4" if what == 2 else "copy2", n, off)
    return f.pad(size)


class Pack:
    """Cases back to back in fragments of one size.  A case is a function that appends to the fragment it is given; one
    that does not fit begins the next fragment."""

    def __init__(self, gran, frag_log2, family, seed):
        self.gran, self.size, self.family, self.seed = gran, 1 << frag_log2, family, seed
        self.done = []
        self.f = None

    def _new(self):
        self.f = Fragment(self.gran, self.seed + len(self.done), "%s %d, GRAN %d" % (self.family, len(self.done), self.gran))

    def add(self, case):
        if self.f is None:
            self._new()
        mark = self.f.mark()
        case(self.f)
        if self.f.made > self.size:
            assert mark[1] > 0, "a case larger than a fragment"
            self.f.back_to(mark)
            self.close()
            self._new()
            case(self.f)
            assert self.f.made <= self.size

    def close(self):
        if self.f is not None:
            self.done.append(self.f.pad(self.size))
            self.f = None

    def fragments(self):
        self.close()
        return self.done


# ---------------------------------------------------------------------------------------------------- families --
def overlap_offsets(gran):
    return [o for o in list(range(gran, 67)) + [126, 127, 128, 129] if o % gran == 0]


def overlap_cases(gran):
    """(form, length, offset): every pair a copy can carry at multiples of GRAN, in every form that holds it"""
    cases = []
    for off in overlap_offsets(gran):
        for n in range(gran, 65, gran):
            cases += [("copy2", n, off), ("copy4", n, off)] + ([("copy1", n, off)] if 4 <= n <= 11 else [])
    return cases


def overlap(gran):
    """A literal of `off` different bytes, then the copy in each of its forms: each continues the period"""
    pack = Pack(gran, 13, "overlap", 1000 * gran)
    for off in overlap_offsets(gran):
        for n in range(gran, 65, gran):
            def case(f, n=n, off=off):
                f.head(off)
                f.copy("copy2", n, off).copy("copy4", n, off)
                if 4 <= n <= 11:
                    f.copy("copy1", n, off)
            pack.add(case)
    return pack.fragments()


def form_list(gran):
    """(name, form, output bytes, length bytes or offset): literals around 60 / 61 and 256 / 257 and the over-long forms
    of short ones; the three copies, copy-4 with small offsets too"""
    g = gran
    return [("lit0 short", "lit0", g, 0), ("lit0 60", "lit0", 60, 0),
            ("lit1 over-long short", "lit1", g, 1), ("lit1 over-long 60", "lit1", 60, 1), ("lit1 61", "lit1", 60 + g, 1),
            ("lit1 256", "lit1", 256, 1),
            ("lit2 over-long short", "lit2", g, 2), ("lit2 over-long 256", "lit2", 256, 2), ("lit2 257", "lit2", 256 + g, 2),
            ("lit3 over-long short", "lit3", g, 3), ("lit3 over-long 257", "lit3", 256 + g, 3),
            ("lit4 over-long short", "lit4", g, 4), ("lit4 over-long 61", "lit4", 60 + g, 4),
            ("copy1 short", "copy1", 4, 40), ("copy1 long", "copy1", 8 + 3 * (g == 1) + 2 * (g == 2), 2044),
            ("copy2 short", "copy2", g, 2048), ("copy2 long", "copy2", 64, 64), ("copy2 overlapping", "copy2", 64, 3 * g),
            ("copy4 small offset", "copy4", 64, g), ("copy4 short", "copy4", g, 64), ("copy4 far", "copy4", 60, 2100)]


def put_form(f, spec):
    _name, form, n, arg = spec
    if form.startswith("lit"):
        f.lit(n, arg)
    else:
        f.copy(form, n, arg)


def forms(gran):
    """Every form with its tag at every lane of a window: 48 different bytes, a serial literal, `lane` stream bytes of
    two- and three-byte copies of them, the form, a copy behind it.  2200 bytes in front of a fragment's first case: the
    far offsets have their sources."""
    pack = Pack(gran, 13, "forms", 2000 * gran)
    for spec in form_list(gran):
        for lane in LANES:
            def case(f, spec=spec, lane=lane):
                if f.made == 0:
                    f.head(64).pad(2200)
                f.head(48).opener().advance(lane)
                put_form(f, spec)
                f.copy("copy1", 4, 4)
            pack.add(case)
    return pack.fragments()


HEADER_FORMS = (("lit1", 2), ("lit2", 3), ("lit3", 4), ("lit4", 5), ("copy1", 2), ("copy2", 3), ("copy4", 5))
SERIAL_ENDS = (-1, 0, 1)
SKIPS = (1100, 1700, 2600)         # serial literals: longer than the staged ring; over two and over four whole granules


def staging_splits():
    """(form, header bytes in front of the granule boundary, boundary parity): odd boundaries lie in the middle of the
    staged ring, even ones at its wrap"""
    return [(form, s, parity) for form, hdr in HEADER_FORMS for s in range(1, hdr) for parity in (1, 0)]


def _put_header_form(f, form):
    if form.startswith("lit"):
        f.lit(80 if form == "lit1" else 300, int(form[3]))
    else:
        f.copy(form, 8, 16)


def staging_fragments(gran):
    """Built for a fragment whose first byte is the first of its 16-byte line (phase 0): coordinates are stream
    positions.  Run at the sixteen source addresses, each fragment meets that phase once."""
    frags = []

    def new(name):
        f = Fragment(gran, 3000 * gran + len(frags), "staging %d, GRAN %d: %s" % (len(frags), gran, name))
        frags.append(f)
        return f.head(64)
    # header splits: one after the other at the next boundary of the wanted parity, 14 KiB of stream at the most
    f = new("header splits")
    for form, s, parity in staging_splits():
        k = (f.total + 8) // GRANULE + 1
        k += (k & 1) != parity
        if k * GRANULE > 6000:
            f.pad(8192)
            f = new("header splits")
            k = 2 - parity
        f.advance_to(k * GRANULE - s)
        _put_header_form(f, form)
        f.tail()
    f.pad(8192)
    # a serial literal that ends one byte before, on and one byte after a boundary of either parity
    f = new("serial literal ends")
    for parity in (1, 0):
        for extra in (2, 3, 4):
            for d in SERIAL_ENDS:
                k = (f.total + 320) // GRANULE + 1
                k += (k & 1) != parity
                if k * GRANULE > 6000:
                    f.pad(8192)
                    f = new("serial literal ends")
                    k = 2 - parity
                f.advance_to(k * GRANULE + d - 300 - 1 - extra)
                f.lit(300, extra).tail()
    f.pad(8192)
    # serial literals that leave the staged ring behind
    for n in SKIPS:
        for extra in (2, 3):
            f = new("serial literal of %d, %d length bytes" % (n, extra))
            f.lit(n, extra).tail().lit(8, 2).tail().pad(8192)
    return frags


def pass_totals(gran):
    return (OWNER - gran, OWNER, OWNER + gran, 21 * 64)


def passes_family(gran):
    """Windows whose elements make 512 - GRAN, 512, 512 + GRAN and 1344 bytes, as copies alone and with a 256-byte
    literal; 32 two-byte elements in a window"""
    pack = Pack(gran, 13, "passes", 4000 * gran)

    def copies(f, total):
        for _ in range(total // 64):
            f.copy("copy2", 64, 64)
        if total % 64:
            f.copy("copy2", total % 64, 64)
    for total in pass_totals(gran):
        def case(f, total=total):
            f.head(64).opener()
            copies(f, total)
            f.opener().lit(8).copy("copy1", 4, 4)
        pack.add(case)
    for total in pass_totals(gran)[:3]:
        def case(f, total=total):
            f.head(64).opener()
            copies(f, total - 256)
            f.lit(256, 1).copy("copy2", 64, 256).lit(8)
        pack.add(case)

    def thirty_two(f):
        f.head(64).opener()
        for i in range(32):
            f.copy("copy1", 4 if i % 2 else 8, 4 + 4 * (i % 13))
        f.lit(8)
    pack.add(thirty_two)
    return pack.fragments()


def deepest_chain(f):
    """The most copies of one unit's reach that begin in a window and whose output fits a step"""
    g = f.gran
    f.head(64).opener()
    if g == 1:
        order = ["copy2", "copy1"] * 12 + ["copy2", "copy2"]
        for form in order:
            f.copy(form, 4 if form == "copy1" else 1, 1)
    else:
        for _ in range(32):
            f.copy("copy1", 4, g if g == 2 else 4)
    f.lit(8)


def chains(gran):
    g = gran
    pack = Pack(gran, 13, "chains", 5000 * gran)
    pack.add(deepest_chain)
    for depth in range(1, 22):                           # a literal, then `depth` copies of the unit in front
        def case(f, depth=depth):
            f.head(64).opener().lit(g)
            for _ in range(depth):
                f.copy("copy2", g, g)
            f.lit(8)
        pack.add(case)
    for units in (8, 3):                                 # offsets equal to the length and below it, down to one unit
        def case(f, units=units):
            f.head(64).opener().lit(units * g)
            off = units
            while off >= 1:
                f.copy("copy2", units * g, off * g)
                off = off // 2 if off > 1 else 0
            f.lit(8)
        pack.add(case)

    def mix(f):                                          # literal to copy to copy, and copies that read two elements
        f.head(64).opener()
        for i in range(6):
            f.lit(2 * g).copy("copy2", 2 * g, 2 * g).copy("copy4", 4 * g, 3 * g).copy("copy2", 2 * g, 8 * g if i else 2 * g)
        f.lit(8)
    pack.add(mix)
    return pack.fragments()


def ring_fragment(gran, frag_log2):
    """A full fragment with copies whose offset is everything made so far: after the first 64 bytes, in the middle and
    for the last 64 bytes and the last unit; in 64 KiB that is the farthest copy-2 there is, and copy-4 go beyond 32767"""
    size = 1 << frag_log2
    f = Fragment(gran, 6000 * gran + frag_log2, "ring %d, GRAN %d" % (frag_log2, gran))
    f.head(64).copy("copy2", 64, 64).tail()
    f.pad(size // 2)
    f.copy("copy2" if f.made < 65536 else "copy4", 64, f.made).copy("copy4", 32, f.made).tail()
    if frag_log2 == 16:
        f.pad(40000)
        f.copy("copy4", 64, 32768).copy("copy4", 64, f.made).copy("copy4", 8, 40000 - 4 * gran).tail()
    f.pad(size - 64 - gran)
    return f.copy("copy2", 64, f.made).copy("copy2", gran, f.made)      # (in 64 KiB: the farthest copy-2 there is)


def rings(gran, frag_log2):
    return [ring_fragment(gran, frag_log2), mixed(gran, 1 << frag_log2, 6100 * gran + frag_log2, "ring %d filler" % frag_log2)]


def window(gran):
    """8 KiB fragments that keep the match window of 3072: through the 4 KiB ring that gives output back 1 KiB at a time"""
    g = gran
    frags = []
    f = Fragment(g, 7000 * g, "window: copies across the flush points, GRAN %d" % g)
    f.head(64)
    for k in range(1, 8):
        f.pad(FLUSH * k - 32)
        # (k = 4: the output lies across the ring's wrap; k = 7: the source does)
        f.copy("copy4" if k % 2 else "copy2", 64, min(WINDOW_REACH, f.made)).tail()
    frags.append(f.pad(8192))
    f = Fragment(g, 7000 * g + 1, "window: serial literals across the flush points, GRAN %d" % g)
    f.head(64)
    for k in range(1, 8):
        f.pad(FLUSH * k - 100)
        f.lit(200, 2 + k % 3).copy("copy2", 64, min(WINDOW_REACH, f.made - f.made % g)).tail()
    frags.append(f.pad(8192))
    f = Fragment(g, 7000 * g + 2, "window: passes of 512 bytes at offset 3072, GRAN %d" % g)
    f.head(64).pad(WINDOW_REACH)
    for _ in range(3):
        f.opener()
        for _ in range(8):
            f.copy("copy2", 64, WINDOW_REACH)
        f.lit(1100, 2)                                                            # the next pass lies elsewhere in the ring
    f.opener().copy("copy2", g, WINDOW_REACH).lit(60).copy("copy1", 4, 4).copy("copy4", g, WINDOW_REACH)
    frags.append(f.pad(8192))
    frags.append(mixed(g, 8192, 7000 * g + 3, "window: mixed, GRAN %d" % g))
    return frags


def small_fragment(gran, n, seed):
    f = Fragment(gran, seed, "last fragment of %d, GRAN %d" % (n, gran))
    if n < 16:
        return f.lit(n)
    half = (n // 2) - (n // 2) % gran
    return f.head(half).copy("copy2", n - half, half)


def end_sizes(gran, frag_log2=13):
    return (gran, 2 * gran, 60, 64, 68, (1 << frag_log2) - gran)


Frames = collections.namedtuple("Frames", "label frag_log2 chunks window_ok")


def ends(gran):
    """Frames of their own: ragged last fragments (a chunk each, the chunks of different compressed sizes), a fragment
    of one element, a chunk of one fragment, chunks of 65 and of 129 fragments of 1 KiB"""
    g = gran
    found = []
    chunks = []
    for i, n in enumerate(end_sizes(g)):
        last = small_fragment(g, n, 8200 * g + i) if n < 100 else mixed(g, n, 8000 * g + i, "last fragment of %d" % n)
        chunks.append([mixed(g, 8192, 8100 * g + i, "full fragment in front of %d" % n), last])
    found.append(Frames("ends: ragged last fragments, GRAN %d" % g, 13, chunks, True))
    one = Fragment(g, 8300 * g, "a single element, GRAN %d" % g).lit(1024, 2)
    found.append(Frames("ends: a fragment of one element, GRAN %d" % g, 10, [[one]], False))
    lone = Fragment(g, 8301 * g, "a single unit, GRAN %d" % g).lit(g)
    found.append(Frames("ends: a chunk of one unit, GRAN %d" % g, 13, [[lone]], True))
    for count in (65, 129):
        frags = [mixed(g, 1024, 8400 * g + 200 * (count == 129) + i, "%d of %d" % (i, count)) for i in range(count - 1)]
        frags.append(small_fragment(g, 64 + 4 * (count == 129), 8500 * g + count))
        found.append(Frames("ends: a chunk of %d fragments, GRAN %d" % (count, g), 10, [frags], False))
    return found


def chunks_of(frags):
    """Fragments of full size as chunks of four, two or one"""
    per = 4 if len(frags) % 4 == 0 else 2 if len(frags) % 2 == 0 else 1
    return [list(frags[i: i + per]) for i in range(0, len(frags), per)]


PACKED = collections.OrderedDict([("overlap", overlap), ("forms", forms), ("staging", staging_fragments),
                                  ("passes", passes_family), ("chains", chains), ("window", window)])
FAMILIES = tuple(PACKED) + ("rings", "ends")
PER_FRAME = 24                     # fragments of 8 KiB to a frame


@functools.lru_cache(None)
def fragments(family, gran):
    return tuple(PACKED[family](gran))


@functools.lru_cache(None)
def family_frames(family, gran):
    """The family's frames: (label, log2 of the fragment size, chunks, whether every offset stays within 3072)"""
    if family == "ends":
        return tuple(ends(gran))
    if family == "rings":
        return tuple(Frames("rings %d, GRAN %d" % (k, gran), k, chunks_of(rings(gran, k)), False) for k in FRAG_LOG2S)
    frags = fragments(family, gran)
    found = []
    for at in range(0, len(frags), PER_FRAME):
        part = frags[at: at + PER_FRAME]
        found.append(Frames("%s %d, GRAN %d" % (family, at // PER_FRAME, gran), 13, chunks_of(part),
                            all(max_offset(f.stream()) <= WINDOW_REACH for f in part)))
    return tuple(found)


def max_offset(stream):
    return max([e.off for e in bare_elements(stream) if e.form.startswith("copy")] or [0])


# ---------------------------------------------------------------------------------------------- the promises --
PROMISES = ("granularity", "window", "fragment start", "fragment end", "table", "snappy")


def broken(chunk, sizes, gran, windowed, frag_log2, total, cut=0):
    """The promises a chunk of fragments breaks, in the order of the first offence.  chunk: the bare streams; sizes:
    what the table says of them; total: the output the chunk's length prefix counts; cut: bytes the chunk lacks at its
    end.  Plain Python over the elements."""
    size = 1 << frag_log2
    found = []

    def note(what):
        if what not in found:
            found.append(what)
    whole = b"".join(bytes(s) for s in chunk)
    whole = whole[: len(whole) - cut]
    try:
        S.decode(S.varint(total) + whole)
        els = bare_elements(whole)
    except ValueError:
        note("snappy")
        els = []
    starts = {e.pos for e in els} | {len(whole)}
    if sum(sizes) != len(whole) or len(sizes) != len(chunk):
        note("table")
    at = made = i = 0
    first_out = 0
    bounds = []
    for s in sizes:
        bounds.append(at)
        at += s
    for e in els:
        while i < len(bounds) and bounds[i] <= e.pos:
            if bounds[i] != e.pos or bounds[i] not in starts:
                note("table")
            elif made != i * size:
                note("fragment end")
            first_out = i * size
            i += 1
        if e.n % gran or e.off % gran:
            note("granularity")
        if e.form.startswith("copy"):
            if windowed and e.off > WINDOW_REACH:
                note("window")
            if e.off > made - first_out:
                note("fragment start")
        made += e.n
    return found


# -------------------------------------------------------------------------------------------------------- lies --
Lie = collections.namedtuple("Lie", "name gran window256 chunk sizes cut promise valid")
# chunk: two fragments of 8 KiB (frag_log2 13); sizes: the table's (None: the streams'); cut: bytes the chunk and its
# size lack at the end; valid: Snappy for its chunk.  The code an invalid one makes is RESULT_OF_INVALID.
RESULT_OF_INVALID = 3              # HapResult_Bad_Frame: what hap.c makes of a chunk that snappy_uncompress refuses
SLOT_AT = 4400                     # output position of the twins' slot: an offset of 4096 has its source


def _replay(f, stream):
    for e in bare_elements(stream):
        if e.form.startswith("lit"):
            f.lit(e.n, int(e.form[3]), stream[e.pos + e.hdr: e.pos + e.hdr + e.n])
        else:
            f.copy(e.form, e.n, e.off)


@functools.lru_cache(None)
def _body(gran, size, seed):
    return mixed(gran, size, seed).stream()


def _twin(gran, seed, slot, name, before=b"", last=8):
    """An ordinary body, a serial literal, the slot (16 bytes of output), an ordinary body, a literal"""
    f = Fragment(gran, seed, name, before)
    _replay(f, _body(gran, SLOT_AT - 2 * gran, seed + 1))
    f.opener()
    assert f.made == SLOT_AT
    slot(f)
    assert f.made == SLOT_AT + 16, name
    _replay(f, _body(gran, 8192 - 8 - f.made, seed + 2))
    return f.lit(last)


def _honest_slot(f):
    f.lit(8).copy("copy2", 8, 8)


@functools.lru_cache(None)
def honest_twin(gran):
    a = _twin(gran, 9000 * gran, _honest_slot, "honest twin, first, GRAN %d" % gran)
    b = _twin(gran, 9000 * gran + 10, _honest_slot, "honest twin, second, GRAN %d" % gran, a.out)
    return [a, b]


@functools.lru_cache(None)
def lies(gran):
    g = gran
    found = []

    def add(name, promise, slot, which=0, window256=0, valid=True):
        a, b = honest_twin(g)
        if which == 0:
            a = _twin(g, 9000 * g, slot, name)
            b = _twin(g, 9000 * g + 10, _honest_slot, "honest second", a.out)
        else:
            b = _twin(g, 9000 * g + 10, slot, name, a.out)
        found.append(Lie("GRAN %d: %s" % (g, name), g, window256, [a, b], None, 0, promise, valid))
    if g >= 2:
        h = g // 2                                                     # a multiple of GRAN / 2 that is none of GRAN
        add("literal length %d" % (8 - h), "granularity", lambda f: f.lit(8 - h).lit(h).copy("copy2", 8, 8))
        add("copy length %d" % (8 - h), "granularity", lambda f: f.lit(8).copy("copy2", 8 - h, 8).copy("copy2", h, 8), which=1)
        add("copy offset %d" % (8 - h), "granularity", lambda f: f.lit(8).copy("copy2", 8, 8 - h))
        add("serial literal of %d" % (8 - h), "granularity", lambda f: f.lit(8 - h, 2).lit(h).copy("copy2", 8, 8), which=1)
        if g == 4:                                                     # (bit 0 of the serial path's check, beside bit 1)
            add("serial literal of 7", "granularity", lambda f: f.lit(7, 2).lit(1).copy("copy2", 8, 8))
    # one unit past the window: 3073 under GRAN 1; under GRAN 2 and 4 an offset of 3073 would break the granularity as
    # well, and a lie breaks one promise
    add("offset %d under a window promise" % (WINDOW_REACH + g), "window",
        lambda f: f.lit(8).copy("copy2", 8, WINDOW_REACH + g), window256=WINDOW_BYTE)
    add("offset 4096 under a window promise", "window", lambda f: f.lit(8).copy("copy2", 8, SLIDE_RING), which=1, window256=WINDOW_BYTE)
    add("copy from one unit before the fragment", "fragment start", lambda f: f.lit(8).copy("copy2", g, SLOT_AT + 8 + g).lit(8 - g), which=1)
    # an element across the fragment boundary: the first fragment's last literal one unit longer, the second's one shorter
    a = _twin(g, 9000 * g, _honest_slot, "one unit too many", last=8 + g)
    b = _twin(g, 9000 * g + 10, _honest_slot, "one unit too few", a.out[:8192], last=8 - g)
    a.claims = b.claims = 8192
    found.append(Lie("GRAN %d: an element across the fragment boundary" % g, g, 0, [a, b], None, 0, "fragment end", True))
    a, b = honest_twin(g)
    found.append(Lie("GRAN %d: two sizes of the table moved by one byte" % g, g, 0, [a, b], [a.total + 1, b.total - 1], 0, "table", True))
    found.append(Lie("GRAN %d: two sizes of the table moved back by one byte" % g, g, WINDOW_BYTE, [a, b], [a.total - 1, b.total + 1], 0, "table", True))
    # invalid for every decoder
    add("offset 0", "snappy", lambda f: f.lit(8).copy("copy2", 8, 0), valid=False)
    found.append(Lie("GRAN %d: the last element cut short by the chunk size" % g, g, 0, [a, b], [a.total, b.total - 1], 1, "snappy", False))
    short = _twin(g, 9000 * g + 10, _honest_slot, "one unit too few", a.out, last=8 - g)
    short.claims = 8192
    found.append(Lie("GRAN %d: a fragment that makes fewer bytes than its share" % g, g, 0, [a, short], None, 0, "snappy", False))
    return tuple(found)


# ------------------------------------------------------------------------------------------------------ frames --
Frame = collections.namedtuple("Frame", "frame want starts fragments")
# starts: where in the frame each fragment's first byte lies; want: None where the chunk is no Snappy


def frame_of_fragments(chunks, frag_log2, gran_log2, window256, fmt=FMT_DXT5, version=1, sizes=None, cut=0):
    """A Hap frame of one texture: compressor table (0x0B per chunk), chunk sizes, section 0x46, then the chunks, each a
    varint of its total and its fragments' bare elements.  Every chunk holds the same number of fragments, all but a
    chunk's last of 1 << frag_log2 bytes.  version 3: [3][13][g][w], the sizes, then 96 bytes per fragment that nobody
    may read (0xFF).  sizes: the table's entries where they are not the streams'; cut: bytes taken off the last chunk."""
    size = 1 << frag_log2
    per = len(chunks[0])
    streams, frags = [], []
    for c in chunks:
        claims = [f.made if f.claims is None else f.claims for f in c]
        assert len(c) == per and all(n == size for n in claims[:-1]) and 1 <= claims[-1] <= size, [f.name for f in c]
        streams.append(S.varint(sum(claims)) + b"".join(f.stream() for f in c))
        frags += c
    if cut:
        streams[-1] = streams[-1][: len(streams[-1]) - cut]
    entries = [f.total for f in frags] if sizes is None else list(sizes)
    assert len(entries) == len(frags)
    table = bytes([version, frag_log2, gran_log2, window256]) + b"".join(n.to_bytes(4, "little") for n in entries)
    if version == 3:
        assert frag_log2 == 13
        table += bytes([0xFF]) * (V3_GROUP_TABLE * len(frags))
    else:
        assert version == 1
    secs = section(2, bytes([0x0B]) * len(streams)) + section(3, b"".join(len(s).to_bytes(4, "little") for s in streams)) + \
        section(0x46, table)
    head = section(1, secs)
    frame = section(0xC0 | FORMAT_NIBBLE[fmt], head + b"".join(streams))
    at = len(frame) - sum(len(s) for s in streams)
    starts = []
    for c, s in zip(chunks, streams):
        p = at + len(S.varint(sum(f.made if f.claims is None else f.claims for f in c)))
        for f in c:
            starts.append(p)
            p += f.total
        at += len(s)
    return Frame(frame, b"".join(bytes(f.out) for f in frags), starts, frags)


def frame_of_lie(lie, fmt=FMT_DXT5):
    built = frame_of_fragments([lie.chunk], 13, GRAN_LOG2[lie.gran], lie.window256, fmt, 1, lie.sizes, lie.cut)
    return built if lie.valid else built._replace(want=None)


def lie_breaks(lie):
    return broken([f.stream() for f in lie.chunk], lie.sizes or [f.total for f in lie.chunk], lie.gran, lie.window256 != 0,
                  13, sum(f.made if f.claims is None else f.claims for f in lie.chunk), lie.cut)


# ------------------------------------------------------------------------------------------------- description --
def _walk(stream):
    """(pass, lane, element, output position) of every element, with the pass that takes it"""
    els = bare_elements(stream)
    for p in passes(stream):
        out = p.out
        for e in els[p.first: p.first + p.count]:
            yield p, e.pos - p.ip, e, out
            out += e.n


def _spec_of(gran):
    return {(form, n, arg): name for name, form, n, arg in form_list(gran)}


@functools.lru_cache(None)
def describe(gran):
    """What the families of a granularity hold, read back from the built bytes through elements() and the pass model"""
    d = {}
    # overlap: the copies
    d["overlap"] = {(e.form, e.n, e.off) for f in fragments("overlap", gran) for e in bare_elements(f.stream()) if e.form.startswith("copy")}
    # forms: (name, lane) for every element that is one of the listed forms; a literal of 2 to 4 length bytes is
    # met at the lane the chain in front of it stops at
    specs = _spec_of(gran)
    lanes = collections.defaultdict(set)

    def filler(e):
        return (e.form == "copy1" and e.n == 4 and e.off <= 32) or (e.form == "copy2" and e.n == gran and e.off == 4 * gran)
    for f in fragments("forms", gran):
        els = bare_elements(f.stream())
        by_ip = {p.ip: p for p in passes(f.stream())}
        for i, e in enumerate(els):
            if e.form != "lit2" or e.n != 2 * gran:
                continue
            start, j = e.pos + e.hdr + e.n, i + 1
            while filler(els[j]):
                j += 1
            x = els[j]
            key = (x.form, x.n, int(x.form[3]) if x.form.startswith("lit") else x.off)
            p, lane = by_ip[start], x.pos - start
            taken = p.first <= j < p.first + p.count if p.kind == "window" else j == p.first
            if key in specs and lane < 64 and (taken or p.stop == lane):
                lanes[specs[key]].add(lane)
    d["forms"] = dict(lanes)
    # staging, at phase 0: header splits by boundary parity; serial literal ends; what the staging did
    splits, serial_ends, events, memory = set(), set(), collections.Counter(), 0
    for f in fragments("staging", gran):
        for e, at, across in coordinates(f.stream(), 0):
            for boundary in across:
                splits.add((e.form, boundary - at, (boundary // GRANULE) & 1))
            if e.form in SPECIAL:
                end = e.pos + e.hdr + e.n
                near = (end + 1) // GRANULE * GRANULE
                if abs(end - near) <= 1:
                    serial_ends.add((end - near, (near // GRANULE) & 1))
        for p, event, mem in staging(f.stream(), 0):
            events[event] += 1
            memory += mem
    d["staging splits"], d["staging serial ends"], d["staging events"], d["staging memory steps"] = splits, serial_ends, events, memory
    d["staging skips"] = sorted({e.n for f in fragments("staging", gran) for e in bare_elements(f.stream()) if e.form in SPECIAL and e.n > 1024})
    # passes
    ps = [p for f in fragments("passes", gran) for p in passes(f.stream()) if p.kind == "window"]
    d["pass totals"] = {p.seen for p in ps}
    d["pass totals with a 256-byte literal"] = set()
    for f in fragments("passes", gran):
        els = bare_elements(f.stream())
        for p in passes(f.stream()):
            chain, q = [], p.first
            while p.kind == "window" and q < len(els) and els[q].pos - p.ip < 64 and els[q].form not in SPECIAL:
                chain.append(els[q])
                q += 1
            if any(e.form == "lit1" and e.n == 256 for e in chain):
                d["pass totals with a 256-byte literal"].add(p.seen)
    d["passes that end at 512"] = sum(1 for p in ps if p.N == OWNER)
    d["passes cut"] = sum(1 for p in ps if p.N < p.seen)
    d["most elements in a pass"] = max(p.count for p in ps)
    d["two-byte passes"] = sum(1 for p in ps if p.count == 32 and p.adv == 64)
    # chains
    depths = [x for f in fragments("chains", gran) for x in chain_depths(f.stream(), gran)]
    d["chain depths"] = set(depths)
    d["deepest chain"] = max(depths)
    d["chain offsets"] = {(e.n // gran, e.off // gran) for f in fragments("chains", gran) for e in bare_elements(f.stream())
                          if e.form.startswith("copy")}
    # window
    w = {"at reach": set(), "flush copies": set(), "flush serial": set(), "source across wrap": 0, "destination across wrap": 0, "most": 0}
    for f in fragments("window", gran):
        for p, lane, e, out in _walk(f.stream()):
            crossed = {k for k in range(1, 8) if out < FLUSH * k < out + e.n}
            if e.form.startswith("copy"):
                w["most"] = max(w["most"], e.off)
                w["flush copies"] |= crossed
                if e.off == WINDOW_REACH and p.N == OWNER:
                    w["at reach"] |= ({"first"} if e.pos == p.ip else set()) | ({"last"} if out + e.n == p.out + p.N else set())
                src = out - e.off
                w["source across wrap"] += src < SLIDE_RING < src + e.n
                w["destination across wrap"] += out < SLIDE_RING < out + e.n
            elif p.kind == "serial":
                w["flush serial"] |= crossed
    d["window"] = w
    # ends
    d["ends"] = [(fr.frag_log2, [[f.made for f in c] for c in fr.chunks]) for fr in family_frames("ends", gran)]
    d["rings"] = {fr.frag_log2: sorted({(e.form, e.off) for c in fr.chunks for f in c for p, _l, e, out in _walk(f.stream())
                                        if e.form.startswith("copy") and (e.off == out or e.off >= 32768)})
                  for fr in family_frames("rings", gran)}
    d["fragments"] = {fam: collections.Counter((fr.frag_log2) for fr in family_frames(fam, gran) for c in fr.chunks for _f in c)
                      for fam in FAMILIES}
    d["frames"] = {fam: len(family_frames(fam, gran)) for fam in FAMILIES}
    d["lies"] = len(lies(gran))
    return d

"""Hand-built Snappy streams for the foreign-stream decoders, and a plain decoder to hold them against.

Everything here is written from the format description: a varint length prefix, then elements whose
tag byte's low two bits say literal / copy with a 1-byte offset tail / 2-byte offset / 4-byte offset.  No GPU, no
ctypes: tests/test_snappy_streams.py pins decode() to libsnappy and to the oracle on every stream built here, and
tests/test_foreign_streams_gpu.py then uses decode() as the reference of the three roads a foreign stream can take
through hap_amd/csrc/snappy_decode.hip (whole stream / a wavefront per 64 KiB block / a workgroup per 64 KiB block).

The sweeps are deterministic generators.  Each returns a list of (name, stream, expected) where `expected` is the
number of the stream's blocks the workgroup-per-block kernel must take.  Two rules decide it, both read off the
kernel's own text and neither taken from a run:
  1. a block whose compressed bytes span more than 1024 windows of 64 bytes is declined (kBrkMaxWindows);
  2. a stream with a copy that reaches before its block is not made of independent blocks: none of it counts.
Every other block counts 1.  expected_blocks() recomputes the figure from the built bytes alone.
"""
import collections
import functools

import numpy as np

K = 65536                         # output bytes of a block (libsnappy's, and the block scan's)
MAX_WINDOWS = 1024                # windows of 64 compressed bytes the workgroup-per-block kernel takes
ADDRESS_PHASES = range(16)        # a stream's coordinates on the device begin at (address & 15): any of these


# ------------------------------------------------------------------------------------------------ element writers --
def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def lit(data, length_bytes=None):
    """A literal.  length_bytes: how many bytes follow the tag to hold the length (0: in the tag itself, up to 60);
    None picks the shortest form, anything longer than needed is valid Snappy all the same."""
    data = bytes(data)
    n = len(data)
    assert n >= 1
    if length_bytes is None:
        length_bytes = 0 if n <= 60 else 1 if n <= 256 else 2 if n <= 65536 else 3 if n <= 1 << 24 else 4
    if length_bytes == 0:
        assert n <= 60
        return bytes([(n - 1) << 2]) + data
    assert 1 <= length_bytes <= 4 and n <= 1 << (8 * length_bytes)
    return bytes([(59 + length_bytes) << 2]) + (n - 1).to_bytes(length_bytes, "little") + data


def copy1(n, off):
    assert 4 <= n <= 11 and 0 <= off < 2048
    return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 255])


def copy2(n, off):
    assert 1 <= n <= 64 and 0 <= off < 65536
    return bytes([2 | ((n - 1) << 2)]) + off.to_bytes(2, "little")


def copy4(n, off):
    assert 1 <= n <= 64 and 0 <= off < 1 << 32
    return bytes([3 | ((n - 1) << 2)]) + off.to_bytes(4, "little")


COPY_WRITERS = {"copy1": copy1, "copy2": copy2, "copy4": copy4}


def frame_of_streams(streams, fmt_byte=0xCE):
    """A Hap frame whose texture is these Snappy streams, one chunk each (decode instructions container with
    compressor and size tables)."""
    n = len(streams)
    comp = bytes([n & 255, n >> 8 & 255, n >> 16, 2]) + bytes([0x0B] * n)
    sizes = bytes([(4 * n) & 255, (4 * n) >> 8 & 255, (4 * n) >> 16, 3]) + b"".join(len(s).to_bytes(4, "little") for s in streams)
    tables = comp + sizes
    body = len(tables).to_bytes(3, "little") + bytes([1]) + tables + b"".join(streams)
    if len(body) < (1 << 24):
        return len(body).to_bytes(3, "little") + bytes([fmt_byte]) + body
    return bytes([0, 0, 0, fmt_byte]) + len(body).to_bytes(4, "little") + body


# ------------------------------------------------------------------------------------------------- plain decoder --
Element = collections.namedtuple("Element", "pos form hdr n off")      # form: lit0..lit4 (extra length bytes), copy1/2/4


def read_varint(stream):
    value = 0
    for i in range(5):
        if i >= len(stream):
            raise ValueError("truncated length prefix")
        value |= (stream[i] & 0x7F) << (7 * i)
        if not stream[i] & 0x80:
            if value >> 32:
                raise ValueError("length prefix above 32 bits")
            return value, i + 1
    raise ValueError("length prefix longer than five bytes")


def elements(stream):
    """The elements of a stream, in order, with their positions in it.  Raises where one is cut off."""
    _total, at = read_varint(stream)
    end = len(stream)
    while at < end:
        tag = stream[at]
        kind = tag & 3
        if kind == 0:
            code = tag >> 2
            if code < 60:
                extra, n = 0, code + 1
            else:
                extra = code - 59
                if at + 1 + extra > end:
                    raise ValueError("truncated literal header")
                n = int.from_bytes(stream[at + 1: at + 1 + extra], "little") + 1
            if at + 1 + extra + n > end:
                raise ValueError("truncated literal")
            el = Element(at, "lit%d" % extra, 1 + extra, n, 0)
            at += 1 + extra + n
        else:
            hdr = (0, 2, 3, 5)[kind]
            if at + hdr > end:
                raise ValueError("truncated copy")
            if kind == 1:
                el = Element(at, "copy1", 2, 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | stream[at + 1])
            else:
                el = Element(at, "copy2" if kind == 2 else "copy4", hdr, (tag >> 2) + 1,
                             int.from_bytes(stream[at + 1: at + hdr], "little"))
            at += hdr
        yield el


def decode(stream):
    """What the stream says, or ValueError.  Slices for literals; a copy that overlaps its own output repeats the
    `off` bytes in front of it."""
    stream = bytes(stream)
    total, _ = read_varint(stream)
    out = bytearray()
    for el in elements(stream):
        if el.form.startswith("lit"):
            out += stream[el.pos + el.hdr: el.pos + el.hdr + el.n]
        else:
            if el.off == 0:
                raise ValueError("offset zero")
            if el.off > len(out):
                raise ValueError("offset beyond the start")
            start = len(out) - el.off
            if el.off >= el.n:
                out += out[start: start + el.n]
            else:
                period = bytes(out[start:])
                out += (period * (el.n // el.off + 1))[: el.n]
        if len(out) > total:
            raise ValueError("output longer than the prefix")
    if len(out) != total:
        raise ValueError("output shorter than the prefix")
    return bytes(out)


def blocks_of(stream):
    """[(from, to, out_len, independent)] per 64 KiB of output: the compressed positions an element begins / the next
    block's begins at, and whether every copy of the block stays inside it.  None: an element crosses a block's end."""
    stream = bytes(stream)
    total, first = read_varint(stream)
    found, made, start, ok = [], 0, first, True
    for el in elements(stream):
        if made == K * (len(found) + 1):
            found.append((start, el.pos, K, ok))
            start, ok = el.pos, True
        if made // K != (made + el.n - 1) // K:
            return None
        if el.form.startswith("copy") and el.off > made % K:
            ok = False
        made += el.n
    found.append((start, len(stream), made - K * len(found), ok))
    assert made == total
    return found


def windows_spanned(start, end, phase=0):
    """Windows of 64 compressed bytes a block touches, as the workgroup-per-block kernel counts them"""
    return ((end + phase - 1) >> 6) - ((start + phase) >> 6) + 1


def expected_blocks(stream):
    """Blocks the workgroup-per-block kernel must take, by the two rules at the top, for every address phase the same
    (asserted: a sweep leaves no block's span to the address)."""
    blocks = blocks_of(stream)
    if blocks is None or not all(b[3] for b in blocks):
        return 0
    count = 0
    for start, end, _n, _ok in blocks:
        spans = {windows_spanned(start, end, s) > MAX_WINDOWS for s in ADDRESS_PHASES}
        assert len(spans) == 1, "a block's span depends on the stream's address"
        count += 0 if spans.pop() else 1
    return count


# ---------------------------------------------------------------------------------------------------- the builder --
class Block:
    """Elements of one block, and the output they make so far, so that a generator can state offsets and positions
    against the block.  at: the position in its stream of the block's first byte (the builders below pass it along;
    all their streams hold 16 KiB .. 2 MiB, a three-byte prefix).  before: the output in front of the block, for the
    one stream that reaches into it on purpose."""

    def __init__(self, seed, at=3, before=b""):
        self.rng = np.random.default_rng(seed)
        self.at = at
        self.before = bytes(before)
        self.parts = []
        self.out = bytearray()
        self.clen = 0

    @property
    def made(self):
        return len(self.out)

    @property
    def pos(self):
        """stream position of the next element's tag"""
        return self.at + self.clen

    def _add(self, part):
        self.parts.append(part)
        self.clen += len(part)

    def lit(self, n, length_bytes=None):
        """n seeded incompressible bytes"""
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self._add(lit(data, length_bytes))
        self.out += data
        return self

    def copy(self, form, n, off, reach=False):
        assert 1 <= off and (off <= self.made or reach), (form, n, off, self.made)
        self._add(COPY_WRITERS[form](n, off))
        if off > self.made:
            assert off - self.made <= len(self.before) and off - self.made >= n
            start = len(self.before) - (off - self.made)
            self.out += self.before[start: start + n]
        elif off >= n:
            start = self.made - off
            self.out += self.out[start: start + n]
        else:
            period = bytes(self.out[self.made - off:])
            self.out += (period * (n // off + 1))[:n]
        return self

    def fill(self, total):
        """Ordinary body up to at most `total`: a 40-byte literal and a copy of it, over and over (0.55 compressed:
        padding with literals alone would carry a block's compressed bytes past the 1024 windows)"""
        while total - self.made >= 80:
            self.lit(40)
            self.copy("copy2", 40, 40)
        return self

    def pad(self, total):
        """Exactly up to `total` with literals of at most 60 bytes: no case of their own"""
        assert self.made <= total
        while self.made < total:
            self.lit(min(60, total - self.made))
        return self

    def fill_to(self, total):
        return self.fill(total).pad(total)

    def align(self, phase):
        """Literals until the next tag's stream position is `phase` mod 64"""
        d = (phase - self.pos) % 64
        if d == 1:
            d = 65
        while d:
            step = min(d, 61)
            if d - step == 1:
                step -= 1
            self.lit(step - 1)
            d -= step
        assert self.pos % 64 == phase % 64
        return self

    def encoded(self):
        return b"".join(self.parts)


def stream_of(blocks):
    """Length prefix + blocks.  At least two blocks (the host only has streams scanned whose output may exceed
    64 KiB), every block but the last exactly 64 KiB, each where it said it would be."""
    assert len(blocks) >= 2
    total = sum(b.made for b in blocks)
    prefix = varint(total)
    at = len(prefix)
    for i, b in enumerate(blocks):
        assert b.made == K if i + 1 < len(blocks) else 1 <= b.made <= K, (i, b.made)
        assert b.at == at, (i, b.at, at)
        at += b.clen
    stream = prefix + b"".join(b.encoded() for b in blocks)
    # what the host reserves for a scanned stream: a unit slot per 64 KiB of 22 x the compressed bytes
    assert 22 * len(stream) >= total, "the host would not reserve a slot for every block"
    return stream


def _after(blocks):
    return blocks[-1].at + blocks[-1].clen if blocks else 3


def exact_block(seed, at, out_total, comp_total):
    """A block of `out_total` output bytes in exactly `comp_total` compressed bytes: literals of at most 60 bytes
    and copy2(64, 64)"""
    for copies in range(out_total // 64):
        lits = comp_total - out_total + 61 * copies
        lit_out = out_total - 64 * copies
        if lits >= 2 and lits <= lit_out <= 60 * lits:
            break
    else:
        raise AssertionError("no such block")
    b = Block(seed, at)
    base, extra = divmod(lit_out, lits)
    assert 2 * base >= 64
    for j in range(lits):
        b.lit(base + (1 if j < extra else 0))
        if j >= 1 and copies:
            b.copy("copy2", 64, 64)
            copies -= 1
    assert copies == 0 and b.made == out_total and b.clen == comp_total
    return b


# ------------------------------------------------------------------------------------------------------ a: overlaps --
OVERLAP_COPY4_OFFSETS = (1, 2, 3, 5, 63)


def overlap_cases():
    cases = []
    for off in range(1, 64):
        for n in range(off + 1, 65):
            cases.append(("copy2", n, off))
            if 4 <= n <= 11:
                cases.append(("copy1", n, off))
            if off in OVERLAP_COPY4_OFFSETS:
                cases.append(("copy4", n, off))
    return cases


@functools.lru_cache(None)
def sweep_overlap():
    """Every overlapping copy a 64-byte element can be: a seeded literal of off + 3 bytes, then the copy, back to back"""
    blocks, b = [], Block(1000)
    for form, n, off in overlap_cases():
        if b.made + off + 3 + n > K:
            blocks.append(b.pad(K))
            b = Block(1000 + len(blocks), _after(blocks))
        b.lit(off + 3)
        b.copy(form, n, off)
    blocks.append(b)
    return [("overlap table", stream_of(blocks), len(blocks))]


# ------------------------------------------------------------------------------------------- b: window / segment phase --
# the nine element forms, by what elements() says of them: (form, output bytes)
PHASE_FORMS = [("lit0", 20), ("lit1", 100), ("lit2", 300), ("lit3", 300), ("lit4", 5),
               ("copy1", 8), ("copy2", 30), ("copy4", 40), ("copy2", 64)]
PHASE_SEQUENCE_OUT = sum(n for _f, n in PHASE_FORMS)


def _phase_sequence(b):
    """Each form once.  Every copy reads the block's first 64 bytes (seeded literal bytes) -- the copy-1, whose offset
    ends at 2047, does so while it can and reads its own output of the repetition before from then on."""
    for extra, n in enumerate([20, 100, 300, 300, 5]):
        b.lit(n, extra)
    b.copy("copy1", 8, b.made - 3 if b.made - 3 < 2048 else PHASE_SEQUENCE_OUT)
    b.copy("copy2", 30, b.made - 7)
    b.copy("copy4", 40, b.made - 11)
    b.copy("copy2", 64, b.made)


def _phase_block(seed, at, p, total):
    b = Block(seed, at)
    b.lit(1 + p, 1)               # (one length byte for every p: the elements behind it move by one byte per phase)
    b.lit(64)
    while b.made + PHASE_SEQUENCE_OUT <= total:
        _phase_sequence(b)
    return b.pad(total)


@functools.lru_cache(None)
def sweep_phase():
    """The nine element forms in a fixed sequence that fills a block, pushed along by a literal of 1 + p bytes:
    over the 64 phases every form's tag sits at every byte of a window"""
    cases = []
    for p in range(64):
        first = _phase_block(2000 + 2 * p, 3, p, K)
        tail = _phase_block(2001 + 2 * p, _after([first]), p, 20000 + 37 * p)
        cases.append(("phase %d" % p, stream_of([first, tail]), 2))
    return cases


# ------------------------------------------------------------------------------- c: field widths of brk_do_window --
def _put_form(b, which):
    form, n = PHASE_FORMS[which]
    if form.startswith("lit"):
        b.lit(n, int(form[3]))
    else:
        b.copy(form, n, 100)


@functools.lru_cache(None)
def sweep_fields():
    """What brk_do_window packs into words, at the edges of the fields.  A tag's byte in its window depends on the
    stream's address on the device (coordinates begin at address & 15), so what wants a tag at a given byte comes
    sixteen times, once for every address."""
    cases = []
    blocks = []
    # 511 / 512 / 513 output bytes of elements that begin in one window, from the window's first byte on, with one
    # more tag in the same window behind them: the cut of a production pass at 512
    b = Block(3000).lit(64)
    for total in (511, 512, 513):
        for s in ADDRESS_PHASES:
            b.align(-s)
            for _ in range(total // 64):
                b.copy("copy2", 64, 64)
            if total % 64:
                b.copy("copy2", total % 64, 64)
            b.copy("copy2", 64, 64)
            b.lit(7)
    blocks.append(b.fill_to(K))
    # a one-length-byte literal of 256 bytes with its tag at the window's last byte: the furthest a window's staged
    # bytes are read
    b = Block(3001, _after(blocks)).lit(64)
    for s in ADDRESS_PHASES:
        b.align(63 - s)
        b.lit(256, 1)
        b.copy("copy2", 64, 256)
    blocks.append(b.fill_to(K))
    # offsets at the value the offset field saturates at
    b = Block(3002, _after(blocks)).lit(64).fill(700)
    for off in (510, 511, 512, 513):
        for n in (1, 64):
            for form in ("copy2", "copy4", "copy1"):
                if form == "copy1" and n == 64:
                    continue
                b.copy(form, 4 if form == "copy1" else n, off)
                b.lit(3)
    blocks.append(b.fill_to(K))
    # a block whose first element is a long literal
    for extra, n in ((2, 300), (3, 300), (4, 5), (2, 4000)):
        blocks.append(Block(3010 + extra + n, _after(blocks)).lit(n, extra).fill_to(K))
    blocks.append(Block(3020, _after(blocks)).lit(300, 2).fill_to(2999))
    cases.append(("field widths", stream_of(blocks), len(blocks)))
    # a block, and a stream, whose last element is each of the nine forms
    for which, (form, n) in enumerate(PHASE_FORMS):
        first = Block(3100 + which).fill_to(K - n)
        _put_form(first, which)
        tail = Block(3200 + which, _after([first])).fill_to(3000 + which - n)
        _put_form(tail, which)
        cases.append(("last element %s of %d" % (form, n), stream_of([first, tail]), 2))
    return cases


# --------------------------------------------------------------------------------------------------- d: block lengths --
TAILS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 8191, 8192, 8193, 65535, 65536)
THREE_BLOCK_TAILS = (1, 3, 65535)


def _tail_block(seed, at, n):
    """n bytes, with a copy where there is room for one"""
    b = Block(seed, at)
    if n < 5:
        return b.lit(n)
    if n <= 120:
        b.lit((n + 1) // 2)
        return b.copy("copy2", n // 2, (n + 1) // 2)
    return b.fill_to(n)


@functools.lru_cache(None)
def sweep_lengths():
    """Streams that end in blocks of every length class: below, at and above four, a window, a fine piece, a block"""
    cases = []
    for full, tails in ((1, TAILS), (2, THREE_BLOCK_TAILS)):
        for n in tails:
            blocks = []
            for i in range(full):
                blocks.append(Block(4000 + 7 * n + i, _after(blocks)).fill_to(K))
            blocks.append(_tail_block(4500 + n, _after(blocks), n))
            cases.append(("%d blocks, tail %d" % (full + 1, n), stream_of(blocks), full + 1))
    return cases


# ---------------------------------------------------------------------------------------------------------- e: chains --
@functools.lru_cache(None)
def sweep_chains():
    """Copies of copies of copies: the pointers of a block jump along them"""
    cases = []

    def add(name, chain):
        tail = Block(5100 + len(cases), _after([chain])).fill_to(30001)
        cases.append((name, stream_of([chain, tail]), 2))

    b = Block(5000).lit(4)
    for _ in range(16383):
        b.copy("copy1", 4, 4)
    add("copy1(4, 4), 16383 deep", b)
    b = Block(5001).lit(64)
    for _ in range(1023):
        b.copy("copy2", 64, 64)
    add("copy2(64, 64), 1023 deep", b)
    b = Block(5002).lit(1)
    while b.made < K:
        b.copy("copy2", min(64, K - b.made), 1)
    add("copy2(64, 1) run", b)
    b = Block(5003).lit(8)
    while K - b.made >= 40:
        b.copy("copy2", 24, 8)            # overlapping: three periods of the eight bytes in front
        b.copy("copy2", 16, 16)           # not overlapping: the two last of them again
    add("overlapping and plain copies in turn", b.pad(K))
    return cases


# ------------------------------------------------------------------------------------------------------ f: ring edges --
RINGS = (2048, 32768)


def ring_cases(ring):
    return [(off, n) for off in (ring - 1, ring, ring + 1, ring + 63, ring + 64) for n in (1, 63, 64)]


def _ring_block(seed, at, ring, total):
    b = Block(seed, at).lit(64)
    # just behind the ring's length: the source is the block's beginning
    for off, n in ring_cases(ring):
        if b.made < off:
            b.fill_to(off)
        b.copy("copy2", n, off)
        b.lit(5)
    # again further on, the copy's output lying across a multiple of 2048 (a ring's end, or a piece it gives back)
    for off, n in ring_cases(ring):
        at_out = ((b.made + 10 + n) // 2048 + 1) * 2048 - n // 2
        assert at_out + n <= total, (ring, off, n, at_out)
        b.fill_to(at_out)
        b.copy("copy4" if n == 63 else "copy2", n, off)
    return b.fill_to(total)


def _ring_margin_block(seed, at, ring, n):
    """Every offset from 1152 below the ring's length to 64 above it, once: the kernel takes a source from memory when
    it lies further back than the ring less one production pass (1088 bytes), whatever byte of the pass the copy is at:
    somewhere in this range a copy's source is part in the ring and part in memory"""
    b = Block(seed, at).lit(64).fill_to(ring + 64)
    for off in range(ring - 1152, ring + 65):
        b.copy("copy2", n, off)
    return b.fill_to(K)


@functools.lru_cache(None)
def sweep_ring():
    """Copies from as far back as the decoders' LDS rings are long (2 KiB: a wavefront per block; 32 KiB: the whole
    stream), all inside their block: a workgroup per block must take them too"""
    blocks = []
    for i, ring in enumerate(RINGS):
        blocks.append(_ring_block(6000 + i, _after(blocks), ring, K))
    blocks.append(_ring_margin_block(6010, _after(blocks), 2048, 48))
    blocks.append(_ring_margin_block(6011, _after(blocks), 32768, 24))
    blocks.append(_ring_block(6020, _after(blocks), 32768, 64901))
    return [("ring edges", stream_of(blocks), len(blocks))]


# --------------------------------------------------------------------------------------------- g: declines by design --
SPAN_BLOCK_COMPRESSED = K - 15            # 1024 windows from a window's first sixteen bytes, 1025 from its last sixteen
REACHING_STREAM = "copy into the block before"


@functools.lru_cache(None)
def sweep_declines():
    """Blocks the workgroup-per-block kernel leaves to the others by design: more than 1024 windows of compressed
    bytes; and a stream whose blocks are not independent, which is nobody's but the whole-stream decoder's"""
    cases = []
    first = Block(7000).lit(K)
    cases.append(("one literal of 64 KiB", stream_of([first, Block(7001, _after([first])).fill_to(30000)]), 1))
    for name, lead, want in (("1024 windows", 64 * 900 - 3, 3), ("1025 windows", 64 * 900 - 3 + 48, 2)):
        blocks = [exact_block(7010, 3, K, lead)]
        blocks.append(exact_block(7011, _after(blocks), K, SPAN_BLOCK_COMPRESSED))
        blocks.append(Block(7012, _after(blocks)).fill_to(5000))
        cases.append((name, stream_of(blocks), want))
    first = Block(7020).fill_to(K)
    second = Block(7021, _after([first]), before=first.out).lit(8)
    second.copy("copy2", 40, 4000, reach=True)
    cases.append((REACHING_STREAM, stream_of([first, second.fill_to(K)]), 0))
    return cases


SWEEPS = collections.OrderedDict([("overlap", sweep_overlap), ("phase", sweep_phase), ("fields", sweep_fields),
                                  ("lengths", sweep_lengths), ("chains", sweep_chains), ("ring", sweep_ring),
                                  ("declines", sweep_declines)])


@functools.lru_cache(None)
def decoded(stream):
    return decode(stream)

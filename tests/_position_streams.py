"""The position-per-lane Snappy compressor (snappy_compress_wg_kernel<GRAN, FL>, hap_amd/csrc/snappy_compress.hip) as
plain scalar code, and inputs that reach the corners of its rules.

compress_fragment() is the definition the kernel is held to, byte for byte (tests/test_position_streams_gpu.py).  It is
written from the rules, one position at a time; nothing of lanes, ballots or waves is in it.  tests/test_position_streams.py
pins it without a GPU: its streams decode through the plain decoder of tests/_snappy_streams.py, libsnappy and the
oracle, keep the promises the fragment table makes, and a few tiny ones are written out by hand.

The rules, for one fragment of n bytes (n a multiple of GRAN; a position is a multiple of GRAN):

  geometry   a TILE is 64 positions (64 * GRAN bytes), a SUPERTILE two tiles, a ROUND four supertiles.
  table      2048 entries, all zero at first, indexed by (le32(4 bytes at p) * 0x1e35a7bd) >> 21.  Every position looked
             up in a round sees the table as it stood after the round before.  After a round, every position of the
             round at which a literal granule or a copy begins and that has 4 bytes left (p + 4 <= n) is entered; an
             entry holds the highest position entered so far.  (Entering position 0 changes nothing: an entry that was
             never written and one that holds position 0 are the same thing, and both offer position 0 as a candidate.)
  room       a copy that begins at p ends at or before its supertile's end and the data's, and is at most 64 bytes.
  hash       candidate c = the entry of p's hash.  It counts when p + 4 <= n, room >= 4, c < p, p - c <= window (when
             there is one) and at least 4 bytes agree; its length is the number of agreeing bytes, at most the room,
             rounded down to GRAN.
  fixed      for k = 1..4, distance k * pitch (pitch: the block size, 8 or 16 bytes): the run of granules from p on that
             equal the granule `distance` before them (which must exist), at most the room.
  choice     the longest candidate; among fixed distances of equal length the FARTHER one; the hash candidate only
             when strictly longer than every fixed one.  Shorter than 4 bytes: no candidate.
  selection  left to right through a tile: a position with a candidate begins a copy, and the next position looked at
             is the one behind it; a position without is a literal granule.  A copy that began in a supertile's first
             tile may end in its second: that tile begins behind it.
  literals   the literal granules of a TILE that follow one another are one literal (so a literal never crosses a tile's
             end): tag (len - 1) << 2 up to 60 bytes, above that tag 60 << 2 and one byte len - 1 (a tile is at most 256).
  copies     length < 12 and offset < 2048: copy-1 (2 bytes), else copy-2 (3 bytes).

RULES holds the four constants the pinning tests perturb one at a time (tests/test_position_streams.py).
"""
import collections
import functools

import numpy as np

from _snappy_streams import copy2, lit, varint
from _snappy_streams import elements as _parse_elements

HASH_BITS = 11
HASH_MUL = 0x1E35A7BD
FIXED = 4                                   # candidates at 1..4 block pitches
WINDOW = 3072                               # what 8 KiB fragments of large textures promise (12 x 256 bytes)

Rules = collections.namedtuple("Rules", "same_round_visible tie_farther copy1_below literal_tag_max")
RULES = Rules(same_round_visible=False, tie_farther=True, copy1_below=12, literal_tag_max=60)

# pos: where the element's output begins in the fragment; kind: lit / copy1 / copy2; via: lit / hash / fixed;
# pitches: which fixed distance (0 otherwise)
El = collections.namedtuple("El", "pos kind n off via pitches")


def tile_bytes(gran):
    return 64 * gran


def supertile_bytes(gran):
    return 128 * gran


def round_bytes(gran):
    return 512 * gran


def hash_of(word):
    return ((word * HASH_MUL) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def fragment_elements(data, gran, pitch, window=None, rules=RULES, stats=None):
    """The elements of one fragment, in order.  stats (a Counter) learns what the hash stage met on the way."""
    data = bytes(data)
    n = len(data)
    assert gran in (1, 2, 4) and pitch in (8, 16) and 0 < n <= 65536 and n % gran == 0
    tile, sup, rnd = tile_bytes(gran), supertile_bytes(gran), round_bytes(gran)
    a = np.frombuffer(data, dtype=np.uint8)
    # fixed[k][p]: bytes from p on, in whole granules, that equal what lies k pitches before them (uncapped)
    fixed = [None]
    for k in range(1, FIXED + 1):
        d = k * pitch
        same = np.zeros(n // gran, dtype=bool)
        if n > d:
            eq = (a[d:] == a[:-d]).reshape(-1, gran).all(axis=1)
            same[d // gran:] = eq
        # (the run from i on ends at the first granule from i on that is not the same)
        at = np.arange(n // gran)
        ends = np.minimum.accumulate(np.where(same, n // gran, at)[::-1])[::-1]
        fixed.append(((ends - at) * gran).tolist())
    padded = data + bytes(4)
    words = [int.from_bytes(padded[p: p + 4], "little") for p in range(0, n, gran)]
    table = {}
    els = []
    if stats is None:
        stats = collections.Counter()

    def candidate(p, room):
        """(length, rank, offset, via, pitches) of the best candidate at p, or None.  rank decides between equal
        lengths: the hash candidate's is the lowest."""
        found = []
        if p + 4 <= n and room >= 4:
            entry = table.get(hash_of(words[p // gran]))
            c = entry or 0
            if c < p and (window is None or p - c <= window):
                m = 0
                while m < room and data[c + m] == data[p + m]:
                    m += 1
                if m >= 4:
                    found.append((m - m % gran, 0, p - c, "hash", 0))
                    stats["hash candidates at position 0 from an entry never written" if entry is None else "hash candidates"] += 1
                else:
                    stats["entries never written that fail the comparison" if entry is None
                          else "entries that fail the comparison"] += 1
            elif c < p:
                stats["entries beyond the window"] += 1
        for k in range(1, FIXED + 1):
            found.append((min(fixed[k][p // gran], room), k if rules.tie_farther else FIXED + 1 - k, k * pitch, "fixed", k))
        best = max(found)
        return best if best[0] >= 4 else None

    for round_at in range(0, n, rnd):
        entered = []

        def enter(p):
            if p + 4 <= n and p:                     # (position 0 is what an entry never written offers anyway)
                if rules.same_round_visible:
                    table[hash_of(words[p // gran])] = p
                else:
                    entered.append(p)

        for sup_at in range(round_at, min(n, round_at + rnd), sup):
            sup_end = min(n, sup_at + sup)
            p = sup_at
            for tile_at in range(sup_at, sup_end, tile):
                tile_end = min(sup_end, tile_at + tile)
                p = max(p, tile_at)
                run_at = None                        # where the literal being gathered began
                while p < tile_end:
                    found = candidate(p, min(64, sup_end - p))
                    if found is None:
                        if run_at is None:
                            run_at = p
                        enter(p)
                        p += gran
                        continue
                    if run_at is not None:
                        els.append(El(run_at, "lit", p - run_at, 0, "lit", 0))
                        run_at = None
                    length, _rank, off, via, pitches = found
                    small = length < rules.copy1_below and off < 2048
                    els.append(El(p, "copy1" if small else "copy2", length, off, via, pitches))
                    enter(p)
                    p += length
                if run_at is not None:
                    els.append(El(run_at, "lit", tile_end - run_at, 0, "lit", 0))
        for p in entered:                            # (in rising order: the highest position stays)
            table[hash_of(words[p // gran])] = p
    return els


def encode_elements(data, els, rules=RULES):
    out = bytearray()
    for el in els:
        if el.kind == "lit":
            body = data[el.pos: el.pos + el.n]
            out += bytes([(el.n - 1) << 2]) + body if el.n <= rules.literal_tag_max else lit(body, 1)
        elif el.kind == "copy1":
            out += bytes([1 | ((el.n - 4) << 2) | ((el.off >> 8) << 5), el.off & 255])
        else:
            out += copy2(el.n, el.off)
    return bytes(out)


def compress_fragment(data, gran, pitch, window=None, rules=RULES):
    data = bytes(data)
    return encode_elements(data, fragment_elements(data, gran, pitch, window, rules), rules)


def chunk_fragments(data, gran, pitch, frag_log2=13, window=None, rules=RULES):
    """[fragment streams] of a chunk: fragments of 2^frag_log2 bytes, the last one whatever is left"""
    size = 1 << frag_log2
    return [compress_fragment(data[at: at + size], gran, pitch, window, rules) for at in range(0, len(data), size)]


def compress_chunk(data, gran, pitch, frag_log2=13, window=None, rules=RULES):
    """A chunk's Snappy stream: the length prefix, then its fragments' elements"""
    return varint(len(data)) + b"".join(chunk_fragments(data, gran, pitch, frag_log2, window, rules))


def stream_elements(stream):
    """the elements of a fragment's stream (no length prefix in front), positions counted in it"""
    for el in _parse_elements(bytes([0]) + bytes(stream)):
        yield el._replace(pos=el.pos - 1)


# ------------------------------------------------------------------------------------------------------- inputs --
# A CASE is one fragment's worth of bytes (or less, for a last fragment).  Its body is seeded noise, which neither the
# table nor the fixed distances find anything in; what the case is about is written over it.  A texture is cases one
# after the other and compressible filler behind them, so that its chunk shrinks whatever the cases do.
class Frag:
    def __init__(self, size, seed):
        self.rng = np.random.default_rng([20261019] + list(seed))
        self.b = bytearray(self.rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        self.wanted = []                        # (position, offset, length, write it anew) of the hash copies asked for

    def noise(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def put(self, at, what):
        assert 0 <= at and at + len(what) <= len(self.b), (at, len(what), len(self.b))
        self.b[at: at + len(what)] = what
        return self

    def differ(self, at, *others):
        """the byte at `at` made unlike the bytes at `others`"""
        if at < len(self.b):
            v = self.b[at]
            while any(o < len(self.b) and self.b[o] == v for o in others if o != at):
                v = (v + 1) & 255
            self.b[at] = v
        return self

    def repeat(self, at, n, dist):
        """n bytes at `at` equal what lies `dist` before them (overlapping: periodic), and not one byte more: the byte
        in front and the byte behind differ from theirs"""
        assert at >= dist
        if at > dist:
            self.differ(at - 1, at - 1 - dist)
        for q in range(at, min(len(self.b), at + n)):
            self.b[q] = self.b[q - dist]
        self.differ(at + n, at + n - dist)
        return self

    def again(self, at, n, src, found=True, fresh=True):
        """n bytes at `at` equal the n at `src` (far in front), and not one more.  found: settle() sees to it that the
        table offers `src` at `at` (fresh: it may write other bytes to both places for that)"""
        assert src + n <= at

        def write(anew):
            if anew:
                self.put(src, self.noise(n))
            self.b[at: at + n] = self.b[src: src + n]
            self.differ(at + n, src + n)
            if src:
                self.differ(at - 1, src - 1)
        write(False)
        if found:
            assert fresh or src == 0
            self.wanted.append((at, at - src, min(n, 64), write if fresh else None))
        return self

    def want(self, at, off, n, write):
        self.wanted.append((at, off, n, write))
        return self

    def flat(self, start, stop, value):
        self.b[start: stop] = bytes([value]) * (stop - start)
        return self

    def settle(self, gran, pitch, window=None):
        """The table has 2048 entries: noise between a source and its repeat may take the source's.  Until every hash
        copy asked for is in the definition's elements, the sources that were lost get other bytes."""
        for _ in range(400):
            at_of = {e.pos: e for e in fragment_elements(self.bytes(), gran, pitch, window) if e.via == "hash"}
            lost = [w for w in self.wanted
                    if not (w[0] in at_of and at_of[w[0]].off == w[1] and at_of[w[0]].n == w[2] - w[2] % gran)]
            if not lost:
                return self
            for at, _off, _n, write in lost:
                if write is None:                   # (the fragment's first bytes are the source: other noise behind them)
                    self.put(8, self.noise(at - 16))
                else:
                    write(True)
        raise AssertionError("the hash copies asked for cannot all be had: %r" % [w[:3] for w in lost])

    def bytes(self):
        return bytes(self.b)


LENGTHS = tuple(range(3, 71))


def lengths_fixed_places(gran, size=8192):
    """[(fragment of the fixed half of sweep a, position, length)]: one repeat per supertile, 16 bytes into it (it ends
    inside the supertile)"""
    sup = supertile_bytes(gran)
    per = size // sup
    return [(i // per, (i % per) * sup + 16, n) for i, n in enumerate(LENGTHS)]


def lengths_hash_places(gran, size=8192):
    """[(fragment of the hash half, position, length)]: rounds in pairs, the first holds the sources, the second the
    repeats, one per supertile: the distance is a round's bytes, more than four pitches"""
    sup, rnd = supertile_bytes(gran), round_bytes(gran)
    per = 4 * (size // (2 * rnd))
    return [(i // per, ((i % per) // 4) * 2 * rnd + (i % 4) * sup + 16 + rnd, n) for i, n in enumerate(LENGTHS)] if per else []


def sweep_lengths(gran, pitch, size=8192):
    """a: repeats of every length 3..70, one pitch back (`fixed`) and a round back (`hash`)"""
    rnd = round_bytes(gran)
    cases = []
    for places, far in ((lengths_fixed_places(gran, size), False), (lengths_hash_places(gran, size), True)):
        for frag in sorted({p[0] for p in places}):
            f = Frag(size, (2 if far else 1, gran, pitch, size, frag))
            for _frag, at, n in (p for p in places if p[0] == frag):
                if far:
                    f.again(at, n, at - rnd, found=n - n % gran >= 4)
                    if (n - 64) - (n - 64) % gran >= 4:                  # what the cap at 64 leaves is a copy of its own
                        f.want(at + 64, rnd, n - 64, f.wanted[-1][3])
                else:
                    f.repeat(at, n, pitch)
            cases.append(("lengths %s %d" % ("hash" if far else "fixed", frag), f.settle(gran, pitch).bytes()))
    return cases


def offsets_of(gran, size, window):
    """the hash offsets sweep b goes for"""
    want = [d for d in range(2044, 2053) if d % gran == 0]
    if window:
        want += [window - gran, window, window + gran]
    if size >= 8192:
        want += [size - 12]
    if size > 32768:
        want += [32768 - gran, 32768, 32768 + gran, 40000]
    return want


def sweep_offsets(gran, pitch, size=8192, window=None):
    """b: hash copies of 8 bytes at chosen offsets; ties between candidates"""
    rnd = round_bytes(gran)
    cases = []
    if size >= 8192:
        # the fragment is one value (that takes one entry of the table, not thousands) but for 48 bytes of noise
        # around every source and every repeat; a repeat stands 32 bytes into a supertile
        f = Frag(size, (3, gran, pitch, size))
        island = f.noise(48 * 64)
        f.flat(16, size, 0xA5)
        taken, nxt = [], 2048
        for i, d in enumerate(offsets_of(gran, size, window)):
            spans = lambda at: [(max(0, x - 16), min(size, x + 32)) for x in (at - d, at)]
            free = lambda at: all(hi <= t0 or t1 <= lo for lo, hi in spans(at) for t0, t1 in taken)
            if d < size - 12:
                nxt = max(nxt, (d + 64 + 127) // 128 * 128)
                while not free(nxt + 32):
                    nxt += 128
                at, nxt = nxt + 32, nxt + 128
            else:
                at = size - 8                                      # (size - 12: from byte 4 to the last 8 bytes)
            assert free(at) and at + 40 <= size or at == size - 8, d
            for lo, hi in spans(at):
                taken.append((lo, hi))
                f.put(lo, island[48 * len(taken): 48 * len(taken) + hi - lo])
            f.again(at, 8, at - d, found=not (window and d > window))
        cases.append(("offsets", f.settle(gran, pitch, window).bytes()))
        if not window:
            # the longest offset there is: the fragment's first four bytes again as its last four
            f = Frag(size, (4, gran, pitch, size))
            f.flat(1024, size - 32, 0x5A)
            f.again(size - 4, 4, 0, fresh=False)
            cases.append(("offset size - 4", f.settle(gran, pitch).bytes()))
    f = Frag(size, (5, gran, pitch, size))
    base = size - rnd if size >= 2 * rnd else 0
    # two fixed distances, equal length: three blocks that agree in their first 4 bytes and not in the fifth.  The
    # second one copies 4 bytes from the first; the third can take them from either
    t = base + 64
    head = f.noise(4)
    for k in range(3):
        f.put(t + k * pitch, head)
    f.differ(t + pitch + 4, t + 4).differ(t + 2 * pitch + 4, t + 4, t + pitch + 4)
    if size >= 2 * rnd:
        # fixed against hash, equal length: 8 bytes that stand a round in front and one pitch in front
        q, far = base + 192, base - rnd + 40

        def equal(anew):
            s8 = f.noise(8)
            f.put(far, s8).put(q, s8).put(q + pitch, s8)
            f.differ(far + 8, q + 8)
            f.differ(q + pitch + 8, far + 8, q + 8)
        equal(True)
        f.want(q, q - far, 8, equal)
        # hash longer by a granule: 8 + GRAN bytes a round in front, 8 of them one pitch in front
        r, farther = base + 320, base - rnd + 120

        def longer(anew):
            s12 = f.noise(8 + gran)
            f.put(farther, s12).put(r, s12[:8]).put(r + pitch, s12)
            f.differ(farther + 8, r + 8)
            f.differ(r + pitch + 8 + gran, farther + 8 + gran, r + 8 + gran)
        longer(True)
        f.want(r, r - farther, 8, longer).want(r + pitch, r + pitch - farther, 8 + gran, longer)
    f.settle(gran, pitch, window)
    cases.append(("ties", f.bytes()))
    return cases


def positions_places(gran, size=8192):
    """[(fragment of sweep c, position, length, which position of its supertile)]: supertiles in pairs behind a leading
    one; the repeat begins in the first of a pair, what it spills lands in the second"""
    sup = supertile_bytes(gran)
    slots = max(1, (size // sup - 1) // 2)
    frags = -(-128 // slots)
    return [(k * frags + j // slots, sup * (1 + 2 * (j % slots)) + gran * j, n, j)
            for k, n in enumerate((12, 64)) for j in range(128)]


def sweep_positions(gran, pitch, size=8192):
    """c: a 12-byte and a 64-byte repeat (one pitch back) beginning at every position of a supertile"""
    places = positions_places(gran, size)
    cases = []
    for frag in range(places[-1][0] + 1):
        f = Frag(size, (6, gran, pitch, size, frag))
        for _frag, at, n, _j in (p for p in places if p[0] == frag):
            f.repeat(at, n, pitch)
        cases.append(("positions %d" % frag, f.bytes()))
    return cases


def sweep_literals(gran, pitch, size=8192):
    """d: literals of 60 bytes and a granule more, behind a copy carried into their tile and from a tile's first byte;
    a granule between two copies; whole tiles of literals (the noise around).  A fragment each, in its second
    supertile."""
    tile = tile_bytes(gran)
    t = 2 * tile
    cases = []

    def case(name, build):
        f = Frag(size, (7, gran, pitch, size, len(cases)))
        build(f)
        cases.append(("literals " + name, f.bytes()))

    for run in (60, 60 + gran):
        def carried(f, run=run):
            # a copy that ends `lead` bytes into the supertile's second tile, `run` literal bytes, a copy or the tile's end
            lead = min(8, tile - run)
            f.repeat(t + tile + lead - 12, 12, pitch)
            if lead + run + 12 <= tile:
                f.repeat(t + tile + lead + run, 12, pitch)
        case("%d carried" % run, carried)
        if run + 12 <= tile:
            case("%d first" % run, lambda f, run=run: f.repeat(t + run, 12, pitch))
    case("between", lambda f: f.repeat(t + 16, 12, pitch).repeat(t + 28 + gran, 12, pitch))
    return cases


def sweep_table(gran, pitch, size=8192):
    """e: what the table holds when.  Five cases in one fragment, each with 8 bytes of its own:
         same      again 80 bytes on, in the same round: not found
         before    again a round later: found
         waves     twice in one round (two supertiles apart), again two rounds later: the later of the two is found
         covered   16 bytes, again a round later (a copy), their bytes 4..12 again two rounds later: found in the
                   literal, not in the copy, although the copy is nearer
         first     the fragment's first 8 bytes again in its first round: found at position 0"""
    rnd, sup = round_bytes(gran), supertile_bytes(gran)
    if size < 4 * rnd:
        return []
    f = Frag(size, (8, gran, pitch, size))
    f.again(16 + 80, 8, 16, found=False)                            # same
    f.again(sup + 16 + rnd, 8, sup + 16)                            # before

    def waves(anew):
        f.put(sup + 48, f.noise(8))
        f.again(3 * sup + 16, 8, sup + 48, found=False)             # the second source (same round: not found) ...
        f.again(2 * rnd + sup + 48, 8, sup + 48, found=False)       # ... and the repeat
    waves(True)
    f.want(2 * rnd + sup + 48, 2 * rnd + sup + 48 - (3 * sup + 16), 8, waves)

    def covered(anew):
        f.put(2 * sup + 32, f.noise(16))
        f.again(rnd + 2 * sup + 32, 16, 2 * sup + 32, found=False)
        f.again(3 * rnd + 2 * sup + 32, 8, 2 * sup + 36, found=False)
    covered(True)
    f.want(rnd + 2 * sup + 32, rnd, 16, covered).want(3 * rnd + 2 * sup + 32, 3 * rnd - 4, 8, covered)
    f.again(2 * sup + 80, 8, 0, fresh=False)                        # first
    f.settle(gran, pitch)
    return [("table", f.bytes())]


def end_sizes(gran):
    tile, sup = tile_bytes(gran), supertile_bytes(gran)
    return [16, 48, tile - gran, tile + gran, sup - gran, sup + gran]


def sweep_ends(gran, pitch, size=8192):
    """f: last fragments of 16 and 48 bytes, and of a tile and a supertile less and more a granule: [(name, texture)],
    each texture a full fragment of filler and the short one.  The short ones of 16 and 48 bytes are two equal halves
    (8 and 24 bytes apart: a fixed distance at pitch 8, at pitch 16 what the table's unwritten entries find at
    position 0); the others end in a repeat one pitch back that runs to the data's last byte.  Then tiles in whose
    last 4 bytes, and last 3 or 2, a repeat begins."""
    cases = []
    for n in end_sizes(gran):
        f = Frag(size + n, (9, gran, pitch, size, n))
        f.put(0, filler(size, n))
        if n < 64:
            f.put(size + n // 2, f.b[size: size + n // 2])         # the second half equals the first
        else:
            f.repeat(size + n - 20, 20, pitch)
        cases.append(("end %d" % n, f.bytes()))
    # a repeat that begins in the data's last 3 bytes (no copy: fewer than 4 are left; GRAN 4 has no such position),
    # and one of exactly the last 4
    n = tile_bytes(gran)
    for back in ([4] if gran == 4 else [4, 4 - gran]):
        f = Frag(size + n, (10, gran, pitch, size, back))
        f.put(0, filler(size, back)).repeat(size + n - back, back, pitch)
        cases.append(("end begins %d before" % back, f.bytes()))
    return cases


def filler(n, seed=0):
    """compressible bytes behind the cases: runs of 24..200 equal bytes"""
    rng = np.random.default_rng([77, seed])
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(24, 200))
    return bytes(out[:n])


FRAGMENT_SWEEPS = collections.OrderedDict([("lengths", sweep_lengths), ("offsets", sweep_offsets),
                                           ("positions", sweep_positions), ("literals", sweep_literals),
                                           ("table", sweep_table)])


@functools.lru_cache(None)
def cases(sweep, gran, pitch, size=8192, window=None):
    if sweep == "offsets":
        return tuple(sweep_offsets(gran, pitch, size, window))
    return tuple(FRAGMENT_SWEEPS[sweep](gran, pitch, size))


@functools.lru_cache(None)
def texture(gran, pitch, frag_log2=13, window=None, sweeps=tuple(FRAGMENT_SWEEPS), total=None):
    """(texture, fragments that hold cases): the cases of `sweeps` one after the other, then filler for a third of
    their bytes in whole fragments (or up to `total` bytes): one chunk, which shrinks whatever the cases do."""
    size = 1 << frag_log2
    body = b"".join(c for sweep in sweeps for _name, c in cases(sweep, gran, pitch, size, window))
    assert len(body) % size == 0
    extra = -(-len(body) // (3 * size)) * size if total is None else total - len(body)
    assert extra * 3 >= len(body)
    return body + filler(extra, len(body)), len(body) // size


def unaligned_texture(gran, pitch):
    """Two chunks of an odd number of 8-byte blocks (3073): the second begins at 8 mod 16.  Each is a case fragment
    and filler."""
    chunk = 8 * 3073
    parts = [cases(sweep, gran, pitch)[0][1] for sweep in ("table", "literals")]
    return b"".join(c + filler(chunk - len(c), i) for i, c in enumerate(parts)), chunk


@functools.lru_cache(None)
def modelled(data, gran, pitch, window=None):
    """(elements, stream) of one fragment, computed once"""
    els = fragment_elements(data, gran, pitch, window)
    return tuple(els), encode_elements(data, els)


def model_chunk(data, gran, pitch, frag_log2=13, window=None):
    """(stream, [fragment sizes]) of a chunk through the cache"""
    size = 1 << frag_log2
    parts = [modelled(data[at: at + size], gran, pitch, window)[1] for at in range(0, len(data), size)]
    return varint(len(data)) + b"".join(parts), [len(p) for p in parts]


# (gran, pitch, fragment log2, window): what the roads of tests/test_position_streams_gpu.py run
SETTINGS = [(2, 16, 13, None), (2, 8, 13, None), (4, 16, 13, None), (4, 8, 13, None), (1, 16, 13, None), (1, 8, 13, None),
            (2, 16, 10, None), (4, 8, 10, None), (2, 16, 13, WINDOW)]
BIG = (2, 16, 16, None)                     # 64 KiB fragments: the offsets sweep and one fragment of lengths

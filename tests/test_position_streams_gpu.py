"""The position-per-lane Snappy compressor (snappy_compress_wg_kernel<GRAN, FL>, hap_amd/csrc/snappy_compress.hip) against
its scalar definition, tests/_position_streams.py, byte for byte, on every road of the product library that reaches it.

The textures are raw bytes: the sweeps of the definition's module (repeats of every length, offsets around the edges of
the element forms and the match window, a repeat at every position of a supertile, literal edges, what the table holds
when, short last fragments, a chunk at 8 mod 16).  tests/test_position_streams.py holds the definition to the decoders
and to hand-written streams, and asserts from its element lists that every sweep reaches what it is there for.

Per road: every Snappy chunk's bytes and every fragment size of the table are the definition's, the table's header
says the granularity, fragment size and window the road stands for (a texture that went to the block-per-lane kernels
instead would carry a version-4 table and fail here), both checkers and this library's decoder give the texture back
without a table fall-back, and a second encode, three to a batch, gives the first frame's bytes three times."""
import os

import numpy as np
import pytest

import _libs as L
import _position_streams as M
from test_gpu_parity import CHECKERS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hap():
    import hap_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hap_amd


@pytest.fixture(scope="module")
def contexts(hap):
    """A context per setting that is the context's and not the call's: the default one, HAP_AMD_BYTE_GRANULAR=1,
    fragments of 1 KiB and of 64 KiB."""
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "bytes":
                os.environ["HAP_AMD_BYTE_GRANULAR"] = "1"
            try:
                c = hap.Context(0)
            finally:
                os.environ.pop("HAP_AMD_BYTE_GRANULAR", None)
            if kind in ("1k", "64k"):
                assert c.set_fragment_log2(10 if kind == "1k" else 16) == 0
            made[kind] = c
        return made[kind]
    yield get
    for c in made.values():
        c.close()


# ----------------------------------------------------------------------------------------------- reading a frame --
def _section(frame, at):
    """(header bytes, length, type) of the section at `at`"""
    n = int.from_bytes(frame[at: at + 3], "little")
    if n:
        return 4, n, frame[at + 3]
    return 8, int.from_bytes(frame[at + 4: at + 8], "little"), frame[at + 3]


def textures_of(frame):
    """Per texture of a frame: dict(type, codecs, sizes, table, chunks).  table: (version, header bytes, fragment sizes)
    of the private section 0x46 (any fragment size), or None; chunks: the chunks' bytes as stored."""
    frame = bytes(frame)
    hdr, n, kind = _section(frame, 0)
    assert hdr + n == len(frame)
    spans = []
    if kind == 0x0D:
        at = hdr
        while at < len(frame):
            h, m, _k = _section(frame, at)
            spans.append((at, at + h + m))
            at += h + m
    else:
        spans.append((0, len(frame)))
    found = []
    for start, stop in spans:
        h, m, kind = _section(frame, start)
        tex = dict(type=kind, codecs=b"", sizes=[], table=None, chunks=[])
        if kind >> 4 == 0xC:
            ih, im, ik = _section(frame, start + h)
            assert ik == 0x01
            at, end = start + h + ih, start + h + ih + im
            while at < end:
                sh, sm, sk = _section(frame, at)
                body = frame[at + sh: at + sh + sm]
                if sk == 0x02:
                    tex["codecs"] = body
                elif sk == 0x03:
                    tex["sizes"] = [int.from_bytes(body[i: i + 4], "little") for i in range(0, sm, 4)]
                elif sk == 0x46:
                    tex["table"] = (body[0], body[:4], body[4:])
                at += sh + sm
            assert at == end
            for size in tex["sizes"]:
                tex["chunks"].append(frame[at: at + size])
                at += size
            assert at == stop
        found.append(tex)
    return found


def fragment_sizes(table, count):
    assert table[0] == 1 and len(table[2]) == 4 * count, (table[0], len(table[2]), count)
    return [int.from_bytes(table[2][i: i + 4], "little") for i in range(0, 4 * count, 4)]


# ------------------------------------------------------------------------------------------------- the comparison --
def against_definition(tex, data, chunks, gran, pitch, log2, window, header, modelled=None, what=""):
    """One texture of a frame (textures_of) against the definition.  header: the table's four bytes, None where the road
    writes no table.  modelled: how many fragments from the first to hold to the definition (all by default); the
    others' sizes are taken from the table."""
    size = 1 << log2
    cb = len(data) // chunks
    assert tex["type"] >> 4 == 0xC and len(tex["chunks"]) == chunks and bytes(tex["codecs"]) == bytes([0x0B] * chunks), \
        (what, hex(tex["type"]), bytes(tex["codecs"]))
    per_chunk = -(-cb // size)
    sizes = None
    if header is None:
        assert tex["table"] is None, what
    else:
        assert tex["table"] is not None and bytes(tex["table"][1]) == bytes(header), (what, tex["table"] and bytes(tex["table"][1]))
        sizes = fragment_sizes(tex["table"], chunks * per_chunk)
    for c in range(chunks):
        chunk = data[c * cb: (c + 1) * cb]
        got = tex["chunks"][c]
        prefix = M.varint(cb)
        assert got[: len(prefix)] == prefix, (what, c)
        at = len(prefix)
        for j in range(per_chunk):
            f = c * per_chunk + j
            if modelled is not None and f >= modelled:
                break
            piece = chunk[j * size: (j + 1) * size]
            want = M.modelled(piece, gran, pitch, window)[1]
            have = got[at: at + len(want)]
            if have != want:
                bad = next((i for i in range(min(len(have), len(want))) if have[i] != want[i]), min(len(have), len(want)))
                made = 0
                for el in M.stream_elements(want):
                    if el.pos + el.hdr + (el.n if el.form.startswith("lit") else 0) > bad:
                        break
                    made += el.n
                raise AssertionError("%s: chunk %d differs at stream byte %d: fragment %d, byte %d of its stream, tile %d "
                                     "(output byte %d of the fragment); want %s, got %s"
                                     % (what, c, at + bad, f, bad, made // M.tile_bytes(gran), made,
                                        want[bad: bad + 8].hex(), have[bad: bad + 8].hex()))
            if sizes is not None:
                assert sizes[f] == len(want), (what, f, sizes[f], len(want))
            at += len(want)
        else:
            assert at == len(got), (what, c, at, len(got))
    if sizes is not None:
        for c in range(chunks):
            assert sum(sizes[c * per_chunk: (c + 1) * per_chunk]) + len(M.varint(cb)) == len(tex["chunks"][c]), (what, c)


def encode(hap, ctx, textures, formats, chunks, flags, batch=1):
    caps = hap.HapMaxEncodedLength([len(t) for t in textures], formats, chunks) + 65536
    outs = [np.zeros(caps, dtype=np.uint8) for _ in range(batch)]
    r, used, res = ctx.encode_frames([list(textures)] * batch, formats, [L.COMP_SNAPPY] * len(formats), chunks, outs, flags=flags)
    assert r == 0 and res == [0] * batch, (r, res)
    return [outs[i][: used[i]].tobytes() for i in range(batch)]


def decodes_everywhere(ctx, frame, textures, formats):
    n0 = ctx.table_fallbacks()
    for index, (data, fmt) in enumerate(zip(textures, formats)):
        for name, api in CHECKERS:
            assert api.decode(frame, index, len(data)) == (0, data, fmt), name
        dec = np.zeros(len(data), dtype=np.uint8)
        r, used, dfmt, res = ctx.decode_frames([frame], [len(frame)], index, [dec])
        assert (r, used, dfmt, res) == (0, [len(data)], [fmt], [0])
        assert dec.tobytes() == data
    assert ctx.table_fallbacks() == n0


def run_road(hap, ctx, data, fmt, gran, pitch, log2, window, header, flags, chunks=1, modelled=None, what=""):
    frame, = encode(hap, ctx, [data], [fmt], [chunks], flags)
    tex, = textures_of(frame)
    against_definition(tex, data, chunks, gran, pitch, log2, window, header, modelled, what)
    decodes_everywhere(ctx, frame, [data], [fmt])
    # a second time, three to a batch: the same bytes whatever the wave timing and the place in the batch
    assert encode(hap, ctx, [data], [fmt], [chunks], flags, batch=3) == [frame] * 3, what


# --------------------------------------------------------------------------------------------------------- roads --
# name: (context, format, flags, GRAN, pitch, fragment log2, the table's header)
INDEX, COARSE, SMALLER = 1, 2, 4
ROADS = {
    "bc7": ("default", L.FMT_BC7, INDEX, 2, 16, 13, [1, 13, 1, 0]),
    "bc6h": ("default", L.FMT_BC6U, INDEX, 2, 16, 13, [1, 13, 1, 0]),
    "rgtc1": ("default", L.FMT_RGTC1, INDEX, 2, 8, 13, [1, 13, 1, 0]),
    "coarse-dxt5": ("default", L.FMT_DXT5, INDEX | COARSE, 4, 16, 13, [1, 13, 2, 0]),
    "coarse-rgtc1": ("default", L.FMT_RGTC1, INDEX | COARSE, 4, 8, 13, [1, 13, 2, 0]),
    "bytes-bc7": ("bytes", L.FMT_BC7, INDEX, 1, 16, 13, [1, 13, 0, 0]),
    "bytes-rgtc1": ("bytes", L.FMT_RGTC1, INDEX, 1, 8, 13, [1, 13, 0, 0]),
    "1k-bc7": ("1k", L.FMT_BC7, INDEX, 2, 16, 10, [1, 10, 1, 0]),
    "1k-dxt1": ("1k", L.FMT_DXT1, INDEX, 4, 8, 10, [1, 10, 2, 0]),
}


def test_flag_values(hap):
    assert (hap.ENCODE_FRAGMENT_INDEX, hap.ENCODE_COARSE_MATCHES, hap.ENCODE_SMALLER_FILES) == (INDEX, COARSE, SMALLER)


@pytest.mark.parametrize("road", sorted(ROADS))
def test_every_sweep_comes_out_as_the_definition_writes_it(hap, contexts, road):
    kind, fmt, flags, gran, pitch, log2, header = ROADS[road]
    data, _cases = M.texture(gran, pitch, log2)
    if road == "coarse-rgtc1":
        # whole 8-byte blocks under COARSE_MATCHES go to the block-per-lane kernel ([4, 4] fields); a plane whose
        # size is 4 mod 8 stays with positions per lane
        data += M.filler(4, 1)
    run_road(hap, contexts(kind), data, fmt, gran, pitch, log2, None, header, flags, what=road)


@pytest.mark.parametrize("road", ["bc7", "rgtc1", "coarse-dxt5", "bytes-bc7", "1k-bc7"])
def test_short_last_fragments(hap, contexts, road):
    """16 and 48 bytes, a tile and a supertile less and more a granule behind a full fragment: the loads' ragged end
    (sizes that are no multiple of 16), tiles and supertiles that the data ends in"""
    kind, fmt, flags, gran, pitch, log2, header = ROADS[road]
    for name, data in M.sweep_ends(gran, pitch, 1 << log2):
        run_road(hap, contexts(kind), data, fmt, gran, pitch, log2, None, header, flags, what="%s %s" % (road, name))


@pytest.mark.parametrize("road", ["rgtc1", "bytes-rgtc1", "1k-dxt1"])
def test_a_chunk_that_begins_at_8_mod_16_is_loaded_byte_by_byte_to_the_same_stream(hap, contexts, road):
    kind, fmt, flags, gran, pitch, log2, header = ROADS[road]
    data, chunk = M.unaligned_texture(gran, pitch)
    assert chunk % 16 == 8 and len(data) == 2 * chunk
    run_road(hap, contexts(kind), data, fmt, gran, pitch, log2, None, header, flags, chunks=2, what=road)


def test_rgtc1_as_the_second_texture_beside_the_field_kernel(hap, contexts):
    """Hap Q Alpha: the YCoCg texture goes to the block-per-lane kernel (a version-4 table), the RGTC1 plane to the
    position-per-lane kernel at blockIdx.y = 1"""
    ctx = contexts("default")
    alpha, _cases = M.texture(2, 8, 13)
    colour = M.filler(2 * len(alpha), 5)
    formats = [L.FMT_YCOCG, L.FMT_RGTC1]
    frames = encode(hap, ctx, [colour, alpha], formats, [1, 1], INDEX) + encode(hap, ctx, [colour, alpha], formats, [1, 1], INDEX, batch=3)
    first, second = textures_of(frames[0])
    assert first["table"] is not None and first["table"][0] == 4 and bytes(first["codecs"]) == b"\x0b"
    against_definition(second, alpha, 1, 2, 8, 13, None, [1, 13, 1, 0], what="second texture")
    decodes_everywhere(ctx, frames[0], [colour, alpha], formats)
    assert frames[1:] == [frames[0]] * 3


@pytest.mark.parametrize("how", ["context", "smaller-files"])
def test_fragments_of_64_kib(hap, contexts, how):
    """The dynamic-LDS instantiation at its largest, offsets beyond 32768 among the cases: through
    set_fragment_log2(16) with its table, and through HAPGPU_ENCODE_SMALLER_FILES, which writes none"""
    gran, pitch, log2, _w = M.BIG
    data, _cases = M.texture(gran, pitch, log2, None, ("lengths", "offsets"))
    if how == "context":
        run_road(hap, contexts("64k"), data, L.FMT_BC7, gran, pitch, log2, None, [1, 16, 1, 0], INDEX, what=how)
    else:
        run_road(hap, contexts("default"), data, L.FMT_BC7, gran, pitch, log2, None, None, INDEX | SMALLER, what=how)


def test_the_3_kib_window_of_large_textures(hap, contexts):
    """A BC7 texture of exactly 1 MiB: hash candidates further back than 3072 bytes are not taken, the table says so;
    the fragments that hold cases are held to the definition, the filler behind them need only decode"""
    data, held = M.texture(2, 16, 13, M.WINDOW, total=1 << 20)
    assert len(data) == 1 << 20
    run_road(hap, contexts("default"), data, L.FMT_BC7, 2, 16, 13, M.WINDOW, [1, 13, 1, 12], INDEX, modelled=held, what="window")

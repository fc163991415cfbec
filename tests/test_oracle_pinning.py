"""Pins the CPU oracle (oracle/*.c) before anything trusts it:

  * against the committed golden vectors captured from the unmodified reference
    (tests/golden/hap_golden.json), and
  * against the reference's answers (oracle/_ref/libhap_ref.so + libsnappy 1.1.8)
    over swept formats / chunk counts / data kinds and malformed frames: recorded
    as digests in tests/golden/reference_answers.json, and asked of the live
    library as well wherever it is built.

CPU only.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _data as D
import _libs as L

ORA = L.oracle_api()
REF = L.recorded_reference()


# ---------------------------------------------------------------- golden ----
@pytest.mark.parametrize("v", D.golden_vectors("frame"), ids=lambda v: v["name"])
def test_golden_frames(v):
    tex = [bytes.fromhex(t) for t in v["textures"]]
    assert ORA.max_encoded_length([len(t) for t in tex], v["formats"], v["chunks"]) == v["max_encoded_length"]
    r, frame = ORA.encode(tex, v["formats"], v["compressors"], v["chunks"])
    assert r == v["result"]
    if v["frame"] is None:
        return
    assert frame.hex() == v["frame"]
    assert list(ORA.texture_count(frame)) == v["texture_count"]
    for idx, d in enumerate(v["decode"]):
        dr, out, fmt = ORA.decode(frame, idx, out_bytes=max(len(t) for t in tex) + 64)
        assert (dr, fmt, ORA.callback_calls) == (d["result"], d["format"], d["callback_calls"])
        assert (out == tex[idx]) == d["equals_input"]
        assert list(ORA.chunk_count(frame, idx)) == d["chunk_count"]
        assert list(ORA.texture_format(frame, idx)) == d["texture_format"]


@pytest.mark.parametrize("v", D.golden_vectors("snappy"), ids=lambda v: v["name"])
def test_golden_snappy_compress(v):
    data = bytes.fromhex(v["input"])
    comp = D.osnappy_compress(data)
    assert comp.hex() == v["compressed"]
    assert D.osnappy_uncompress(comp, len(data)) == (0, data)


@pytest.mark.parametrize("v", D.golden_vectors("snappy_stream"), ids=lambda v: v["name"])
def test_golden_snappy_streams(v):
    r, out = D.osnappy_uncompress(bytes.fromhex(v["stream"]), v["capacity"])
    assert r == v["result"]
    assert (out.hex() if out is not None else None) == v["output"]


# ------------------------------------------------------- live reference ----
# REF answers what the unmodified reference answers: recorded digests (tests/golden/reference_answers.json), checked
# against the live library wherever oracle/_ref is built.  Where the oracle's answer is needed as bytes (a frame to
# corrupt, a stream to decode), the oracle's own answer is used once its digest equals the reference's.
DATA_KINDS = ["zero", "random", "mixed", "runs"]
H = L.digest


@pytest.mark.parametrize("kind", DATA_KINDS)
@pytest.mark.parametrize("n", [0, 1, 14, 15, 16, 17, 255, 4096, 65535, 65536, 65537, 200001])
def test_snappy_compress_byte_identical(kind, n):
    data = D.stream_bytes(n, kind, seed=n + 1)
    assert H(D.osnappy_compress(data)) == REF.ask("snappy_compress", data)


def test_snappy_compress_dxt_like_byte_identical():
    img = D.rgba(256, 128)
    for fmt in (L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1):
        tex = D.oracle_bc_encode(img, fmt)
        assert H(D.osnappy_compress(tex)) == REF.ask("snappy_compress", tex)


def test_snappy_uncompress_agrees_on_corruption():
    rng = np.random.default_rng(7)
    data = D.stream_bytes(6000, "runs")
    base = D.osnappy_compress(data)
    assert H(base) == REF.ask("snappy_compress", data)
    for trial in range(300):
        s = bytearray(base)
        mode = trial % 3
        if mode == 0:
            s[rng.integers(0, len(s))] ^= 1 << rng.integers(0, 8)
        elif mode == 1:
            s = s[: rng.integers(0, len(s))]
        else:
            i = rng.integers(0, len(s))
            s[i:i] = bytes(rng.integers(0, 256, 3, dtype=np.uint8))
        assert H(D.osnappy_uncompress(s, 8192)) == REF.ask("snappy_uncompress", bytes(s), 8192), (trial, mode)


def _frames_for_sweep():
    cases = []
    for fmt in L.ALL_FORMATS:
        for chunks in (1, 2, 3, 7, 8):
            for kind in DATA_KINDS:
                cases.append((fmt, chunks, kind, 16 * 96))
    cases += [(L.FMT_YCOCG, 24, "runs", 16 * 24 * 50), (L.FMT_DXT1, 64, "mixed", 8 * 64 * 300)]
    return cases


def _decode(api, frame, index, out_bytes):
    """(result, texture, format, callback calls) of one decode: REF.ask("decode", ...)'s shape"""
    return tuple(api.decode(frame, index, out_bytes)) + (api.callback_calls,)


@pytest.mark.parametrize("fmt,chunks,kind,nbytes", _frames_for_sweep())
def test_frames_byte_identical_to_reference(fmt, chunks, kind, nbytes):
    tex = D.stream_bytes(nbytes, kind, seed=chunks * 131 + fmt)
    for comp in (L.COMP_NONE, L.COMP_SNAPPY):
        assert ORA.max_encoded_length([nbytes], [fmt], [chunks]) == REF.ask("max_encoded_length", [nbytes], [fmt], [chunks])
        ro, fo = ORA.encode([tex], [fmt], [comp], [chunks])
        assert H((ro, fo)) == REF.ask("encode", [tex], [fmt], [comp], [chunks])
        fr = fo                                                   # == the reference's frame (digest above)
        assert H(_decode(ORA, fr, 0, nbytes)) == REF.ask("decode", fr, 0, nbytes)
        assert H(ORA.chunk_count(fr, 0)) == REF.ask("chunk_count", fr, 0)
        # output buffer one byte short
        assert ORA.decode(fr, 0, nbytes - 1)[0] == REF.ask("decode", fr, 0, nbytes - 1)[0]


def test_dual_texture_and_inspectors():
    a = D.stream_bytes(16 * 64, "runs")
    b = D.stream_bytes(8 * 64, "mixed")
    for comps in ([1, 1], [0, 1], [1, 0]):
        for chunks in ([1, 1], [4, 2], [5, 64]):
            ro, fo = ORA.encode([a, b], [L.FMT_YCOCG, L.FMT_RGTC1], comps, chunks)
            assert H((ro, fo)) == REF.ask("encode", [a, b], [L.FMT_YCOCG, L.FMT_RGTC1], comps, chunks) and ro == 0
            fr = fo
            assert H(ORA.texture_count(fr)) == REF.ask("texture_count", fr) == [0, 2]
            for idx in (0, 1, 2):
                assert H(ORA.decode(fr, idx, 4096)) == REF.ask("decode", fr, idx, 4096)[:3]
                assert H(ORA.texture_format(fr, idx)) == REF.ask("texture_format", fr, idx)
                assert H(ORA.chunk_count(fr, idx)) == REF.ask("chunk_count", fr, idx)


def test_bad_arguments_match():
    tex = bytes(64)
    for args in [([tex], [0x1234], [1], [1]), ([tex], [L.FMT_DXT1], [2], [1]), ([tex], [L.FMT_DXT1], [1], [0]),
                 ([tex, tex, tex], [L.FMT_YCOCG] * 3, [1] * 3, [1] * 3)]:
        assert ORA.encode(*args, out_bytes=4096)[0] == REF.ask("encode", *args, 4096)[0]
    # output buffer below the worst case for the compressor -> Buffer_Too_Small before any work
    assert ORA.encode([tex], [L.FMT_DXT1], [1], [1], out_bytes=80)[0] == REF.ask("encode", [tex], [L.FMT_DXT1], [1], [1], 80)[0] == L.R_TOO_SMALL
    assert ORA.max_encoded_length([64], [L.FMT_DXT1], [0]) == REF.ask("max_encoded_length", [64], [L.FMT_DXT1], [0]) == 0


def test_malformed_frames_match():
    """Truncations and payload corruptions. (Size-table corruptions that make the
    reference read out of bounds -- hap.c:798-809 has no bounds check -- are
    exercised only against the hardened product, not against the reference.)"""
    rng = np.random.default_rng(3)
    tex = D.stream_bytes(16 * 256, "runs")
    r, frame = ORA.encode([tex], [L.FMT_DXT5], [1], [4])
    assert H((r, frame)) == REF.ask("encode", [tex], [L.FMT_DXT5], [1], [4])
    hdr = 4 + 4 + 5 * 4 + 8
    for cut in list(range(0, hdr + 4)) + [len(frame) - 1, len(frame) - 7]:
        f = frame[:cut]
        assert ORA.decode(f, 0, 8192)[0] == REF.ask("decode", f, 0, 8192)[0], cut
        assert H(ORA.texture_count(f)) == REF.ask("texture_count", f)
        assert H(ORA.chunk_count(f, 0)) == REF.ask("chunk_count", f, 0)
    for trial in range(200):
        f = bytearray(frame)
        i = int(rng.integers(hdr, len(f)))
        f[i] ^= 1 << int(rng.integers(0, 8))
        assert H(ORA.decode(f, 0, 8192)) == REF.ask("decode", f, 0, 8192)[:3], (trial, i)
    for byte3 in range(256):       # every top-level type byte
        f = bytearray(frame)
        f[3] = byte3
        if (byte3 >> 4) == 0xB:    # reference would parse the tables as a raw Snappy stream: still in-bounds
            pass
        assert ORA.decode(f, 0, 8192)[0] == REF.ask("decode", f, 0, 8192)[0], byte3
        assert H(ORA.texture_format(f, 0)) == REF.ask("texture_format", f, 0)
        assert H(ORA.chunk_count(f, 0)) == REF.ask("chunk_count", f, 0)


# ------------------------------------------------- block layouts vs Pillow ----
def _pin_images():
    rng = np.random.default_rng(5)
    extremes = np.zeros((16, 16, 4), dtype=np.uint8)
    extremes[:4] = 255
    extremes[4:8, :8] = (255, 0, 0, 0)
    extremes[4:8, 8:] = (0, 0, 255, 255)
    extremes[8:12, ::2] = (10, 200, 30, 128)
    extremes[12:, :, 3] = np.arange(16, dtype=np.uint8) * 17
    return [D.rgba(256, 64, frame=4), D.rgba(512, 512, frame=1), rng.integers(0, 256, (32, 64, 4), dtype=np.uint8), extremes]


@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5, L.FMT_RGTC1])
def test_block_layouts_against_pillow(fmt):
    """the reference has no block encoder, so oracle/bc_oracle.c defines the algorithm -- but the block
    LAYOUT (endpoint order, index bit order, interpolants) is external (S3TC, RGTC).  Pillow's DDS reader decodes the
    oracle encoder's blocks, and random blocks, to exactly what the oracle's own decoders say, and close to the source."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(6)
    for img in _pin_images():
        h, w = img.shape[:2]
        blocks = D.oracle_bc_encode(img, fmt)
        mine = D.oracle_bc_decode(blocks, fmt, w, h)
        theirs = D.pillow_bc_decode(blocks, fmt, w, h)
        assert theirs.shape == mine.shape and np.array_equal(theirs, mine)
    # quality measured with the third-party decoder only
    pic = D.rgba(512, 512, frame=1)
    dec = D.pillow_bc_decode(D.oracle_bc_encode(pic, fmt), fmt, 512, 512)
    if fmt == L.FMT_RGTC1:
        assert D.psnr(dec, pic[..., 3]) > 40.0
    else:
        assert D.psnr(dec[..., :3], pic[..., :3]) > 30.0
    if fmt == L.FMT_DXT5:
        assert D.psnr(dec[..., 3], pic[..., 3]) > 40.0
    # random blocks: both endpoint orders (DXT1's 3-colour + transparent mode, the 6-interpolant alpha mode)
    w, h = 128, 64
    blocks = rng.integers(0, 256, (w // 4) * (h // 4) * D.BLOCK_BYTES[fmt], dtype=np.uint8).tobytes()
    mine, theirs = D.oracle_bc_decode(blocks, fmt, w, h), D.pillow_bc_decode(blocks, fmt, w, h)
    if fmt == L.FMT_DXT1:
        # transparent-black texels of the 3-colour mode: Hap1 is opaque RGB, the oracle keeps alpha 255 there
        assert np.array_equal(theirs[..., :3], mine[..., :3])
    else:
        assert np.array_equal(theirs, mine)


# dB of the shipped definition (oracle/bc_oracle.c) on tests/_data.quality_images(), measured in round 4; the floors of the
# tests are these minus 0.3 dB: the definition cannot drift (it was changed three times in one round
# under floors of 30 / 33 / 40 dB)
QUALITY_R04 = {
    ("smooth", L.FMT_DXT1): (43.943,), ("smooth", L.FMT_DXT5): (43.943, 99.0), ("smooth", L.FMT_YCOCG): (46.525,), ("smooth", L.FMT_RGTC1): (99.0,),
    ("noisy", L.FMT_DXT1): (30.824,), ("noisy", L.FMT_DXT5): (30.824, 47.157), ("noisy", L.FMT_YCOCG): (33.461,), ("noisy", L.FMT_RGTC1): (47.157,),
    ("hard_edge", L.FMT_DXT1): (19.775,), ("hard_edge", L.FMT_DXT5): (19.775, 39.153), ("hard_edge", L.FMT_YCOCG): (27.183,), ("hard_edge", L.FMT_RGTC1): (39.153,),
}


@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1])
def test_block_encoder_quality_is_pinned(fmt):
    """The reference has no block encoder (parity unpinned by the reference), so oracle/bc_oracle.c DEFINES
    it -- and a definition that may change needs a quality floor that notices: within 0.3 dB of the recorded values on
    three fixed pictures (smooth, noisy, hard edges), every format, colour and alpha separately."""
    for name, img in D.quality_images().items():
        got = D.block_quality(D.oracle_bc_encode(img, fmt), fmt, img)
        want = QUALITY_R04[(name, fmt)]
        assert len(got) == len(want)
        for g, w_ in zip(got, want):
            assert g >= w_ - 0.3, (name, fmt, got, want)


def test_projection_indices_stay_close_to_the_exhaustive_search(tmp_path):
    """The shipped definition picks colour indices by projection and ramp positions by one multiply-add (what fast
    real-time encoders do); -DOBC_EXACT_NEAREST builds the same file with the exhaustive nearest-of-4 / nearest-of-8
    searches.  The shortcut may cost at most 0.3 dB anywhere (measured r04: 0.23 dB on the pure gradient's colour,
    under 0.03 dB on every other picture and plane) and never more than 0.1 dB on noisy or hard-edged content."""
    import subprocess
    so = str(tmp_path / "bc_exact.so")
    src = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "oracle", "bc_oracle.c")
    try:
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-DOBC_EXACT_NEAREST", "-o", so, src], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except (OSError, subprocess.CalledProcessError):
        pytest.skip("no C compiler")
    exact = C.CDLL(so)

    def encode_exact(img, fmt):
        h, w = img.shape[:2]
        out = np.zeros((h // 4) * (w // 4) * D.BLOCK_BYTES[fmt], dtype=np.uint8)
        fn = getattr(exact, D._ORACLE_BC[fmt])
        fn.restype = None
        fn(img.ctypes.data_as(C.c_void_p), C.c_uint(w), C.c_uint(h), C.c_size_t(img.strides[0]), out.ctypes.data_as(C.c_void_p))
        return out.tobytes()
    for name, img in D.quality_images().items():
        for fmt in (L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1):
            shipped = D.block_quality(D.oracle_bc_encode(img, fmt), fmt, img)
            best = D.block_quality(encode_exact(img, fmt), fmt, img)
            for a, b in zip(shipped, best):
                assert a >= b - (0.3 if name == "smooth" else 0.1), (name, fmt, shipped, best)


def test_ycocg_blocks_are_dxt5_blocks_a_hap_q_shader_reconstructs():
    """Scaled YCoCg-DXT5: Pillow reads the oracle encoder's blocks as plain DXT5 (Co, Cg, scale code, Y), numpy applies the
    shader arithmetic of the YCoCg-DXT paper -> the picture comes back (PSNR) and agrees with the oracle's integer
    decoder within rounding."""
    pytest.importorskip("PIL")
    for img in _pin_images()[:2]:
        h, w = img.shape[:2]
        blocks = D.oracle_bc_encode(img, L.FMT_YCOCG)
        tex = D.pillow_bc_decode(blocks, L.FMT_YCOCG, w, h)
        assert set(np.unique(tex[..., 2])) <= {0, 8, 24}                       # (scale - 1) * 8, scale in {1, 2, 4}
        rgb = D.shader_ycocg_to_rgb(tex)
        assert D.psnr(rgb, img[..., :3]) > 33.0
        mine = D.oracle_bc_decode(blocks, L.FMT_YCOCG, w, h)
        assert np.abs(rgb.astype(int) - mine[..., :3].astype(int)).max() <= 2


# ---- the scalar definition of the GPU's block compressor (oracle/field_stream_oracle.c) ----
@pytest.mark.parametrize("fmt,layout,block", [(L.FMT_YCOCG, 4, 16), (L.FMT_DXT5, 4, 16), (L.FMT_DXT1, 2, 8), (L.FMT_RGTC1, 6, 8),
                                              (L.FMT_YCOCG, 8, 16)])      # (layout 8: opaque 16-byte blocks as four dwords)
def test_field_stream_definition_is_snappy_and_keeps_its_promises(fmt, layout, block):
    """What ofs_compress_fragment writes is an ordinary Snappy stream (libsnappy and the restatement decode it to the
    input) that keeps the promises of the fragment table version 4: the group bytes add up (compressed and produced), every group holds the same
    number of elements (the last ones fewer), no element crosses a 128-byte half-tile, elements start on field
    boundaries, copies reach back whole blocks inside the fragment, literal runs use at most one length byte."""
    o = L.oracle_lib()
    o.ofs_compress_fragment.restype = C.c_uint
    tex = D.oracle_bc_encode(D.rgba(1024, 512, frame=9), fmt)
    starts = {4: (0, 2, 8, 12), 2: (0, 4), 6: (0, 2), 8: (0, 4, 8, 12)}[layout]
    rng = np.random.default_rng(7)
    sizes = [8192, 8192, 8192, 8192, 4096, 1024 + 3 * block, block, 8192 - block, 128, 128 + block]
    total_in = total_out = 0
    for trial, n in enumerate(sizes * 3):
        at = int(rng.integers(0, (len(tex) - n) // block)) * block
        data = tex[at: at + n]
        out = (C.c_ubyte * (8192 + 512))()
        table = (C.c_ubyte * 196)()
        m = o.ofs_compress_fragment(data, C.c_uint(n), C.c_uint(layout), C.c_uint(0 if trial % 2 else 3072), out, table)
        stream = bytes(out[:m])
        entries = [int.from_bytes(bytes(table[3 * g: 3 * g + 3]), "little") for g in range(64)]
        groups = [e & 0xFFF for e in entries]
        made = [e >> 12 for e in entries]
        elements = int.from_bytes(bytes(table[192:194]), "little")
        assert sum(groups) == m and m <= n + n // 32 + 64 and sum(made) == n and bytes(table[194:196]) == bytes(2)
        head = bytearray()
        v = n
        while v >= 128:
            head.append((v & 127) | 128)
            v >>= 7
        head.append(v)
        assert D.osnappy_uncompress(bytes(head) + stream, n) == (0, data)
        assert REF.ask("snappy_uncompress", bytes(head) + stream, n) == H((0, data))
        q = produced = 0
        counts = []
        for g in range(64):
            end, count = q + groups[g], 0
            assert produced == sum(made[:g])
            while q < end:
                tag = stream[q]
                kind = tag & 3
                assert (produced % 128) % block in starts
                if kind == 0:
                    ln, hd = (tag >> 2) + 1, 1
                    assert ln <= 61
                    if ln == 61:
                        ln, hd = stream[q + 1] + 1, 2
                        assert ln > 60
                    q += hd + ln
                else:
                    assert kind in (1, 2)
                    ln = 4 + ((tag >> 2) & 7) if kind == 1 else (tag >> 2) + 1
                    off = ((tag >> 5) << 8) | stream[q + 1] if kind == 1 else stream[q + 1] | (stream[q + 2] << 8)
                    assert off % block == 0 and block <= off <= produced
                    if trial % 2 == 0:
                        assert off <= 3072
                    q += 1 + kind
                assert produced // 128 == (produced + ln - 1) // 128          # inside one half-tile
                produced += ln
                count += 1
            assert q == end
            counts.append(count)
        assert q == m and produced == n and sum(counts) == elements
        per_group = (sum(counts) + 63) // 64
        full = sum(counts) // per_group
        assert counts[:full] == [per_group] * full and sum(counts[full + 1:]) == 0
        total_in += n
        total_out += m
    assert total_out < total_in

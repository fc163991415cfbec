"""CPU-side checks of the product library (no compute calls: there is no GPU here):
the C ABI loads, exports every symbol include/*.h declares, and the host-only functions
(size arithmetic, frame inspectors) agree with the oracle / golden vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _data as D
import _libs as L

ROOT = L.ROOT


def _declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(Hap[A-Za-z0-9]+)\s*\(", text)) - {"HapDecodeWorkFunction", "HapDecodeCallback"})


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_every_declared_symbol_is_exported(hap):
    lib = C.CDLL(os.path.join(ROOT, "hap_amd", "libhap_amd.so"))
    names = _declared_functions("hap.h") + _declared_functions("hap_gpu.h") + _declared_functions("hap_sequence.h")
    assert len(names) >= 31
    for n in names:
        assert hasattr(lib, n), n
    for n in ("HapMaxEncodedLength", "HapEncode", "HapDecode", "HapGetFrameTextureCount",
              "HapGetFrameTextureFormat", "HapGetFrameTextureChunkCount"):
        assert n in names


def test_enum_values_match_reference_abi(hap):
    hdr = open(os.path.join(ROOT, "include", "hap.h")).read()
    for name, val in [("HapTextureFormat_RGB_DXT1", 0x83F0), ("HapTextureFormat_RGBA_DXT5", 0x83F3),
                      ("HapTextureFormat_YCoCg_DXT5", 0x01), ("HapTextureFormat_A_RGTC1", 0x8DBB),
                      ("HapTextureFormat_RGBA_BPTC_UNORM", 0x8E8C), ("HapTextureFormat_RGB_BPTC_UNSIGNED_FLOAT", 0x8E8F),
                      ("HapTextureFormat_RGB_BPTC_SIGNED_FLOAT", 0x8E8E), ("HapCompressorNone", 0), ("HapCompressorSnappy", 1),
                      ("HapResult_No_Error", 0), ("HapResult_Bad_Arguments", 1), ("HapResult_Buffer_Too_Small", 2),
                      ("HapResult_Bad_Frame", 3), ("HapResult_Internal_Error", 4)]:
        m = re.search(name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == val, name


def test_max_encoded_length_matches_oracle(hap):
    ora = L.oracle_api()
    rng = np.random.default_rng(0)
    for _ in range(300):
        count = int(rng.integers(1, 3))
        lengths = [int(rng.integers(1, 1 << 22)) * 8 for _ in range(count)]
        fmts = [int(rng.choice(L.ALL_FORMATS)) for _ in range(count)]
        chunks = [int(rng.integers(1, 200)) for _ in range(count)]
        assert hap.HapMaxEncodedLength(lengths, fmts, chunks) == ora.max_encoded_length(lengths, fmts, chunks)
    assert hap.HapMaxEncodedLength([64], [L.FMT_DXT1], [0]) == 0
    assert hap.HapMaxEncodedLength([], [], []) == 0
    # BASELINE configs
    assert hap.HapMaxEncodedLength([33177600], [L.FMT_YCOCG], [24]) == ora.max_encoded_length([33177600], [L.FMT_YCOCG], [24])
    assert hap.HapMaxEncodedLength([268435456, 134217728], [L.FMT_YCOCG, L.FMT_RGTC1], [64, 64]) == \
        ora.max_encoded_length([268435456, 134217728], [L.FMT_YCOCG, L.FMT_RGTC1], [64, 64])


def test_inspectors_on_golden_and_malformed_frames(hap):
    ora = L.oracle_api()
    frames = [bytes.fromhex(v["frame"]) for v in D.golden_vectors("frame") if v["frame"]]
    rng = np.random.default_rng(1)
    for frame in frames:
        variants = [frame] + [frame[:k] for k in range(1, min(len(frame), 40))]
        for _ in range(40):
            f = bytearray(frame)
            f[int(rng.integers(0, min(len(f), 48)))] = int(rng.integers(0, 256))
            variants.append(bytes(f))
        for f in variants:
            assert hap.HapGetFrameTextureCount(f) == ora.texture_count(f)
            for idx in (0, 1, 2):
                assert hap.HapGetFrameTextureFormat(f, idx) == ora.texture_format(f, idx)
                assert hap.HapGetFrameTextureChunkCount(f, idx) == ora.chunk_count(f, idx)


@pytest.mark.timeout(30)
def test_section_lengths_that_wrap_32_bits_are_rejected(hap):
    """Hardening beyond the reference (hap.c:160-181 adds header + length in 32 bits): a section length of
    0xFFFFFFF8 and more used to wrap the bound check -- the texture counter then never advanced (a hang) and the
    planner accepted a 4 GiB section over a 16-byte frame."""
    huge = (0xFFFFFFF8).to_bytes(4, "little")
    # top: multi-image section, 16 bytes of payload; inside: an 8-byte header announcing 0xFFFFFFF8 bytes
    f1 = (16).to_bytes(3, "little") + b"\x0d" + b"\0\0\0\xcf" + huge + bytes(8)
    assert len(f1) == 20
    assert hap.HapGetFrameTextureCount(f1)[0] == hap.HapResult.Bad_Frame
    assert hap.HapGetFrameTextureFormat(f1, 0)[0] == hap.HapResult.Bad_Frame
    assert hap.HapGetFrameTextureChunkCount(f1, 0)[0] == hap.HapResult.Bad_Frame
    assert hap.HapGpuJoinChunkGroups([f1, f1])[0] == hap.HapResult.Bad_Frame
    # a 16-byte frame whose only section claims 0xFFFFFFF9 bytes (raw and Snappy flavours)
    for type_byte in (0xAB, 0xBB, 0xCB):
        f2 = b"\0\0\0" + bytes([type_byte]) + (0xFFFFFFF9).to_bytes(4, "little") + bytes(8)
        assert hap.HapGetFrameTextureCount(f2)[0] == hap.HapResult.Bad_Frame
        assert hap.HapGetFrameTextureChunkCount(f2, 0)[0] == hap.HapResult.Bad_Frame
        assert hap.HapGpuGetFrameTextureChunkLayout(f2, 0)[0] == hap.HapResult.Bad_Frame


def test_sequence_file_round_trip_and_malformed_files(hap, tmp_path):
    """include/hap_sequence.h (no GPU): frames come back byte for byte, the index is validated on open."""
    ora = L.oracle_api()
    frames = [ora.encode([D.stream_bytes(16 * 64 * (5 + i), "mixed", seed=i)], [L.FMT_DXT5], [1], [1 + i % 3])[1] for i in range(9)]
    path = str(tmp_path / "clip.hapseq")
    with hap.SequenceWriter(path, 256, 64, (30000, 1001)) as w:
        for f in frames:
            assert w.append(f) == 0
        assert w.append(b"") == hap.HapResult.Bad_Arguments
    r = hap.SequenceReader(path)
    assert (r.width, r.height, r.rate, r.frame_count) == (256, 64, (30000, 1001), 9)
    assert [r.frame_bytes(i) for i in range(10)] == [len(f) for f in frames] + [0]
    assert r.read(0, 9) == (0, frames) and r.read(4, 3) == (0, frames[4:7]) and r.read(8, 1) == (0, frames[8:])
    assert r.read(8, 2)[0] == hap.HapResult.Bad_Arguments and r.read(9, 1)[0] == hap.HapResult.Bad_Arguments
    r.close()
    raw = open(path, "rb").read()
    assert len(raw) == 64 + sum(map(len, frames)) + 8 * 10 and raw[:8] == b"HAPSEQ1\0"
    # every frame stored exactly as written: the reference inspectors read them straight from the file image
    at = 64
    for f in frames:
        assert raw[at:at + len(f)] == f
        at += len(f)

    def opens(data):
        bad = str(tmp_path / "bad.hapseq")
        open(bad, "wb").write(data)
        try:
            hap.SequenceReader(bad).close()
            return True
        except OSError:
            return False
    assert opens(raw)
    assert not opens(raw[:40]) and not opens(b"NOTASEQ\0" + raw[8:]) and not opens(raw[:-8])       # short / magic / index cut
    patched = bytearray(raw)
    patched[32:40] = (len(raw) + 1).to_bytes(8, "little")                                               # index beyond the file
    assert not opens(bytes(patched))
    patched = bytearray(raw)
    idx = int.from_bytes(raw[32:40], "little")
    patched[idx + 8:idx + 16] = (10).to_bytes(8, "little")                                              # offsets out of order
    assert not opens(bytes(patched))
    with pytest.raises(OSError):
        hap.SequenceReader(str(tmp_path / "missing.hapseq"))
    with hap.SequenceWriter(str(tmp_path / "empty.hapseq")) as w:
        pass
    e = hap.SequenceReader(str(tmp_path / "empty.hapseq"))
    assert e.frame_count == 0 and e.read(0, 1)[0] == hap.HapResult.Bad_Arguments


def _checkers():
    ref = L.ref_api()
    return [L.oracle_api()] + ([ref] if ref is not None else [])


@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5, L.FMT_YCOCG, L.FMT_RGTC1, L.FMT_BC7])
@pytest.mark.parametrize("groups", [1, 2, 5])
def test_join_chunk_groups_is_a_frame_the_reference_decodes(hap, fmt, groups):
    """HapGpuJoinChunkGroups (host-only): band frames made by the checker's encoder join into one
    frame that the checker / reference decodes to the whole texture, with the chunk lists concatenated."""
    ora = L.oracle_api()
    block = 8 if fmt in (L.FMT_DXT1, L.FMT_RGTC1) else 16
    band = block * 64 * 6
    tex = D.stream_bytes(band * groups, "mixed", seed=groups)
    frames = [ora.encode([tex[g * band:(g + 1) * band]], [fmt], [L.COMP_SNAPPY], [3])[1] for g in range(groups)]
    r, joined = hap.HapGpuJoinChunkGroups(frames)
    assert r == 0
    for api in _checkers():
        assert api.decode(joined, 0, len(tex) + 8) == (0, tex, fmt)
        assert api.chunk_count(joined, 0) == (0, 3 * groups)
        assert api.texture_count(joined) == (0, 1)
    r, layout = hap.HapGpuGetFrameTextureChunkLayout(joined, 0)
    assert (r, layout) == (0, [i * (band // 3) for i in range(3 * groups + 1)])
    # a single group joins to a frame with the same content
    if groups == 1:
        assert ora.decode(joined, 0, len(tex)) == ora.decode(frames[0], 0, len(tex))


def test_join_chunk_groups_mixed_storage_dual_texture_and_errors(hap):
    ora = L.oracle_api()
    # bands stored as-is (random), as one chunk, and chunked -> chunk list 1 + 1 + 4, unequal chunk sizes
    a = D.stream_bytes(16 * 64 * 4, "random", seed=1)
    b = D.stream_bytes(16 * 64 * 2, "runs", seed=2)
    c = D.stream_bytes(16 * 64 * 8, "mixed", seed=3)
    frames = [ora.encode([a], [L.FMT_DXT5], [1], [4])[1], ora.encode([b], [L.FMT_DXT5], [1], [1])[1],
              ora.encode([c], [L.FMT_DXT5], [1], [4])[1]]
    assert frames[0][3] >> 4 == 0xA and frames[1][3] >> 4 == 0xC
    r, joined = hap.HapGpuJoinChunkGroups(frames)
    assert r == 0
    for api in _checkers():
        assert api.decode(joined, 0, len(a + b + c)) == (0, a + b + c, L.FMT_DXT5)
        assert api.chunk_count(joined, 0) == (0, 6)
    assert hap.HapGpuGetFrameTextureChunkLayout(joined, 0) == \
        (0, [0, len(a), len(a) + len(b)] + [len(a) + len(b) + (i + 1) * len(c) // 4 for i in range(4)])
    # nothing compressed anywhere -> a plain uncompressed section (hap.c:478-495), byte-identical to the reference's frame
    r, joined = hap.HapGpuJoinChunkGroups([frames[0], ora.encode([a[::-1]], [L.FMT_DXT5], [1], [2])[1]])
    assert r == 0 and joined == ora.encode([a + a[::-1]], [L.FMT_DXT5], [0], [1])[1]
    # two textures per frame (Hap Q Alpha): both joined, outer 0x0D section rebuilt
    y = D.stream_bytes(16 * 256, "runs", seed=4)
    al = D.stream_bytes(8 * 256, "mixed", seed=5)
    duo = [ora.encode([y[g * 2048:(g + 1) * 2048], al[g * 1024:(g + 1) * 1024]], [L.FMT_YCOCG, L.FMT_RGTC1], [1, 1], [2, 2])[1]
           for g in range(2)]
    r, joined = hap.HapGpuJoinChunkGroups(duo)
    assert r == 0 and joined[3] == 0x0D
    for api in _checkers():
        assert api.texture_count(joined) == (0, 2)
        assert api.decode(joined, 0, len(y)) == (0, y, L.FMT_YCOCG)
        assert api.decode(joined, 1, len(al)) == (0, al, L.FMT_RGTC1)
    # errors: disagreeing formats / texture counts, malformed group, small output
    other = ora.encode([b], [L.FMT_DXT1], [1], [1])[1]
    assert hap.HapGpuJoinChunkGroups([frames[1], other])[0] == hap.HapResult.Bad_Frame
    assert hap.HapGpuJoinChunkGroups([frames[1], duo[0]])[0] == hap.HapResult.Bad_Frame
    assert hap.HapGpuJoinChunkGroups([frames[1], frames[2][:40]])[0] != 0
    assert hap.HapGpuJoinChunkGroups([frames[1], frames[2]], outputBufferBytes=100)[0] == hap.HapResult.Buffer_Too_Small
    assert hap.HapGpuJoinChunkGroups([])[0] == hap.HapResult.Bad_Arguments


def test_chunk_layout_on_golden_and_malformed_frames(hap):
    """The layout inspector equals the running sum of decoded chunk sizes (hap.c:794-838): checked against
    what the checker decodes, chunk by chunk, on the golden frames; malformed input never crashes."""
    ora = L.oracle_api()
    rng = np.random.default_rng(2)
    for v in D.golden_vectors("frame"):
        if not v["frame"]:
            continue
        frame = bytes.fromhex(v["frame"])
        for idx in (0, 1):
            rc, n = ora.chunk_count(frame, idx)
            r, layout = hap.HapGpuGetFrameTextureChunkLayout(frame, idx)
            dec = ora.decode(frame, idx, 1 << 20)
            if dec[0] == 0:
                assert r == 0 and layout[0] == 0 and layout[-1] == len(dec[1])
                assert len(layout) == max(1, n) + 1 and layout == sorted(layout)
            elif rc != 0:
                assert r != 0
        for _ in range(60):
            f = bytearray(frame)
            f[int(rng.integers(0, len(f)))] = int(rng.integers(0, 256))
            hap.HapGpuGetFrameTextureChunkLayout(bytes(f), 0)
            hap.HapGpuJoinChunkGroups([bytes(f), frame])
        for k in range(0, min(len(frame), 64)):
            hap.HapGpuGetFrameTextureChunkLayout(frame[:k] or b"\0", 0)


def test_no_gpu_means_loud_failure_not_fallback(hap):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r, frame = hap.HapEncode([bytes(64)], [L.FMT_DXT1], [1], [1])
    assert r == hap.HapResult.Internal_Error and frame is None
    f = bytes.fromhex(D.golden_vectors("frame")[0]["frame"])
    assert hap.HapDecode(f, 0, outputBufferBytes=64)[0] == hap.HapResult.Internal_Error
    with pytest.raises(RuntimeError):
        hap.Context(0)


def test_product_does_not_reference_the_oracle():
    """The oracle is test infrastructure: nothing under hap_amd/ may include, link, load or import it
    (comments that cite oracle/bc_oracle.c as the definition of the block algorithm are fine)."""
    import re
    forbidden = re.compile(r'#\s*include\s*[<"][^>"]*oracle|liboracle|-loracle|-L\S*oracle|dlopen|'
                           r'import\s+_libs|from\s+_libs|import\s+oracle|oracle_lib|osnappy_|ohap_|obc_encode|'
                           r'CDLL\([^)]*oracle')
    for base, _dirs, files in os.walk(os.path.join(ROOT, "hap_amd")):
        if os.path.basename(base) == "build":
            continue
        for name in files:
            if name.endswith((".c", ".h", ".hip", ".py", "Makefile", ".map")):
                text = open(os.path.join(base, name), errors="ignore").read()
                assert not forbidden.search(text), (base, name, forbidden.search(text).group(0))


def test_only_the_public_surface_is_exported():
    """nm -D of the product library: the six hap.h functions, the two link-compatibility symbols the reference object
    also exposes, and the HapGpu* / HapSequence* additions -- not the internal launch ABI (hapgpu_rt_* / hapgpu_k_*)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hap_amd", "libhap_amd.so")], check=True, capture_output=True, text=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if line.strip()]
    stray = [n for n in names if not (n.startswith("HapGpu") or n.startswith("HapSequence") or n in (
        "HapMaxEncodedLength", "HapEncode", "HapDecode", "HapGetFrameTextureCount", "HapGetFrameTextureFormat",
        "HapGetFrameTextureChunkCount", "hap_get_section_at_index", "hap_decode_single_texture"))]
    assert stray == [], stray
    assert "HapEncode" in names and "HapGpuEncodeFrames" in names


# Every environment switch the PRODUCT library reads, and the test that runs with it set.  (Switches that exist for A/B
# measurements only are read through HAP_AB_ENV, which measurement builds alone define: tools/build_variants.sh.)
ENVIRONMENT_SWITCHES = {
    "HAP_AMD_DEVICE": "test_environment_switches_of_plain_hap_h",
    "HAP_AMD_FRAGMENT_INDEX": "test_plain_hap_h_encode_writes_the_private_table_on_request_only",
    "HAP_AMD_COARSE_MATCHES": "test_environment_switches_of_plain_hap_h",
    "HAP_AMD_SMALLER_FILES": "test_environment_switches_of_plain_hap_h",
    "HAP_AMD_FRAGMENT_LOG2": "test_environment_switches_of_plain_hap_h",
    "HAP_AMD_BYTE_GRANULAR": "test_every_fragment_size_round_trips",
    "HAP_AMD_NO_BLOCK_SCAN": "test_environment_switches_of_plain_hap_h",
    "HAP_AMD_GRAPHS": "test_a_chunk_that_does_not_shrink_sends_its_frame_through_slots",
    "HAP_AMD_NO_FUSION": "test_fragments_placed_by_the_compressor_give_the_same_frames",
    "HAP_AMD_NO_PLACING": "test_a_chunk_that_does_not_shrink_sends_its_frame_through_slots",
    "HAP_AMD_PLACING_MIN_FRAMES": "test_a_chunk_that_does_not_shrink_sends_its_frame_through_slots",
    "HAP_AMD_PLACING_HOLDOFF": "test_a_chunk_that_does_not_shrink_sends_its_frame_through_slots",
    "HAP_AMD_LIBRARY": "test_every_environment_switch_is_documented_and_tested",      # (the Python binding's: which build to load)
}


def test_every_environment_switch_is_documented_and_tested():
    """VERDICT r04 / ADVICE r04: no switch ships that is not written down and run.  The sources are searched for
    getenv("HAP_AMD_..."): each name must be in INTEGRATION.md and in the table above, whose tests must exist and must
    mention the switch; what is read through HAP_AB_ENV (measurement builds only) must not also be read plainly."""
    import glob
    import re
    product, measurement = set(), set()
    for path in glob.glob(os.path.join(ROOT, "hap_amd", "csrc", "*.c")) + glob.glob(os.path.join(ROOT, "hap_amd", "csrc", "*.hip")) + \
            glob.glob(os.path.join(ROOT, "hap_amd", "*.py")):
        text = open(path).read()
        product |= set(re.findall(r'(?<![A-Z_])(?:getenv|environ\.get)\(\s*"(HAP_AMD_[A-Z0-9_]+)"', text))
        measurement |= set(re.findall(r'HAP_AB_ENV\(\s*"(HAP_AMD_[A-Z0-9_]+)"', text))
    assert product, "no switch found: the search pattern is broken"
    assert not (product & measurement), product & measurement
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    tests = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "tests", "test_*.py")))
    for name in sorted(product):
        assert name in doc, "%s is not in INTEGRATION.md" % name
        assert name in ENVIRONMENT_SWITCHES, "%s has no test in the table" % name
        test = ENVIRONMENT_SWITCHES[name]
        assert ("def %s(" % test) in tests, (name, test)
        body = tests[tests.index("def %s(" % test):]
        body = body[: body.index("\ndef ", 1) if "\ndef " in body[1:] else len(body)]
        assert name in body or name == "HAP_AMD_LIBRARY", "%s does not mention %s" % (test, name)
    assert set(ENVIRONMENT_SWITCHES) == product, set(ENVIRONMENT_SWITCHES) ^ product


def test_launch_state_is_per_runtime_and_declared_once():
    """VERDICT r06 / ADVICE r06: no mutable function-local static in the native sources (what a launch depends on is a
    setting of its runtime, fixed when the runtime is made), and extern "C" in a .hip file only in front of a function
    definition (what hapgpu_abi.h declares): a hand-copied C prototype links whatever its arguments say."""
    import glob
    import re
    csrc = os.path.join(ROOT, "hap_amd", "csrc")
    statics, prototypes = [], []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.c"))):
        name = os.path.basename(path)
        text = open(path).read()
        for number, line in enumerate(text.splitlines(), 1):
            if re.match(r"^\s+static\s", line) and not re.match(r"^\s+static\s+(const|constexpr|inline)\s", line):
                statics.append("%s:%d" % (name, number))
        if name.endswith(".hip"):
            for m in re.finditer(r'extern\s+"C"', text):
                rest = text[m.end():]
                brace, semicolon = rest.find("{"), rest.find(";")
                if rest.lstrip().startswith("{") or brace < 0 or (0 <= semicolon < brace):
                    prototypes.append("%s:%d" % (name, text.count("\n", 0, m.start()) + 1))
    assert statics == [], statics
    assert prototypes == [], prototypes


def test_round5_entry_points_without_a_gpu(hap):
    """The integer side of the round-5 additions needs no GPU: HapGpuFineChunkCount is hap.c:277-300's limiting of
    bytes / 8 KiB chunks to a divisor of the block count (0 for arguments HapEncode would refuse), and the
    several-context calls and the two-halves calls refuse missing contexts before they touch a device."""
    lib = hap._lib.lib
    u, ul, vp = C.c_uint, C.c_ulong, C.c_void_p
    # 8K Hap Q: 33 177 600 bytes = 4050 x 8 KiB; 4K DXT1: 518 400 blocks, 507 chunks would be 8 KiB each: 540 is the smallest
    # divisor from there up (chunks of 7680 bytes: one fragment each; until r05 the largest divisor BELOW, 480 chunks of 8640
    # bytes, two fragments each -- ADVICE r05); 1080p DXT5: 270, not 240
    assert hap.fine_chunk_count(7680 * 4320, L.FMT_YCOCG) == 4050
    assert hap.fine_chunk_count(3840 * 2160 // 2, L.FMT_DXT1) == 540
    assert hap.fine_chunk_count(1920 * 1080, L.FMT_DXT5) == 270
    for n, fmt in ((16, L.FMT_YCOCG), (8, L.FMT_DXT1), (8192, L.FMT_RGTC1), (8192 + 16, L.FMT_DXT5), (1 << 20, L.FMT_BC7), (16 * 8191, L.FMT_DXT5)):
        k = hap.fine_chunk_count(n, fmt)
        block = D.BLOCK_BYTES[fmt]
        want = (n + 8191) // 8192
        # a divisor of the block count; chunks of at most 8 KiB unless the block count has no divisor up to four times as many
        assert k >= 1 and (n // block) % k == 0 and (want <= k <= 4 * want or (k < want and not any((n // block) % c == 0 for c in range(want, min(4 * want, n // block) + 1))))
        assert hap.HapMaxEncodedLength([n], [fmt], [k]) > 0
    assert hap.fine_chunk_count(0, L.FMT_DXT1) == 0 and hap.fine_chunk_count(4096, 0x1234) == 0
    assert hap.fine_chunk_count(1 << 33, L.FMT_DXT1) == 0
    res = (u * 2)(7, 7)
    used = (ul * 2)()
    one = (vp * 1)(None)
    assert lib.HapGpuEncodeFramesRGBAOnDevices(None, 0, 2, None, 8, 8, 32, 1, None, None, None, None, None, used, res, 0) == hap.HapResult.Bad_Arguments
    assert lib.HapGpuEncodeFramesRGBAOnDevices(one, 1, 2, None, 8, 8, 32, 1, None, None, None, None, None, used, res, 0) == hap.HapResult.Bad_Arguments
    assert lib.HapGpuDecodeFramesOnDevices(None, 3, 2, None, None, 0, None, None, None, None, res, 0) == hap.HapResult.Bad_Arguments
    assert lib.HapGpuEncodeFramesOnDevices(one, 1, 2, 3, None, None, None, None, None, None, None, used, res, 0) == hap.HapResult.Bad_Arguments
    assert list(res) == [hap.HapResult.Bad_Arguments] * 2                       # (count 3: every frame says so)
    assert lib.HapGpuEncodeFramesFinish(None) == hap.HapResult.Bad_Arguments
    assert lib.HapGpuEncodeFramesRGBABegin(None, 1, None, 8, 8, 32, 1, None, None, None, None, None, used, res, 0) == hap.HapResult.Bad_Arguments
    assert lib.HapGpuPlacementTimeoutCount(None) == 0
    assert lib.HapGpuResolvedBlockCount(None) == 0           # (round 6: blocks of other encoders' streams a workgroup decoded)
    assert lib.HapGpuCollectProfileN(None, 9, None, None) == hap.HapResult.Bad_Arguments

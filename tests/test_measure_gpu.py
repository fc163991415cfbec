"""Textures and Hap frames measured against RGBA8 pictures on the GPU (HapGpuMeasureTexture, HapGpuMeasureFrames).  The
definition is exact: with D what decompress_rgba or decode_frames_rgba returns for the same input and P the reference
picture, sse[c] = sum((D - P)^2) and sad[c] = sum(|D - P|) over every texel, per channel, in numpy's int64 -- every
comparison is by equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
# one lane; two lanes; 65 blocks a row (a block row ends inside a wave); 272 blocks (a second tile of 256 with 16 live
# lanes); 2313 blocks (ten tiles of 256, the last with 9 live lanes: three workgroups of four tiles, the last with two)
GEOMETRIES = ((4, 4), (8, 4), (260, 8), (68, 64), (1028, 36))
SENTINEL = 0xA7


@pytest.fixture(scope="module")
def hap():
    import hap_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hap_amd


@pytest.fixture(scope="module")
def ctx(hap):
    c = hap.Context(0)
    yield c
    c.close()


def sums(decoded, picture):
    """numpy's side of the definition: (sse, sad, texels) of two [h, w, 4] uint8 pictures"""
    d = decoded.astype(np.int64) - picture.astype(np.int64)
    return (tuple(int(v) for v in (d * d).sum(axis=(0, 1))), tuple(int(v) for v in np.abs(d).sum(axis=(0, 1))),
            decoded.shape[0] * decoded.shape[1])


def as_tuple(error):
    return error.sse, error.sad, error.texels


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_picture(picture, row_bytes=None):
    """An [h, w, 4] picture in device memory, rows row_bytes apart with sentinel bytes between them and behind the last"""
    h, w, _ = picture.shape
    row_bytes = row_bytes or w * 4
    raw = np.full((h, row_bytes), SENTINEL, dtype=np.uint8)
    raw[:, : w * 4] = picture.reshape(h, w * 4)
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


@functools.lru_cache(maxsize=None)
def random_texture(ctx, case, w, h):
    """Seeded random bytes: any 8 / 16 bytes are a block.  (texture, plane | None, what decompress_rgba makes of them);
    made once"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([CASES.index(case), w, h])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    r, out = ctx.decompress_rgba(tex, FORMATS[case], w, h, alpha=plane)
    assert r == 0
    decoded = np.frombuffer(out, dtype=np.uint8).reshape(h, w, 4).copy()
    decoded.setflags(write=False)
    return tex, plane, decoded


# ------------------------------------------------------------------------------- 1. every edge of the grid, textures --
@pytest.mark.parametrize("size", GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_textures_at_every_edge_of_the_grid(ctx, case, size):
    w, h = size
    tex, plane, decoded = random_texture(ctx, case, w, h)
    rng = np.random.default_rng([7, CASES.index(case), w, h])
    noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    # the decoded picture with one byte changed in the last texel of the last block, and another in texel 0
    touched = decoded.copy()
    touched[h - 1, w - 1, 2] ^= 0x10                        # B of the last texel: off by 16
    touched[0, 0, 1] = (int(touched[0, 0, 1]) + 3) % 256    # G of texel 0: off by 3, or by 253 where it wraps
    first = abs(int(touched[0, 0, 1]) - int(decoded[0, 0, 1]))
    assert sums(decoded, touched) == ((0, first * first, 256, 0), (0, first, 16, 0), w * h)
    dtex, dplane = dev(tex), dev(plane) if plane else None
    for name, picture in (("random", noise), ("itself", decoded), ("two bytes", touched)):
        want = sums(decoded, picture)
        if name == "itself":
            assert want == ((0,) * 4, (0,) * 4, w * h)
        reference = dev_picture(picture)
        for t, p in ((tex, plane), (dtex, dplane)):          # textures in host and in device memory
            r, error = ctx.measure_texture(t, FORMATS[case], w, h, reference, alpha=p)
            assert r == 0 and as_tuple(error) == want, (name, as_tuple(error), want)
        # the reference picture is read, never written
        assert np.array_equal(reference.cpu().numpy().reshape(h, w, 4), picture), name


@pytest.mark.parametrize("case", CASES)
def test_rows_longer_than_the_picture(ctx, case):
    w, h = 260, 8
    tex, plane, decoded = random_texture(ctx, case, w, h)
    noise = np.random.default_rng([8, CASES.index(case)]).integers(0, 256, (h, w, 4), dtype=np.uint8)
    row_bytes = w * 4 + 48
    for picture in (noise, decoded):
        reference = dev_picture(picture, row_bytes)
        r, error = ctx.measure_texture(tex, FORMATS[case], w, h, reference, alpha=plane, row_bytes=row_bytes)
        # (the sentinels between the rows do not count: against itself every sum is zero)
        assert r == 0 and as_tuple(error) == sums(decoded, picture)
        assert (reference.cpu().numpy()[:, w * 4:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------ 2. the width of the sums --
def test_sums_beyond_32_bits(ctx):
    w, h = 512, 516
    tex, plane, decoded = random_texture(ctx, "ycocg_alpha", w, h)
    picture = np.where(decoded >= 128, 0, 255).astype(np.uint8)
    want = sums(decoded, picture)
    assert all(v > 1 << 32 for v in want[0])                # every channel's sse needs more than 32 bits
    r, error = ctx.measure_texture(tex, L.FMT_YCOCG, w, h, dev_picture(picture), alpha=plane)
    assert r == 0 and as_tuple(error) == want


def test_more_workgroups_than_the_reduction_has_lanes(ctx):
    """bc_measure_reduce_kernel's 1024 lanes stride over a picture's workgroup partials.  4100 x 4096 texels are
    1 049 600 blocks and 1025 workgroups of 1024 blocks: lane 0 takes a second turn, for a full workgroup's partials."""
    w, h = 4100, 4096
    assert (w // 4) * (h // 4) == 1025 * 1024
    rng = np.random.default_rng([12, w, h])
    tex = rng.integers(0, 256, (w // 4) * (h // 4) * 8, dtype=np.uint8).tobytes()
    picture = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    r, out = ctx.decompress_rgba(tex, L.FMT_DXT1, w, h)                # (not random_texture: nothing this large is kept)
    assert r == 0
    decoded = np.frombuffer(out, dtype=np.uint8).reshape(h, w, 4)
    sse, sad = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for y in range(0, h, 256):                                         # by row bands: the differences of 64 MiB in int32
        d = decoded[y: y + 256].astype(np.int32) - picture[y: y + 256].astype(np.int32)
        sse += (d * d).sum(axis=(0, 1), dtype=np.int64)
        sad += np.abs(d).sum(axis=(0, 1), dtype=np.int64)
    want = (tuple(int(v) for v in sse), tuple(int(v) for v in sad), w * h)
    assert all(v > 1 << 32 for v in want[0][:3])
    r, error = ctx.measure_texture(tex, L.FMT_DXT1, w, h, dev_picture(picture))
    assert r == 0 and as_tuple(error) == want, (as_tuple(error), want)


# ------------------------------------------------------------------------------------------------------- 3. frames --
W, H = 64, 32
NB = (W // 4) * (H // 4)


def frames_of(ctx, hap, fmts, pictures, w, h, flags=0):
    """One Hap frame per RGBA picture (textures of `fmts`), made by encode_frames_rgba: list of bytes"""
    sizes = [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]
    chunks = [2] * len(fmts)
    bufs = [np.zeros(hap.HapMaxEncodedLength(sizes, fmts, chunks), dtype=np.uint8) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba([np.ascontiguousarray(p) for p in pictures], w, h, w * 4, fmts, [1] * len(fmts),
                                          chunks, bufs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return [b[:u].tobytes() for b, u in zip(bufs, used)]


def hap_encode(hap, textures, fmts):
    r, frame = hap.HapEncode(list(textures), list(fmts), [1] * len(fmts), [2] * len(fmts))
    assert r == 0
    return frame


def decoded_pictures(ctx, frames, count, flags=0):
    """What decode_frames_rgba writes for the frames: (results, [H, W, 4] pictures)"""
    pics = [np.zeros(H * W * 4, dtype=np.uint8) for _ in frames]
    _r, res = ctx.decode_frames_rgba(frames, [len(f) for f in frames], count, pics, W, H, flags=flags)
    return res, [p.reshape(H, W, 4) for p in pics]


def references(seed, n):
    """a different random reference picture for every frame"""
    rng = np.random.default_rng([9, seed])
    return [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(n)]


@pytest.fixture(scope="module")
def batches(ctx, hap):
    """name -> (frames, texture_count, decode_frames_rgba's pictures by frame); made once"""
    table = hap.ENCODE_FRAGMENT_INDEX
    out = {}
    mixed = [hap_encode(hap, [random_texture(ctx, "dxt1", W, H)[0]], [L.FMT_DXT1]),
             frames_of(ctx, hap, [L.FMT_DXT5], [D.rgba(W, H, 1)], W, H, flags=table)[0],
             hap_encode(hap, [random_texture(ctx, "ycocg", W, H)[0]], [L.FMT_YCOCG]),
             frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 3)], W, H, flags=table)[0],
             frames_of(ctx, hap, [L.FMT_DXT1], [D.rgba(W, H, 4)], W, H)[0],
             frames_of(ctx, hap, [L.FMT_YCOCG], [D.rgba(W, H, 5)], W, H)[0]]
    res, pictures = decoded_pictures(ctx, mixed, 1)
    assert res == [0] * len(mixed)
    out["mixed"] = (mixed, 1, pictures)
    tex, plane, _decoded = random_texture(ctx, "ycocg_alpha", W, H)
    qa = ([hap_encode(hap, [tex, plane], [L.FMT_YCOCG, L.FMT_RGTC1])]
          + frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 5), D.rgba(W, H, 6)], W, H, flags=table)
          + frames_of(ctx, hap, [L.FMT_YCOCG, L.FMT_RGTC1], [D.rgba(W, H, 7), D.rgba(W, H, 8)], W, H))
    res, pictures = decoded_pictures(ctx, qa, 2)
    assert res == [0] * len(qa)
    out["hap_q_alpha"] = (qa, 2, pictures)
    return out


@pytest.mark.parametrize("name", ("hap_q_alpha", "mixed"))
def test_every_frame_against_its_own_picture(ctx, batches, name):
    # hap_q_alpha: a reference-made frame, two with the fragment table, two plain, textureCount 2
    # mixed: Hap, Hap Alpha and Hap Q frames, reference-made, with the table and plain, in one call
    frames, count, decoded = batches[name]
    n = len(frames)
    assert n >= 5
    refs = references(CASES.index("dxt5") if name == "mixed" else 0, n)
    refs[1] = decoded[1].copy()                              # one frame against its own decoded picture
    pictures = [dev_picture(p) for p in refs]
    r, res, errors = ctx.measure_frames(frames, [len(f) for f in frames], count, pictures, W, H)
    assert r == 0 and res == [0] * n
    want = [sums(decoded[i], refs[i]) for i in range(n)]
    assert [as_tuple(e) for e in errors] == want
    assert want[1] == ((0,) * 4, (0,) * 4, W * H)
    # (a mix-up would show: no two frames have the same sums)
    assert len(set(want)) == n


def test_one_launch_per_format_present_in_the_existing_class(ctx, batches):
    frames, count, _decoded = batches["mixed"]
    pictures = [dev_picture(p) for p in references(3, len(frames))]
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.measure_frames(frames, [len(f) for f in frames], count, pictures, W, H)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 3, prof["block_decode"]


def test_frames_with_longer_rows_from_addresses(ctx, batches):
    frames, count, decoded = batches["hap_q_alpha"]
    refs = references(4, len(frames))
    row_bytes = W * 4 + 16
    pictures = [dev_picture(p, row_bytes) for p in refs]
    r, res, errors = ctx.measure_frames(frames, [len(f) for f in frames], count, [p.data_ptr() for p in pictures], W, H,
                                        row_bytes=row_bytes)
    assert r == 0 and res == [0] * len(frames)
    assert [as_tuple(e) for e in errors] == [sums(d, p) for d, p in zip(decoded, refs)]


# ------------------------------------------------------------------------------------------- 4. per-frame failures --
@pytest.mark.parametrize("bptc_flag", (False, True))
def test_a_bad_frame_fails_alone(ctx, hap, batches, bptc_flag):
    good, _count, decoded = batches["mixed"]
    bad, broken = hap.HapResult.Bad_Arguments, hap.HapResult.Bad_Frame
    hap_r = frames_of(ctx, hap, [L.FMT_BC7], [D.rgba(W, H, 8)], W, H, flags=hap.ENCODE_BPTC_BLOCKS)[0]
    #         good     Hap R  good     truncated      good     no picture  good
    frames = [good[0], hap_r, good[1], good[2][:-3], good[3], good[4], good[2]]
    source = [0, None, 1, None, 3, None, 2]
    expect = [0, bad, 0, broken, 0, bad, 0]
    refs = references(5, len(frames))
    pictures = [None if i == 5 else dev_picture(p) for i, p in enumerate(refs)]
    r, res, errors = ctx.measure_frames(frames, [len(f) for f in frames], 1, pictures, W, H,
                                        flags=hap.DECODE_BPTC_PICTURES if bptc_flag else 0)
    assert res == expect and r == bad
    for i, e in enumerate(errors):
        if source[i] is None:
            assert as_tuple(e) == ((0,) * 4, (0,) * 4, 0), i
        else:
            assert as_tuple(e) == sums(decoded[source[i]], refs[i]), i


def test_a_host_or_misaligned_picture_fails_alone(ctx, hap, batches):
    frames, count, decoded = batches["mixed"]
    frames, decoded = frames[:3], decoded[:3]
    bad = hap.HapResult.Bad_Arguments
    refs = references(6, 3)
    off = torch.zeros(H * W * 4 + 16, dtype=torch.uint8, device="cuda")
    pictures = [np.ascontiguousarray(refs[0]), off.data_ptr() + 4, dev_picture(refs[2])]
    r, res, errors = ctx.measure_frames(frames, [len(f) for f in frames], count, pictures, W, H)
    assert r == bad and res == [bad, bad, 0]
    assert [as_tuple(e) for e in errors] == [((0,) * 4, (0,) * 4, 0)] * 2 + [sums(decoded[2], refs[2])]


# ------------------------------------------------------------------------------------------------- 5. arguments --
def test_arguments(ctx, hap, batches):
    w, h = 68, 64
    bad = hap.HapResult.Bad_Arguments
    tex, _plane, decoded = random_texture(ctx, "dxt5", w, h)
    picture = np.random.default_rng(10).integers(0, 256, (h, w, 4), dtype=np.uint8)
    reference = dev_picture(picture, w * 4 + 16)
    assert as_tuple(ctx.measure_texture(tex, L.FMT_DXT5, w, h, dev_picture(picture))[1]) == sums(decoded, picture)
    # a host picture; an address off by 4; rows too short, or no multiple of 16
    assert ctx.measure_texture(tex, L.FMT_DXT5, w, h, np.ascontiguousarray(picture)) == (bad, None)
    assert ctx.measure_texture(tex, L.FMT_DXT5, w, h, reference.data_ptr() + 4) == (bad, None)
    assert ctx.measure_texture(tex, L.FMT_DXT5, w, h, reference, row_bytes=w * 4 - 16) == (bad, None)
    assert ctx.measure_texture(tex, L.FMT_DXT5, w, h, reference, row_bytes=w * 4 + 8) == (bad, None)
    assert ctx.measure_texture(tex, L.FMT_DXT5, w, h, None) == (bad, None)
    # BC7, BC6H or a lone RGTC1
    for fmt in (L.FMT_BC7, 0x8E8F, 0x8E8E, L.FMT_RGTC1):
        assert ctx.measure_texture(tex, fmt, w, h, reference, row_bytes=w * 4 + 16) == (bad, None), fmt
    # ... and nothing is written: the struct of a refused call stays as it was
    lib = hap._lib.lib
    error = hap._lib.HapGpuPictureError()
    C.memset(C.byref(error), 0x5A, C.sizeof(error))
    keep = np.frombuffer(tex, dtype=np.uint8)
    for fmt, address, row in ((L.FMT_BC7, reference.data_ptr(), w * 4 + 16), (L.FMT_DXT5, reference.data_ptr() + 4, w * 4 + 16),
                              (L.FMT_DXT5, picture.ctypes.data, w * 4), (L.FMT_DXT5, reference.data_ptr(), w * 4 + 8)):
        assert lib.HapGpuMeasureTexture(ctx.handle, keep.ctypes.data, len(tex), fmt, None, 0, w, h, address, row,
                                        C.byref(error)) == bad
        assert bytes(error) == b"\x5A" * 72
    assert lib.HapGpuMeasureTexture(ctx.handle, keep.ctypes.data, len(tex), L.FMT_DXT5, None, 0, w, h, reference.data_ptr(),
                                    w * 4 + 16, None) == bad
    # frames: the whole call is refused, every result set, no struct written
    frames, count, _decoded = batches["mixed"]
    n = len(frames)
    pictures = [dev_picture(p) for p in references(7, n)]
    keep_frames = [np.frombuffer(f, dtype=np.uint8) for f in frames]
    ptrs = (C.c_void_p * n)(*[k.ctypes.data for k in keep_frames])
    lens = (C.c_ulong * n)(*[len(f) for f in frames])
    pics = (C.c_void_p * n)(*[p.data_ptr() for p in pictures])
    errors = (hap._lib.HapGpuPictureError * n)()
    for name, row, errs, pictures_array in (("short rows", W * 4 - 16, errors, pics), ("rows off 16", W * 4 + 8, errors, pics),
                                            ("no errors", W * 4, None, pics), ("no pictures", W * 4, errors, None)):
        C.memset(errors, 0x5A, C.sizeof(errors))
        res = (C.c_uint * n)(*([77] * n))
        assert lib.HapGpuMeasureFrames(ctx.handle, n, ptrs, lens, count, pictures_array, W, H, row, errs, res, 0) == bad, name
        assert list(res) == [bad] * n and bytes(errors) == b"\x5A" * C.sizeof(errors), name


# ------------------------------------------------------------------------------------------------ 6. determinism --
def test_the_same_call_twice_gives_the_same_structs(ctx, batches):
    frames, count, _decoded = batches["hap_q_alpha"]
    pictures = [dev_picture(p) for p in references(8, len(frames))]
    first = ctx.measure_frames(frames, [len(f) for f in frames], count, pictures, W, H)
    second = ctx.measure_frames(frames, [len(f) for f in frames], count, pictures, W, H)
    assert first[0] == 0 and first == second
    w, h = 1028, 36
    tex, plane, _d = random_texture(ctx, "ycocg_alpha", w, h)
    reference = dev_picture(np.random.default_rng(11).integers(0, 256, (h, w, 4), dtype=np.uint8))
    assert (ctx.measure_texture(tex, L.FMT_YCOCG, w, h, reference, alpha=plane)
            == ctx.measure_texture(tex, L.FMT_YCOCG, w, h, reference, alpha=plane))


# -------------------------------------------------------------------------------------------- 7. transcode sanity --
def test_a_frame_that_passes_through_a_transcode_measures_zero(ctx, hap, batches):
    frames, count, decoded = batches["mixed"]
    source, picture = frames[3], decoded[3]                  # a Hap Q frame
    out = np.zeros(hap.HapMaxEncodedLength([NB * 16], [L.FMT_YCOCG], [2]), dtype=np.uint8)
    r, used, res = ctx.transcode_frames([source], [len(source)], 1, W, H, 0, [L.FMT_YCOCG], [1], [2], [out])
    assert r == 0 and res == [0]
    again = out[: used[0]].tobytes()
    r, res, errors = ctx.measure_frames([again], [len(again)], 1, [dev_picture(picture)], W, H)
    assert r == 0 and res == [0] and as_tuple(errors[0]) == ((0,) * 4, (0,) * 4, W * H)

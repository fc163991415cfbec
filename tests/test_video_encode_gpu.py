"""NV12 video pictures straight to block textures and Hap frames (HapGpuCompressNV12, HapGpuEncodeFramesNV12[Begin]).
The definition is exact -- tests/_video_pictures.py: integers, one rounding, a clamp, each CbCr pair replicated over its
2 x 2 luma samples -- and the textures and frames are those of the RGBA8 picture of these bytes: every comparison here is
byte for byte against compress_rgba / encode_frames_rgba of rgba_of_nv12(...) with the same formats, compressors, chunk
counts and flags.  The planes' pitches differ from each other and are larger than the width, and what lies between the
rows would change the blocks if it were read."""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import _video_pictures as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
ORACLE = L.oracle_api()
REFERENCE = L.ref_api()                                     # the unmodified reference, where it has been built
FORMATS = {"hap": L.FMT_DXT1, "hap_q": L.FMT_YCOCG}
BLOCK_BYTES = {L.FMT_DXT1: 8, L.FMT_YCOCG: 16}
# one lane; two; a wave one short of full, exactly full, and one lane over -- one, two and three block rows
WIDTHS, HEIGHTS = (4, 8, 252, 256, 260), (4, 8, 12)
SLICE = 32768                                               # hap_slice.h: HAP_SLICE_ENTRIES


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


def host(t):
    return t.cpu().numpy()


def filled(n, where="cuda"):
    t = torch.full((n,), SENTINEL, dtype=torch.uint8, device=where)
    if where == "cuda":
        torch.cuda.synchronize()
    return t


def on_device(y, uv, luma_extra=12, chroma_extra=20):
    """The two planes in device memory, rows w + 12 and w + 20 bytes apart, the padding poisoned: (Y view, CbCr view)"""
    w = y.shape[1]
    ywhole, _view = V.padded(y, w + luma_extra)
    cwhole, _view = V.padded(uv, w + chroma_extra)
    yd, cd = torch.from_numpy(ywhole).cuda(), torch.from_numpy(cwhole).cuda()
    torch.cuda.synchronize()
    return yd[:, :w], cd[:, :w]


def texture_size(w, h, fmt):
    return (w // 4) * (h // 4) * BLOCK_BYTES[fmt]


def rgba_texture(ctx, picture, fmt, flags=0):
    h, w = picture.shape[:2]
    r, tex = ctx.compress_rgba(np.ascontiguousarray(picture), w, h, w * 4, fmt, flags=flags)
    assert r == 0
    return tex


def rgba_frames(ctx, pictures, fmt, comp, chunks, cap, flags):
    """HapGpuEncodeFramesRGBA of the pictures (uploaded): (used, [frames])"""
    h, w = pictures[0].shape[:2]
    pics = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pictures]
    outs = [filled(cap) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba(pics, w, h, w * 4, [fmt], [comp], [chunks], outs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return used, [host(o)[:u].tobytes() for o, u in zip(outs, used)]


# -------------------------------------------------------------------------------------------------------- 1. textures --
@pytest.mark.parametrize("row", V.ROWS, ids=lambda r: V.NAMES[r].replace(" ", "_"))
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_textures_are_the_rgba_calls_of_the_converted_picture(ctx, name, row):
    fmt = FORMATS[name]
    calls = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for content, (y, uv) in (("random", V.random_nv12(w, h, 1)), ("extremes", V.extremes_nv12(w, h))):
                want = rgba_texture(ctx, V.rgba_of_nv12(y, uv, *row), fmt)
                yd, cd = on_device(y, uv)
                assert yd.stride(0) != cd.stride(0) and yd.stride(0) > w and cd.stride(0) > w
                where = ("cuda", "cpu")[calls % 2]
                out = filled(len(want) + 64, where)
                r, used = ctx.compress_nv12(yd, cd, w, h, fmt, matrix=row[0], range=row[1], output=out[: len(want)])
                note = (w, h, content, where)
                assert (r, used) == (0, len(want)), note
                got = host(out)
                assert got[: len(want)].tobytes() == want, note
                assert (got[len(want):] == SENTINEL).all(), note
                calls += 1
    print(f"{name} {V.NAMES[row]}: {calls} textures equal to the RGBA call's")


def test_the_defaults_a_short_output_and_planes_that_cannot_be_read(ctx, hap):
    w, h = 8, 8
    y, uv = V.random_nv12(w, h, 2)
    yd, cd = on_device(y, uv)
    bad = hap.HapResult.Bad_Arguments
    r, tex = ctx.compress_nv12(yd, cd, w, h, L.FMT_YCOCG)                                 # BT.709, limited
    assert r == 0 and tex == rgba_texture(ctx, V.rgba_of_nv12(y, uv, V.BT709, V.LIMITED), L.FMT_YCOCG)
    # the pairs as a last dimension of two: the same plane
    r, tex2 = ctx.compress_nv12(yd, cd.unflatten(1, (w // 2, 2)), w, h, L.FMT_YCOCG)
    assert r == 0 and tex2 == tex
    out = filled(128)
    assert ctx.compress_nv12(yd, cd, w, h, L.FMT_YCOCG, output=out[:63])[0] == hap.HapResult.Buffer_Too_Small
    assert ctx.compress_nv12(yd, cd, w, h, L.FMT_DXT5, output=out[:64])[0] == bad
    assert ctx.compress_nv12(yd, cd, w, h, L.FMT_YCOCG, matrix=2, output=out[:64])[0] == bad
    # a plane in host memory, and one two bytes off
    pitches = dict(luma_row_bytes=yd.stride(0), chroma_row_bytes=cd.stride(0))
    on_host = torch.zeros(4096, dtype=torch.uint8)
    for luma, chroma in ((on_host.data_ptr(), cd.data_ptr()), (yd.data_ptr(), on_host.data_ptr()),
                         (yd.data_ptr() + 2, cd.data_ptr()), (yd.data_ptr(), cd.data_ptr() + 2)):
        assert ctx.compress_nv12(luma, chroma, w, h, L.FMT_YCOCG, output=out[:64], **pitches)[0] == bad
    assert (host(out) == SENTINEL).all()
    r, used = ctx.compress_nv12(yd.data_ptr(), cd.data_ptr(), w, h, L.FMT_YCOCG, output=out[:64], **pitches)
    assert (r, used) == (0, 64) and host(out)[:64].tobytes() == tex


# ---------------------------------------------------------------------------------------------- 2. chroma replication --
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_every_texel_takes_its_own_pair(ctx, name):
    """A flat luma under a chroma that differs in every pair and every chroma row, over two waves and three block rows"""
    fmt = FORMATS[name]
    w, h = 260, 12
    y, uv = V.distinct_chroma_nv12(w, h)
    assert len({(int(a), int(b)) for a, b in zip(uv[:, 0::2].ravel(), uv[:, 1::2].ravel())}) > 250
    yd, cd = on_device(y, uv)
    for row in V.ROWS:
        r, tex = ctx.compress_nv12(yd, cd, w, h, fmt, matrix=row[0], range=row[1])
        assert r == 0 and tex == rgba_texture(ctx, V.rgba_of_nv12(y, uv, *row), fmt), row


def test_a_block_checked_by_hand(ctx):
    """4 x 4, BT.601 full range, Y = 100 everywhere, one pair per quadrant.  By hand, with Y' = 65536 * 100 = 6553600:
    (128, 128): grey, (100, 100, 100)
    (128, 255): v = 127: R = (6553600 + 91881 * 127 + 32768) >> 16 = 278 -> 255, G = (6553600 - 46802 * 127 + 32768) >> 16 = 9
    (255, 128): u = 127: G = (6553600 - 22553 * 127 + 32768) >> 16 = 56, B = (6553600 + 116130 * 127 + 32768) >> 16 = 325 -> 255
    (0, 0): u = v = -128: R, B below zero -> 0, G = (6553600 + (22553 + 46802) * 128 + 32768) >> 16 = 235"""
    y = np.full((4, 4), 100, dtype=np.uint8)
    uv = np.array([[128, 128, 128, 255], [255, 128, 0, 0]], dtype=np.uint8)
    hand = np.empty((4, 4, 4), dtype=np.uint8)
    hand[:2, :2], hand[:2, 2:] = (100, 100, 100, 255), (255, 9, 100, 255)
    hand[2:, :2], hand[2:, 2:] = (100, 56, 255, 255), (0, 235, 0, 255)
    assert np.array_equal(V.rgba_of_nv12(y, uv, V.BT601, V.FULL), hand)
    yd, cd = on_device(y, uv)
    for fmt in FORMATS.values():
        r, tex = ctx.compress_nv12(yd, cd, 4, 4, fmt, matrix=V.BT601, range=V.FULL)
        assert r == 0 and tex == rgba_texture(ctx, hand, fmt)
    # the four colours are four end points apart: a DXT1 block that mixed the pairs up would be another block
    swapped = hand[:, ::-1].copy()
    assert rgba_texture(ctx, swapped, L.FMT_DXT1) != rgba_texture(ctx, hand, L.FMT_DXT1)


# ---------------------------------------------------------------------------------------------------------- 3. frames --
def frame_pictures(w, h):
    """three NV12 pictures: random, smooth (frames that compress), the extremes"""
    return [V.random_nv12(w, h, 3), V.smooth_nv12(w, h, 1), V.extremes_nv12(w, h, 1)]


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_frames_equal_the_rgba_calls(ctx, hap, name):
    fmt = FORMATS[name]
    w, h = 64, 32
    size = texture_size(w, h, fmt)
    cap = hap.HapMaxEncodedLength([size], [fmt], [max(3, hap.fine_chunk_count(size, fmt))]) + 4096
    sources = frame_pictures(w, h)
    n = len(sources)
    planes = [on_device(y, uv) for y, uv in sources]
    lumas, chromas = [p[0] for p in planes], [p[1] for p in planes]
    combo = 0
    for flags in (0, hap.ENCODE_FRAGMENT_INDEX, hap.ENCODE_FINE_CHUNKS):
        for comp in (L.COMP_SNAPPY, L.COMP_NONE):
            for chunks in (1, 3):
                row = V.ROWS[combo % 4]
                pictures = [V.rgba_of_nv12(y, uv, *row) for y, uv in sources]
                want_used, want = rgba_frames(ctx, pictures, fmt, comp, chunks, cap, flags)
                outs = [filled(cap + 64) for _ in range(n)]
                r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [comp], [chunks], [o[:cap] for o in outs],
                                                      matrix=row[0], range=row[1], flags=flags)
                note = (flags, comp, chunks, row)
                assert r == 0 and res == [0] * n and used == want_used, (note, r, res, used, want_used)
                got = [host(o) for o in outs]
                assert all((g[cap:] == SENTINEL).all() for g in got), note
                got = [g[:u].tobytes() for g, u in zip(got, used)]
                assert got == want, note
                if comp == L.COMP_SNAPPY:
                    assert used[1] < size, note                 # (the smooth picture shrank: the second stage had work)
                # the frames decode: through the existing picture road ...
                back = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
                frames = [o[:u] for o, u in zip(outs, used)]
                r, res = ctx.decode_frames_rgba(frames, list(used), 1, back, w, h)
                assert r == 0 and res == [0] * n, note
                # ... and frame 0 through the checker and, where it is there, the unmodified reference, to the texture
                texture = rgba_texture(ctx, pictures[0], fmt)
                for api in (ORACLE, REFERENCE):
                    if api is not None:
                        rr, tex, ff = api.decode(got[0], 0, out_bytes=size)
                        assert (rr, ff) == (0, fmt) and tex == texture, note
                combo += 1


def test_one_frame_more_than_a_slice(ctx, hap):
    """32769 frames of 8 x 4: the second slice's CbCr planes are cut from the call's like its pictures (32768 is 3 modulo
    5: a plane looked up by a slice-relative index is another picture's)"""
    w, h, fmt = 8, 4, L.FMT_YCOCG
    row = (V.BT601, V.LIMITED)
    five = [V.random_nv12(w, h, 10 + i) for i in range(5)]
    planes = [on_device(y, uv) for y, uv in five]
    cap = hap.HapMaxEncodedLength([texture_size(w, h, fmt)], [fmt], [1])
    want_used, want = rgba_frames(ctx, [V.rgba_of_nv12(y, uv, *row) for y, uv in five], fmt, L.COMP_SNAPPY, 1, cap, 0)
    assert len(set(want)) == 5
    n = SLICE + 1
    which = np.arange(n) % 5
    out = torch.full((n, cap), SENTINEL, dtype=torch.uint8)
    r, used, res = ctx.encode_frames_nv12([planes[k][0] for k in which], [planes[k][1] for k in which], w, h, [fmt],
                                          [L.COMP_SNAPPY], [1], list(out), matrix=row[0], range=row[1])
    assert r == 0 and res == [0] * n
    assert used == [want_used[k] for k in which]
    small = np.full((5, cap), SENTINEL, dtype=np.uint8)
    for k in range(5):
        small[k, : want_used[k]] = np.frombuffer(want[k], dtype=np.uint8)
    wrong = np.argwhere((out.numpy() != small[which]).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()
    # ... and a Begin of as many is refused before anything is looked at
    results = (C.c_uint * n)(*[0xA7A7A7A7] * n)
    ptrs = (C.c_void_p * n)(*[planes[0][0].data_ptr()] * n)
    one = (C.c_uint * 1)
    r = hap._lib.lib.HapGpuEncodeFramesNV12Begin(ctx.handle, n, ptrs, w + 12, ptrs, w + 20, 0, 0, w, h, 1, one(fmt), one(1), one(1),
                                                 ptrs, (C.c_ulong * n)(), (C.c_ulong * n)(), results, 0)
    assert r == hap.HapResult.Bad_Arguments and (np.frombuffer(results, np.uint32) == 0xA7A7A7A7).all()


def test_a_batch_large_enough_to_be_placed(hap):
    """Nine frames of noise with the fragment table and room in their buffers: the second stage writes fragments where
    they belong in the frame, chunks that do not shrink make their frames be encoded a second time -- from the planes
    again, Y and CbCr.  (A context of its own, the video call first: a call that encodes most frames twice makes the next
    ones gather.)"""
    w, h, n, fmt = 256, 64, 9, L.FMT_YCOCG
    row = (V.BT709, V.FULL)
    size = texture_size(w, h, fmt)
    cap = 2 * hap.HapMaxEncodedLength([size], [fmt], [2]) + 65536
    sources = [V.random_nv12(w, h, 20 + f) for f in range(n)]
    planes = [on_device(y, uv) for y, uv in sources]
    ctx = hap.Context(0)
    outs = [filled(cap) for _ in range(n)]
    r, used, res = ctx.encode_frames_nv12([p[0] for p in planes], [p[1] for p in planes], w, h, [fmt], [L.COMP_SNAPPY], [2],
                                          outs, matrix=row[0], range=row[1], flags=hap.ENCODE_FRAGMENT_INDEX)
    again = ctx.placement_retries()
    print(f"{again} of {n} frames encoded a second time")
    assert r == 0 and res == [0] * n
    assert again > 0
    want_used, want = rgba_frames(ctx, [V.rgba_of_nv12(y, uv, *row) for y, uv in sources], fmt, L.COMP_SNAPPY, 2, cap,
                                  hap.ENCODE_FRAGMENT_INDEX)
    ctx.close()
    assert used == want_used
    assert [host(o)[:u].tobytes() for o, u in zip(outs, used)] == want


# ----------------------------------------------------------------------------------------------------------- 4. flags --
def test_refined_end_points_and_the_bptc_flag(ctx, hap):
    w, h, fmt = 64, 32, L.FMT_DXT1
    row = (V.BT709, V.LIMITED)
    sources = frame_pictures(w, h)
    planes = [on_device(y, uv) for y, uv in sources]
    lumas, chromas = [p[0] for p in planes], [p[1] for p in planes]
    pictures = [V.rgba_of_nv12(y, uv, *row) for y, uv in sources]
    cap = hap.HapMaxEncodedLength([texture_size(w, h, fmt)], [fmt], [2]) + 4096
    made = {}
    for flags in (0, hap.ENCODE_REFINE_ENDPOINTS, hap.ENCODE_BPTC_BLOCKS, hap.ENCODE_REFINE_ENDPOINTS | hap.ENCODE_BPTC_BLOCKS):
        outs = [filled(cap) for _ in sources]
        r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs, flags=flags)
        assert r == 0 and res == [0] * len(sources), flags
        made[flags] = [host(o)[:u].tobytes() for o, u in zip(outs, used)]
    _used, plain = rgba_frames(ctx, pictures, fmt, L.COMP_SNAPPY, 2, cap, 0)
    _used, refined = rgba_frames(ctx, pictures, fmt, L.COMP_SNAPPY, 2, cap, hap.ENCODE_REFINE_ENDPOINTS)
    assert made[0] == plain and made[hap.ENCODE_REFINE_ENDPOINTS] == refined
    assert refined[0] != plain[0]                                                    # (the flag has something to say here)
    assert made[hap.ENCODE_BPTC_BLOCKS] == plain and made[hap.ENCODE_REFINE_ENDPOINTS | hap.ENCODE_BPTC_BLOCKS] == refined
    # Hap Q has no refined form: the flag changes nothing there
    outs = [filled(cap * 2) for _ in sources]
    r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [L.FMT_YCOCG], [L.COMP_SNAPPY], [2], outs,
                                          flags=hap.ENCODE_REFINE_ENDPOINTS)
    assert r == 0 and res == [0] * len(sources)
    _used, hap_q = rgba_frames(ctx, pictures, L.FMT_YCOCG, L.COMP_SNAPPY, 2, cap * 2, 0)
    assert [host(o)[:u].tobytes() for o, u in zip(outs, used)] == hap_q


# ----------------------------------------------------------------------------------------------- 5. per-frame refusal --
def test_a_frame_whose_planes_cannot_be_read_fails_alone(ctx, hap):
    bad = hap.HapResult.Bad_Arguments
    w, h, fmt = 64, 32, L.FMT_YCOCG
    row = (V.BT601, V.FULL)
    sources = [V.smooth_nv12(w, h, f) for f in range(7)]
    planes = [on_device(y, uv) for y, uv in sources]
    pitches = dict(luma_row_bytes=w + 12, chroma_row_bytes=w + 20)
    cap = hap.HapMaxEncodedLength([texture_size(w, h, fmt)], [fmt], [2]) + 4096
    call = dict(matrix=row[0], range=row[1], **pitches)
    lumas, chromas = [p[0].data_ptr() for p in planes], [p[1].data_ptr() for p in planes]
    outs = [filled(cap) for _ in sources]
    r, want_used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs, **call)
    assert r == 0 and res == [0] * 7
    want = [host(o)[:u].tobytes() for o, u in zip(outs, want_used)]
    _used, rgba = rgba_frames(ctx, [V.rgba_of_nv12(y, uv, *row) for y, uv in sources], fmt, L.COMP_SNAPPY, 2, cap, 0)
    assert want == rgba
    # good / NULL luma / good / host chroma / good / chroma at address + 2 / good
    on_host = torch.zeros((h // 2) * (w + 20), dtype=torch.uint8)
    lumas[1] = None
    chromas[3] = on_host.data_ptr()
    chromas[5] += 2
    outs = [filled(cap) for _ in sources]
    r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs, **call)
    assert r == bad                                            # the first failure
    assert res == [0, bad, 0, bad, 0, bad, 0]
    for f, o in enumerate(outs):
        if f % 2 == 0:
            assert used[f] == want_used[f] and host(o)[: used[f]].tobytes() == want[f], f
        else:
            assert (host(o) == SENTINEL).all(), f
    # ... and the other plane of a pair: NULL chroma, host luma, luma at address + 2
    lumas, chromas = [p[0].data_ptr() for p in planes[:4]], [p[1].data_ptr() for p in planes[:4]]
    chromas[0] = None
    lumas[1] = on_host.data_ptr()
    lumas[2] += 2
    outs = [filled(cap) for _ in range(4)]
    r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs, **call)
    assert r == bad and res == [bad, bad, bad, 0]
    assert all((host(o) == SENTINEL).all() for o in outs[:3]) and host(outs[3])[: used[3]].tobytes() == want[3]


# -------------------------------------------------------------------------------------------------- 6. the two halves --
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_begin_and_finish_give_the_blocking_calls_bytes(ctx, hap, name):
    fmt = FORMATS[name]
    w, h = 64, 32
    row = (V.BT709, V.FULL)
    sources = frame_pictures(w, h)
    n = len(sources)
    planes = [on_device(y, uv) for y, uv in sources]
    lumas, chromas = [p[0] for p in planes], [p[1] for p in planes]
    cap = hap.HapMaxEncodedLength([texture_size(w, h, fmt)], [fmt], [2]) + 4096
    call = dict(matrix=row[0], range=row[1], flags=hap.ENCODE_FRAGMENT_INDEX)
    outs = [filled(cap) for _ in range(n)]
    r, want_used, res = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs, **call)
    assert r == 0 and res == [0] * n
    want = [host(o)[:u].tobytes() for o, u in zip(outs, want_used)]
    outs2 = [filled(cap) for _ in range(n)]
    assert ctx.encode_frames_nv12_begin(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], outs2, **call) == 0
    # the caller's arrays need not outlive the first half: planes, outputs and their sizes are overwritten
    _used, _results, yptrs, cptrs, optrs, olens = ctx._pending[:6]
    for array in (yptrs, cptrs, optrs):
        assert isinstance(array, C.Array) and len(array) == n
        for f in range(n):
            array[f] = 0x5A5A5A5A5A58
    for f in range(n):
        olens[f] = 1
    # between the halves the context takes no other call
    internal = hap.HapResult.Internal_Error
    r3, _used3, res3 = ctx.encode_frames_nv12(lumas, chromas, w, h, [fmt], [L.COMP_SNAPPY], [2], [filled(cap) for _ in range(n)], **call)
    assert r3 == internal and res3 == [internal] * n
    assert ctx.compress_nv12(lumas[0], chromas[0], w, h, fmt)[0] == internal
    r2, used2, res2 = ctx.encode_finish()
    assert r2 == 0 and res2 == [0] * n and used2 == want_used
    assert [host(o)[:u].tobytes() for o, u in zip(outs2, used2)] == want


# ------------------------------------------------------------------------------------------- 7. the pictures can tell --
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_a_wrong_converter_would_show(ctx, hap, name):
    """No new code runs here.  For the random 64 x 32 picture the RGBA road's frames from three deliberately wrong
    converters -- the + 32768 dropped, BT.601 used for BT.709, limited used for full -- differ from the right ones: a
    lossy block encoder cannot hide such an error at these shapes."""
    fmt = FORMATS[name]
    w, h = 64, 32
    y, uv = V.random_nv12(w, h, 3)
    cap = hap.HapMaxEncodedLength([texture_size(w, h, fmt)], [fmt], [1]) + 4096
    for row in V.ROWS:
        right = V.rgba_of_nv12(y, uv, *row)
        mutants = {"the rounding dropped": V.rgba_of_nv12(y, uv, *row, rounding=0)}
        if row[0] == V.BT709:
            mutants["BT.601 for BT.709"] = V.rgba_of_nv12(y, uv, *row, coefficients_of=lambda m, r: V.coefficients(V.BT601, r))
        if row[1] == V.FULL:
            mutants["limited for full"] = V.rgba_of_nv12(y, uv, *row, coefficients_of=lambda m, r: V.coefficients(m, V.LIMITED))
        _used, frames = rgba_frames(ctx, [right] + list(mutants.values()), fmt, L.COMP_NONE, 1, cap, 0)
        for mutant, frame in zip(mutants, frames[1:]):
            assert frame != frames[0], (row, mutant)

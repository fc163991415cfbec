"""Frames to frames and textures to textures of another flavour or size without a picture in between
(HapGpuTranscodeTexture, HapGpuTranscodeFrames).  The definition: the output is byte for byte what the encoder makes of
the picture the decoder (at half / quarter size: the scaled decoder) writes for the source.  Every expected texture is
made on the CPU alone -- tests/_data.oracle_bc_decode with the RGTC1 plane into A, the numpy box mean of
tests/test_scaled_decode_gpu.py, tests/_data.oracle_bc_encode per destination format -- and every expected frame is the
frame of the two-call route; every comparison is byte for byte."""
import ctypes as C
import functools

import numpy as np
import pytest

import _data as D
import _libs as L
import _value_space as VS
from test_scaled_decode_gpu import box

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
SCALES = (0, 1, 2)
SOURCES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
SETS = {"dxt1": [L.FMT_DXT1], "dxt5": [L.FMT_DXT5], "ycocg": [L.FMT_YCOCG], "ycocg_alpha": [L.FMT_YCOCG, L.FMT_RGTC1]}
# destination geometries: one lane; the smallest two-lane grids; exactly one wave per block row; a one-lane second wave
# in each row
GEOMETRIES = ((4, 4), (8, 4), (4, 8), (256, 8), (260, 12))
REF = L.ref_api() or L.oracle_api()


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


def dev(data):
    t = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def filled(nbytes, where):
    t = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=where)
    torch.cuda.synchronize()
    return t


def host(buf):
    return buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)


def texture_bytes(w, h, fmts):
    return [(w // 4) * (h // 4) * D.BLOCK_BYTES[f] for f in fmts]


def expected_textures(case, tex, plane, w, h, s, dst):
    """The CPU definition: decode (the plane into A), box mean, encode per destination format."""
    pic = D.oracle_bc_decode(tex, FORMATS[case], w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(plane, L.FMT_RGTC1, w, h)
    if s:
        pic = box(pic, s)
    pic = np.ascontiguousarray(pic)
    return [D.oracle_bc_encode(pic, f) for f in SETS[dst]]


def transcoded(ctx, case, tex, plane, w, h, s, dst, where):
    """transcode_texture into sentinel-filled outputs 64 bytes too long: (result, textures, tails, used)"""
    sizes = texture_bytes(w >> s, h >> s, SETS[dst])
    outs = [filled(n + 64, where) for n in sizes]
    r, used = ctx.transcode_texture(tex, FORMATS[case], w, h, s, SETS[dst], alpha=plane, outputs=outs)
    got = [host(o) for o in outs]
    return r, [g[:n].tobytes() for g, n in zip(got, sizes)], [g[n:] for g, n in zip(got, sizes)], used


# ----------------------------------------------------------------------------------------- 1. the kernel, every pair --
@functools.lru_cache(maxsize=None)
def random_texture(case, w, h):
    """Seeded random bytes: any 8 / 16 bytes are a block.  (texture, plane | None)"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([SOURCES.index(case), w, h])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    return tex, plane


def test_the_random_blocks_reach_both_palette_modes():
    tex = np.frombuffer(random_texture("dxt1", 260 << 2, 12 << 2)[0], np.uint8).view("<u2").reshape(-1, 4)
    assert (tex[:, 0] <= tex[:, 1]).any() and (tex[:, 0] > tex[:, 1]).any()          # three- and four-colour DXT1
    for case, part in (("dxt5", 0), ("ycocg", 0), ("ycocg_alpha", 1)):
        blocks = np.frombuffer(random_texture(case, 260, 12)[part], np.uint8).reshape(-1, 16 if part == 0 else 8)
        assert (blocks[:, 0] <= blocks[:, 1]).any() and (blocks[:, 0] > blocks[:, 1]).any(), case   # both ramp orders


@pytest.mark.parametrize("size", GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", SOURCES)
def test_every_pair_at_every_scale(ctx, case, size):
    for s in SCALES:
        w, h = size[0] << s, size[1] << s                   # the source's geometry
        tex, plane = random_texture(case, w, h)
        dtex, dplane = dev(tex), dev(plane) if plane else None
        for dst in SETS:
            if s == 0 and dst == case:
                want = [tex] + ([plane] if plane else [])    # the set the source is already: copied
            else:
                want = expected_textures(case, tex, plane, w, h, s, dst)
            for where in ("cuda", "cpu"):
                for t, p in ((tex, plane), (dtex, dplane)):
                    r, got, tails, used = transcoded(ctx, case, t, p, w, h, s, dst, where)
                    assert r == 0, (s, dst, where)
                    assert used == [len(x) for x in want], (s, dst, where)
                    for i, (g, x) in enumerate(zip(got, want)):
                        diff = np.flatnonzero(np.frombuffer(g, np.uint8) != np.frombuffer(x, np.uint8))
                        assert g == x, (s, dst, where, i, diff[:4].tolist(), len(diff))
                    assert all((t_ == SENTINEL).all() for t_ in tails), (s, dst, where)
    # the textures the method allocates itself
    tex, plane = random_texture(case, size[0] << 1, size[1] << 1)
    r, got = ctx.transcode_texture(tex, FORMATS[case], size[0] << 1, size[1] << 1, 1, SETS["ycocg_alpha"], alpha=plane)
    assert r == 0 and got == expected_textures(case, tex, plane, size[0] << 1, size[1] << 1, 1, "ycocg_alpha")


def test_short_outputs_and_other_sets_are_refused(ctx, hap):
    tex, plane = random_texture("ycocg_alpha", 64, 32)
    outs = [filled(16 * 8 * 16 - 1, "cuda")]
    r, _used = ctx.transcode_texture(tex, L.FMT_YCOCG, 64, 32, 0, [L.FMT_DXT5], alpha=plane, outputs=outs)
    assert r == hap.HapResult.Buffer_Too_Small and (host(outs[0]) == SENTINEL).all()
    for fmts, s, w in (([L.FMT_BC7], 0, 64), ([L.FMT_RGTC1], 0, 64), ([L.FMT_YCOCG, L.FMT_DXT5], 0, 64), ([], 0, 64),
                       ([L.FMT_DXT1], 3, 64), ([L.FMT_DXT1], 1, 68), ([L.FMT_DXT1], 2, 72)):
        outs = [filled(16 * 8 * 16, "cuda") for _ in fmts]
        r, _used = ctx.transcode_texture(tex * 2, L.FMT_YCOCG, w, 32, s, fmts, alpha=plane * 2, outputs=outs)
        assert r == hap.HapResult.Bad_Arguments, (fmts, s, w)
        assert all((host(o) == SENTINEL).all() for o in outs), (fmts, s, w)
    # a source the kernel does not read
    r, _ = ctx.transcode_texture(tex, L.FMT_BC7, 64, 32, 0, [L.FMT_DXT1])
    assert r == hap.HapResult.Bad_Arguments


# ----------------------------------------------------------------------------------------- 2. the edges of the rules --
EDGE_W, EDGE_H = 1024, 256                                   # 256 x 64 source blocks; at s = 2, 64 x 16 destination blocks
EDGE_BLOCKS = (EDGE_W // 4) * (EDGE_H // 4)


def flat_head(blocks, make):
    """The first four block rows become 4 x 4 groups of one flat block each (make(g): the block of group g): flat
    destination blocks at s = 0 and at s = 2, where the encoders' zero-length segment applies."""
    grid = blocks.reshape(EDGE_H // 4, EDGE_W // 4, -1)
    for g in range(EDGE_W // 16):
        grid[:4, 4 * g: 4 * g + 4] = np.frombuffer(make(g), np.uint8)
    return grid.reshape(len(blocks), -1)


@functools.lru_cache(maxsize=None)
def edge_texture(case):
    """(texture, plane | None) of blocks from the generators of tests/_value_space.py: alpha ramps of every endpoint
    order (a0 <= a1 among them), colour endpoints equal and in both orders, every YCoCg scale code, flat blocks."""
    i = np.arange(EDGE_BLOCKS)
    ramps = VS.ramp_blocks()[(i * 5) % 65536]
    cols = VS.colour_blocks()
    cols = cols[(i * 19) % len(cols)]
    hapq = VS.hapq_colour_blocks()
    hapq = hapq[(i * 7) % len(hapq)]
    plane = None
    if case == "dxt1":
        blocks = flat_head(cols.copy(), lambda g: np.uint16([g * 997, g * 997]).tobytes() + bytes(4))
    elif case == "dxt5":
        blocks = flat_head(np.concatenate([ramps, cols], axis=1),
                           lambda g: bytes([g * 4, g * 4]) + bytes(6) + np.uint16([g * 997, g * 997]).tobytes() + bytes(4))
    else:
        # (a flat Hap Q block: one luma, one Co and Cg, at scale code g mod 32)
        grey = lambda g: np.uint16([(16 << 11) | (32 << 5) | (g % 32)] * 2).tobytes() + bytes(4)
        blocks = flat_head(np.concatenate([ramps, hapq], axis=1), lambda g: bytes([g * 4, g * 4]) + bytes(6) + grey(g))
        if case == "ycocg_alpha":
            plane = flat_head(np.roll(ramps, 4099, axis=0).copy(), lambda g: bytes([255 - g, 255 - g]) + bytes(6)).tobytes()
    return np.ascontiguousarray(blocks).tobytes(), plane


def test_the_edge_blocks_are_what_they_claim():
    for case in SOURCES:
        tex, plane = edge_texture(case)
        blocks = np.frombuffer(tex, np.uint8).reshape(EDGE_BLOCKS, -1)
        colour = np.ascontiguousarray(blocks[:, -8:]).view("<u2")
        assert (colour[:, 0] == colour[:, 1]).any() and (colour[:, 0] < colour[:, 1]).any() and (colour[:, 0] > colour[:, 1]).any()
        if case != "dxt1":
            a0, a1 = blocks[:, 0], blocks[:, 1]
            assert (a0 == a1).any() and (a0 < a1).any() and (a0 > a1).any(), case
        if case.startswith("ycocg"):
            assert len(set((colour[:, 0] & 31).tolist())) == 32 and len(set((colour[:, 1] & 31).tolist())) == 32
            # scale bits 1 / 2 / 4 and the codes no encoder writes, through the interpolated entries too
        # flat destination blocks at both scales: the zero-length segment of the colour and of the alpha encoder
        for s in (0, 2):
            for fmt, out in zip(SETS["ycocg_alpha"], expected_textures(case, tex, plane, EDGE_W, EDGE_H, s, "ycocg_alpha")):
                b = np.frombuffer(out, np.uint8).reshape(-1, D.BLOCK_BYTES[fmt])
                assert (b[:, 0] == b[:, 1]).any(), (case, s, fmt)                          # a0 == a1
                if fmt == L.FMT_YCOCG:
                    c = np.ascontiguousarray(b[:, 8:12]).view("<u2")
                    assert (c[:, 0] == c[:, 1]).any(), (case, s)                           # c0 == c1
            c = np.frombuffer(expected_textures(case, tex, plane, EDGE_W, EDGE_H, s, "dxt1")[0], np.uint8).reshape(-1, 8).view("<u2")
            assert (c[:, 0] == c[:, 1]).any(), (case, s)


@pytest.mark.parametrize("s", (0, 2))
@pytest.mark.parametrize("case", SOURCES)
def test_the_edges_of_the_rules(ctx, case, s):
    tex, plane = edge_texture(case)
    dtex, dplane = dev(tex), dev(plane) if plane else None
    for dst in SETS:
        if s == 0 and dst == case:
            continue
        want = expected_textures(case, tex, plane, EDGE_W, EDGE_H, s, dst)
        r, got, tails, _used = transcoded(ctx, case, dtex, dplane, EDGE_W, EDGE_H, s, dst, "cuda")
        assert r == 0, dst
        for i, (g, x) in enumerate(zip(got, want)):
            diff = np.flatnonzero(np.frombuffer(g, np.uint8) != np.frombuffer(x, np.uint8))
            assert g == x, (dst, i, diff[:4].tolist(), len(diff))
        assert all((t == SENTINEL).all() for t in tails), dst


# -------------------------------------------------------------------------------------------------------- 3. frames --
FLAVOURS = {"hap": "dxt1", "hap_alpha": "dxt5", "hap_q": "ycocg", "hap_q_alpha": "ycocg_alpha"}
FRAME_GEOMETRIES = {(516, 12): (0,), (64, 64): (0, 1, 2)}    # geometry -> the scales it is a multiple of 4 << s for


def source_textures(case, w, h, i):
    """Textures of picture i, made by the CPU encoder: [colour texture] or [colour texture, plane]"""
    return [D.oracle_bc_encode(D.rgba(w, h, i), f) for f in SETS[case]]


def frames_from_textures(ctx, hap, textures, fmts, way):
    """One frame per texture set, made `way`: plain, with the fragment table, stored raw, or by the reference's HapEncode"""
    n = len(fmts)
    if way == "reference":
        out = []
        for t in textures:
            r, frame = REF.encode(t, fmts, [L.COMP_SNAPPY] * n, [1] * n)
            assert r == 0
            out.append(frame)
        return out
    sizes = [len(t) for t in textures[0]]
    bufs = [np.zeros(hap.HapMaxEncodedLength(sizes, fmts, [2] * n) + 4096, dtype=np.uint8) for _ in textures]
    r, used, res = ctx.encode_frames([[np.frombuffer(x, np.uint8) for x in t] for t in textures], fmts,
                                     [L.COMP_NONE if way == "raw" else L.COMP_SNAPPY] * n, [2] * n, bufs,
                                     flags=hap.ENCODE_FRAGMENT_INDEX if way == "index" else 0)
    assert r == 0 and res == [0] * len(textures), (way, r, res)
    return [b[:u].tobytes() for b, u in zip(bufs, used)]


def frame_textures(ctx, frames, count, cap):
    """What decode_frame_textures yields: per frame the list of its textures' bytes (None where one failed)"""
    outs = [np.zeros(cap, dtype=np.uint8) for _ in range(len(frames) * count)]
    _r, used, _fmts, res = ctx.decode_frame_textures(frames, [len(f) for f in frames], count, outs)
    return [[outs[f * count + t][: used[f * count + t]].tobytes() if res[f * count + t] == 0 else None for t in range(count)]
            for f in range(len(frames))]


def two_call_route(ctx, frames, src_count, w, h, s, fmts, comps, chunks, outputs, flags):
    """decode_frames_rgba[_scaled], then encode_frames_rgba: (result of the encode, used, results)"""
    ow, oh = w >> s, h >> s
    pics = [torch.zeros(ow * oh * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    lens = [len(f) for f in frames]
    if s:
        r, res = ctx.decode_frames_rgba_scaled(frames, lens, src_count, pics, w, h, s)
    else:
        r, res = ctx.decode_frames_rgba(frames, lens, src_count, pics, w, h)
    assert r == 0 and res == [0] * len(frames)
    return ctx.encode_frames_rgba(pics, ow, oh, ow * 4, fmts, comps, chunks, outputs, flags=flags)


@pytest.mark.parametrize("size", FRAME_GEOMETRIES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_frames_equal_the_two_call_route_and_the_cpu_definition(ctx, hap, flavour, size):
    w, h = size
    case = FLAVOURS[flavour]
    src_fmts = SETS[case]
    src_count = len(src_fmts)
    ways = ("plain", "index", "raw", "reference")
    textures = [source_textures(case, w, h, i) for i in range(3 * len(ways))]
    frames = []
    for k, way in enumerate(ways):
        frames += frames_from_textures(ctx, hap, textures[3 * k: 3 * k + 3], src_fmts, way)
    lens = [len(f) for f in frames]
    dframes = [dev(f) for f in frames]
    n = len(frames)
    combo = compared = 0
    for s in FRAME_GEOMETRIES[size]:
        ow, oh = w >> s, h >> s
        for dst, fmts in SETS.items():
            count = len(fmts)
            sizes = texture_bytes(ow, oh, fmts)
            through = s == 0 and dst == case
            want = [t if through else expected_textures(case, t[0], t[1] if src_count == 2 else None, w, h, s, dst)
                    for t in textures]
            for flags in (0, hap.ENCODE_FRAGMENT_INDEX, hap.ENCODE_FINE_CHUNKS):
                comps, chunks = [L.COMP_SNAPPY] * count, [2] * count
                cap = hap.HapMaxEncodedLength(sizes, fmts, [max(2, hap.fine_chunk_count(b, f)) for b, f in zip(sizes, fmts)]) + 4096
                combo += 1
                where = ("cuda", "cpu")[combo % 2]            # host and device buffers in turn, sources the other way round
                # (the second stage may use all of the buffer it is given -- fragments written in place before their sizes
                # are known --, as for every encode call: what lies behind the buffer is not its own)
                outs = [filled(cap + 64, where) for _ in range(n)]
                r, used, res = ctx.transcode_frames(frames if where == "cuda" else dframes, lens, src_count, w, h, s, fmts,
                                                    comps, chunks, [o[:cap] for o in outs], encode_flags=flags)
                assert r == 0 and res == [0] * n, (s, dst, flags, where, res)
                got = [host(o) for o in outs]
                assert all((g[cap:] == SENTINEL).all() for g in got), (s, dst, flags)
                got = [g[:u].tobytes() for g, u in zip(got, used)]
                # (a) the frames of the two-call route, where the frame is made anew
                if not through:
                    routes = [filled(cap, "cuda") for _ in range(n)]
                    r2, used2, res2 = two_call_route(ctx, frames, src_count, w, h, s, fmts, comps, chunks, routes, flags)
                    assert r2 == 0 and res2 == [0] * n and used == used2, (s, dst, flags, used, used2)
                    for f in range(n):
                        assert got[f] == host(routes[f])[: used2[f]].tobytes(), (s, dst, flags, f)
                    compared += n
                # (b) their textures: the CPU definition's (a frame passed through: its own)
                fallbacks = ctx.table_fallbacks()
                assert frame_textures(ctx, got, count, max(sizes)) == want, (s, dst, flags)
                assert ctx.table_fallbacks() == fallbacks, (s, dst, flags)
                # (c) ... and the reference's decoder reads the same
                if combo % 6 == 0:
                    for f in (0, n - 1):
                        for t in range(count):
                            rr, tex, fmt = REF.decode(got[f], t, out_bytes=sizes[t])
                            assert (rr, tex, fmt) == (0, want[f][t], fmts[t]), (s, dst, flags, f, t)
    print(f"{flavour} {w}x{h}: {combo} transcode calls of {n} frames, {compared} frames equal to the two-call route's")


# ----------------------------------------------------------------------- 4. a mixed batch and its per-frame results --
W, H = 64, 64


@pytest.fixture(scope="module")
def mixed(ctx, hap):
    """(frames, textures per frame, cases): Hap, Hap Alpha, Hap Q, Hap Q again, then a Hap Q frame cut short and a Hap
    frame of another geometry; all read with one texture"""
    cases = ["dxt1", "dxt5", "ycocg", "ycocg"]
    textures = [source_textures(c, W, H, 20 + i) for i, c in enumerate(cases)]
    frames = [frames_from_textures(ctx, hap, [t], SETS[c], ("plain", "index", "raw", "reference")[i])[0]
              for i, (t, c) in enumerate(zip(textures, cases))]
    cut = frames_from_textures(ctx, hap, [source_textures("ycocg", W, H, 30)], SETS["ycocg"], "plain")[0][:-3]
    other = frames_from_textures(ctx, hap, [source_textures("dxt1", 32, 32, 31)], SETS["dxt1"], "plain")[0]
    return frames + [cut, other], textures, cases


def smallest_output(ctx, hap, w, h, fmts, cap):
    """The fewest output bytes encode_frames_rgba takes for a w x h picture (two Snappy chunks a texture), by bisection"""
    pic = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    count = len(fmts)

    def taken(nbytes):
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        res = ctx.encode_frames_rgba([pic], w, h, w * 4, fmts, [L.COMP_SNAPPY] * count, [2] * count, [out])[2]
        assert res[0] in (0, hap.HapResult.Buffer_Too_Small), res
        return res[0] == 0

    lo, hi = 1, cap                                           # lo refused, hi taken
    assert taken(hi) and not taken(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if taken(mid) else (mid, hi)
    return hi


@pytest.mark.parametrize("s", (0, 2))
@pytest.mark.parametrize("dst", ("dxt1", "ycocg_alpha"))
def test_a_mixed_batch_and_per_frame_results(ctx, hap, mixed, dst, s):
    good, textures, cases = mixed
    fmts = SETS[dst]
    count = len(fmts)
    sizes = texture_bytes(W >> s, H >> s, fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [2] * count)
    # frames 0..3 good; 4 cut short; 5 of another geometry; 6 (= frame 1) with no output; 7 (= frame 2) with an output one
    # byte too small; 8 (= frame 3) good again
    frames = good + [good[1], good[2], good[3]]
    lens = [len(f) for f in frames]
    n = len(frames)
    full = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(n)]
    _r, decode_res = ctx.decode_frames_rgba(frames, lens, 1, full, W, H)
    assert decode_res[4] == hap.HapResult.Bad_Frame and decode_res[5] == hap.HapResult.Bad_Arguments
    expect = [0, 0, 0, 0, hap.HapResult.Bad_Frame, hap.HapResult.Bad_Arguments, hap.HapResult.Bad_Arguments,
              hap.HapResult.Buffer_Too_Small, 0]
    limit = smallest_output(ctx, hap, W >> s, H >> s, fmts, cap)
    want = {f: expected_textures(cases[i], textures[i][0], None, W, H, s, dst) for f, i in ((0, 0), (1, 1), (2, 2), (3, 3), (8, 3))}
    if s == 0 and dst == "dxt1":
        want[0] = textures[0]                                 # the Hap frame passes through
    for where in ("cuda", "cpu"):
        whole = [filled(cap + 64, where) for _ in range(n)]
        outs = [o[:cap] for o in whole]
        outs[6] = None
        outs[7] = outs[7][: limit - 1]
        ctx.set_profiling(True)
        ctx.collect_profile()
        r, used, res = ctx.transcode_frames(frames, lens, 1, W, H, s, fmts, [L.COMP_SNAPPY] * count, [2] * count, outs)
        prof = ctx.collect_profile()
        ctx.set_profiling(False)
        assert res == expect and r == hap.HapResult.Bad_Frame, (where, r, res)
        # one launch per source format present that has a frame to make (the Hap frame that passes through has none)
        assert prof["block_encode"][0] == (2 if s == 0 and dst == "dxt1" else 3) and prof["block_decode"][0] == 0, prof
        for f in range(n):
            got = host(whole[f])
            if f in want:
                assert (got[cap:] == SENTINEL).all(), (where, f)
                assert frame_textures(ctx, [got[: used[f]].tobytes()], count, max(sizes))[0] == want[f], (where, f)
            else:
                assert used[f] == 0 and (got == SENTINEL).all(), (where, f)
    # ... and an output of exactly the smallest size is taken
    outs = [filled(limit, "cuda")]
    r, used, res = ctx.transcode_frames(frames[2:3], lens[2:3], 1, W, H, s, fmts, [L.COMP_SNAPPY] * count, [2] * count, outs)
    assert (r, res) == (0, [0]) and 0 < used[0] <= limit


@pytest.mark.parametrize("where", ("cuda", "cpu"))
def test_a_truncated_frame_between_two_good_ones(ctx, hap, mixed, where):
    """Three frames, the middle one cut short: its result is its decode's code, nothing of its output is written and its
    outputBuffersBytesUsed entry is 0; its neighbours' frames are made as if it were not there"""
    good, textures, cases = mixed
    fmts = SETS["dxt5"]
    sizes = texture_bytes(W, H, fmts)
    cap = hap.HapMaxEncodedLength(sizes, fmts, [2])
    frames = [good[2], good[4], good[3]]
    lens = [len(f) for f in frames]
    _r, decode_res = ctx.decode_frames_rgba(frames, lens, 1, [np.zeros(W * H * 4, dtype=np.uint8) for _ in frames], W, H)
    code = decode_res[1]
    assert decode_res == [0, hap.HapResult.Bad_Frame, 0]
    whole = [filled(cap + 64, where) for _ in frames]
    r, used, res = ctx.transcode_frames(frames, lens, 1, W, H, 0, fmts, [L.COMP_SNAPPY], [2], [o[:cap] for o in whole])
    assert r == code and res == [0, code, 0]
    assert used[1] == 0 and (host(whole[1]) == SENTINEL).all()
    for f, i in ((0, 2), (2, 3)):
        got = host(whole[f])
        assert 0 < used[f] <= cap and (got[cap:] == SENTINEL).all(), f
        want = expected_textures(cases[i], textures[i][0], None, W, H, 0, "dxt5")
        assert frame_textures(ctx, [got[: used[f]].tobytes()], 1, max(sizes))[0] == want, f


# -------------------------------------------------------------------------------------------------- 5. pass-through --
def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def foreign(ctx, hap):
    """name -> (frame, its formats, its textures): Hap R, Hap HDR (unsigned) and Hap Alpha-Only frames of random
    textures, and a Hap Q frame made by the reference's HapEncode"""
    nb = (W // 4) * (H // 4)
    out = {}
    for name, fmt in (("bc7", L.FMT_BC7), ("bc6h", L.FMT_BC6U), ("rgtc1", L.FMT_RGTC1)):
        tex = random_bytes(nb * D.BLOCK_BYTES[fmt], [5, fmt])
        out[name] = (frames_from_textures(ctx, hap, [[tex]], [fmt], "plain")[0], [fmt], [tex])
    tex = source_textures("ycocg", W, H, 40)
    out["hap_q"] = (frames_from_textures(ctx, hap, [tex], [L.FMT_YCOCG], "reference")[0], [L.FMT_YCOCG], tex)
    return out


@pytest.mark.parametrize("name", ("bc7", "bc6h", "rgtc1", "hap_q"))
def test_a_frame_of_the_wanted_formats_passes_through(ctx, hap, foreign, name):
    frame, fmts, textures = foreign[name]
    sizes = [len(t) for t in textures]
    bad = hap.HapResult.Bad_Arguments
    for flags in (hap.ENCODE_FRAGMENT_INDEX, hap.ENCODE_FINE_CHUNKS):
        cap = hap.HapMaxEncodedLength(sizes, fmts, [max(2, hap.fine_chunk_count(sizes[0], fmts[0]))]) + 4096
        for where in ("cuda", "cpu"):
            outs = [filled(cap, where), filled(cap, where)]
            r, used, res = ctx.transcode_frames([frame, dev(frame)], [len(frame)] * 2, 1, W, H, 0, fmts, [L.COMP_SNAPPY], [2],
                                                outs, encode_flags=flags)
            assert r == 0 and res == [0, 0], (flags, where, res)
            made = [host(o)[:u].tobytes() for o, u in zip(outs, used)]
            fallbacks = ctx.table_fallbacks()
            assert frame_textures(ctx, made, 1, sizes[0]) == [textures, textures], (flags, where)
            assert ctx.table_fallbacks() == fallbacks
            # what the encoder's second stage makes of the same textures
            direct = [np.zeros(cap, dtype=np.uint8)]
            r, dused, dres = ctx.encode_frames([[np.frombuffer(textures[0], np.uint8)]], fmts, [L.COMP_SNAPPY], [2], direct,
                                               flags=flags)
            assert r == 0 and dres == [0] and made[0] == direct[0][: dused[0]].tobytes(), (flags, where)
    # no other flavour can become one of these, and none of them another size
    outs = [filled(cap, "cuda")]
    if name != "hap_q":
        r, used, res = ctx.transcode_frames([frame], [len(frame)], 1, W, H, 1, fmts, [L.COMP_SNAPPY], [2], outs)
        assert (r, res) == (bad, [bad]) and (host(outs[0]) == SENTINEL).all()
        other = foreign["hap_q"][0]
        r, used, res = ctx.transcode_frames([other, frame], [len(other), len(frame)], 1, W, H, 0, fmts, [L.COMP_SNAPPY], [2],
                                            [outs[0], filled(cap, "cuda")])
        assert (r, res) == (bad, [bad, 0]) and (host(outs[0]) == SENTINEL).all()
        # ... nor be read by the kernel
        r, used, res = ctx.transcode_frames([frame], [len(frame)], 1, W, H, 0, [L.FMT_DXT1], [L.COMP_SNAPPY], [2], outs)
        assert (r, res) == (bad, [bad]) and (host(outs[0]) == SENTINEL).all()


# ------------------------------------------------------------------------------------------------- 6. argument rules --
def test_argument_rules(ctx, hap, foreign, mixed):
    bad = hap.HapResult.Bad_Arguments
    frames = mixed[0][:3]
    lens = [len(f) for f in frames]
    snappy, two = [L.COMP_SNAPPY], [2]

    def refused(w, h, s, fmts, src_count=1, comps=None, chunks=None, code=bad):
        outs = [filled(1 << 16, "cuda") for _ in frames]
        k = max(1, len(fmts))
        r, used, res = ctx.transcode_frames(frames, lens, src_count, w, h, s, fmts, comps or snappy * k, chunks or two * k, outs)
        assert (r, res) == (code, [code] * len(frames)), (w, h, s, fmts, src_count, r, res)
        assert all((host(o) == SENTINEL).all() for o in outs), (w, h, s, fmts, src_count)

    refused(W, H, 3, [L.FMT_DXT1])                            # scaleLog2 3
    refused(W + 4, H, 1, [L.FMT_DXT1])                        # a width that is a multiple of 4 but not of 4 << s
    refused(W, H + 8, 2, [L.FMT_DXT1])
    refused(W, H, 0, [])                                      # count 0
    refused(W, H, 0, [L.FMT_YCOCG, L.FMT_RGTC1, L.FMT_DXT1])  # count 3
    refused(W, H, 0, [L.FMT_DXT1], src_count=3)               # sourceTextureCount 3
    refused(W, H, 0, [L.FMT_DXT1], src_count=0)
    refused(W, H, 1, [L.FMT_BC7])                             # a BC7 destination at s = 1
    refused(W, H, 1, [L.FMT_RGTC1, L.FMT_YCOCG])              # the pair the other way round: legal at s = 0 only
    refused(W, H, 0, [0x1234])                                # what HapEncode refuses
    refused(W, H, 0, [L.FMT_DXT1], comps=[7])
    refused(W, H, 0, [L.FMT_DXT1], chunks=[0])
    # a NULL array
    lib = hap._lib.lib
    res = (C.c_uint * 2)(77, 77)
    one = (C.c_uint * 1)(1)
    fmt = (C.c_uint * 1)(L.FMT_DXT1)
    assert lib.HapGpuTranscodeFrames(ctx.handle, 2, None, None, 1, W, H, 0, 1, fmt, one, one, None, None, None, res, 0, 0) == bad
    assert list(res) == [bad, bad]
    # a context with an encode call begun and not finished
    pic = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    out = filled(1 << 16, "cuda")
    assert ctx.encode_frames_rgba_begin([pic], W, H, W * 4, [L.FMT_DXT1], snappy, two, [out]) == 0
    try:
        refused(W, H, 0, [L.FMT_DXT5], code=hap.HapResult.Internal_Error)
        tex, _plane = random_texture("dxt1", 8, 4)
        r, _ = ctx.transcode_texture(tex, L.FMT_DXT1, 8, 4, 0, [L.FMT_DXT5])
        assert r == hap.HapResult.Internal_Error
    finally:
        r, _used, res = ctx.encode_finish()
    assert r == 0 and res == [0]
    # ... and takes calls again afterwards
    outs = [filled(1 << 16, "cuda") for _ in frames]
    r, used, res = ctx.transcode_frames(frames, lens, 1, W, H, 1, [L.FMT_DXT5], snappy, two, outs)
    assert r == 0 and res == [0, 0, 0]


# --------------------------------------------------------------------------------------------------------- 7. slicing --
def test_more_frames_than_one_slice_holds(ctx, hap):
    """A call transcodes its frames 32768 at a time; outputs and their sizes are the call's.  32768 + 40 Hap Alpha frames
    of 8 x 4 texels to Hap, cycling through 5 frames of random blocks and 7 output sizes -- 32768 is 1 modulo 7, so an
    output looked up by a frame's place in its slice is another frame's, with or without room."""
    w, h, fmts = 8, 4, [L.FMT_DXT1]
    n = 32768 + 40
    made = []
    for i in range(5):
        r, frame = hap.HapEncode([random_bytes(32, 70 + i)], [L.FMT_DXT5], [L.COMP_SNAPPY], [1])
        assert r == 0
        made.append(frame)
    room = (True, False, True, True, False, False, True)
    cap = hap.HapMaxEncodedLength(texture_bytes(w, h, fmts), fmts, [1])
    # what a call of the five makes of each, with room and with none
    small = filled(5 * cap, "cuda").reshape(5, cap)
    lens5 = [len(f) for f in made]
    r, used5, res5 = ctx.transcode_frames(made, lens5, 1, w, h, 0, fmts, [L.COMP_SNAPPY], [1], list(small))
    assert r == 0 and res5 == [0] * 5
    small = host(small)
    want = [small[i, : used5[i]].tobytes() for i in range(5)]
    assert len(set(want)) == 5 and all((small[i, used5[i]:] == SENTINEL).all() for i in range(5))
    none = filled(5 * cap, "cuda").reshape(5, cap)
    _r, none_used, none_res = ctx.transcode_frames(made, lens5, 1, w, h, 0, fmts, [L.COMP_SNAPPY], [1], [row[:0] for row in none])
    assert all(code != 0 for code in none_res) and none_used == [0] * 5 and (host(none) == SENTINEL).all()
    # the frames in device memory, behind each other at 256-byte steps
    step = 256
    assert max(lens5) <= step
    store = np.zeros(5 * step, dtype=np.uint8)
    for i, f in enumerate(made):
        store[i * step: i * step + len(f)] = np.frombuffer(f, np.uint8)
    store = torch.from_numpy(store).cuda()
    frames = [store[(f % 5) * step: (f % 5 + 1) * step] for f in range(n)]
    out = filled(n * cap, "cuda").reshape(n, cap)
    outputs = [out[f] if room[f % 7] else out[f, :0] for f in range(n)]
    r, used, res = ctx.transcode_frames(frames, [lens5[f % 5] for f in range(n)], 1, w, h, 0, fmts, [L.COMP_SNAPPY], [1], outputs)
    got = host(out)
    f = np.arange(n)
    has_room = np.array(room)[f % 7]
    assert r == none_res[np.argmin(has_room) % 5]                    # (the first frame that fails)
    assert res == [0 if has_room[i] else none_res[i % 5] for i in range(n)]
    assert used == [used5[i % 5] if has_room[i] else 0 for i in range(n)]
    expect = np.full((5, cap), SENTINEL, dtype=np.uint8)
    for i in range(5):
        expect[i, : used5[i]] = np.frombuffer(want[i], np.uint8)
    wrong = np.argwhere((got != np.where(has_room[:, None], expect[f % 5], SENTINEL)).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()

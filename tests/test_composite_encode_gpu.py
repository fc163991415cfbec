"""Layers composited straight to block textures and to Hap frames on the GPU (HapGpuCompositeTexturesEncoded,
HapGpuCompositeFramesEncoded).  The definition: the output is byte for byte what the encoder makes of the picture the
placed compositing call writes for the same layers.  Every expected texture is made on the CPU alone --
tests/_data.oracle_bc_decode per layer (the RGTC1 plane into A), tests/_composite_placed.composite_placed for the canvas,
tests/_data.oracle_bc_encode per destination format -- and every expected frame is the frame of the two-call route; every
comparison is byte for byte.  Outputs lie in sentinel-filled buffers, and what is not the call's to write stays
sentinel."""
import functools

import numpy as np
import pytest

import _composite_placed as KP
import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
SOURCES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
SETS = {"dxt1": [L.FMT_DXT1], "dxt5": [L.FMT_DXT5], "ycocg": [L.FMT_YCOCG], "ycocg_alpha": [L.FMT_YCOCG, L.FMT_RGTC1]}
# canvases: one lane; the smallest two-lane grids; exactly one wave per block row; a one-lane second wave in each row
CANVASES = ((4, 4), (8, 4), (4, 8), (256, 8), (260, 12))
OPACITIES = (0, 1, 128, 255)
BACKGROUNDS = ((0, 0, 0, 255), (10, 200, 30, 77))
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
    if data is None:
        return None
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


def cpu_picture(case, tex, plane, w, h):
    """What the decoder writes for a layer, by the CPU alone: [h, w, 4]"""
    pic = D.oracle_bc_decode(tex, FORMATS[case], w, h)
    if plane is not None:
        pic[..., 3] = D.oracle_bc_decode(plane, L.FMT_RGTC1, w, h)
    return np.ascontiguousarray(pic)


def cpu_textures(canvas_size, pictures, placements, opacities, background, dst):
    """The CPU definition: the placed canvas, encoded per destination format as it is"""
    canvas = np.ascontiguousarray(KP.composite_placed(canvas_size, pictures, placements, opacities, background))
    return [D.oracle_bc_encode(canvas, f) for f in SETS[dst]]


@functools.lru_cache(maxsize=None)
def random_layer(case, w, h, slot=0):
    """Seeded random bytes: any 8 / 16 bytes are a block.  (texture, plane | None, its CPU picture), made once"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([47, SOURCES.index(case), w, h, slot])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    pic = cpu_picture(case, tex, plane, w, h)
    pic.setflags(write=False)
    return tex, plane, pic


@functools.lru_cache(maxsize=None)
def device_layer(case, w, h, slot=0):
    tex, plane, _pic = random_layer(case, w, h, slot)
    return dev(tex), FORMATS[case], dev(plane)


def host_layer(case, w, h, slot=0):
    tex, plane, _pic = random_layer(case, w, h, slot)
    return tex, FORMATS[case], plane


def encoded(ctx, layers, sizes, canvas_size, placements, opacities, background, dst, where):
    """composite_textures_encoded into sentinel-filled outputs 64 bytes too long: the textures"""
    w, h = canvas_size
    need = texture_bytes(w, h, SETS[dst])
    outs = [filled(n + 64, where) for n in need]
    r, used = ctx.composite_textures_encoded(layers, sizes, w, h, SETS[dst], placements=placements, opacities=opacities,
                                             background=background, outputs=outs)
    assert r == 0 and used == need, (r, used, need)
    got = [host(o) for o in outs]
    assert all((g[n:] == SENTINEL).all() for g, n in zip(got, need))
    return [g[:n].tobytes() for g, n in zip(got, need)]


def two_calls_textures(ctx, layers, sizes, canvas_size, placements, opacities, background, dst):
    """composite_textures_placed, then compress_rgba per destination format, on the GPU"""
    w, h = canvas_size
    picture = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    r, _ = ctx.composite_textures_placed(layers, sizes, w, h, placements=placements, opacities=opacities,
                                         background=background, rgba=picture)
    assert r == 0
    out = []
    for f in SETS[dst]:
        r, tex = ctx.compress_rgba(picture, w, h, w * 4, f)
        assert r == 0
        out.append(tex)
    return out


def same(got, want, what):
    for i, (g, x) in enumerate(zip(got, want)):
        diff = np.flatnonzero(np.frombuffer(g, np.uint8) != np.frombuffer(x, np.uint8)) if len(g) == len(x) else None
        assert g == x, (what, i, len(g), len(x), None if diff is None else (diff[:4].tolist(), len(diff)))
    assert len(got) == len(want), what


# ------------------------------------------------------------- 1. the kernel, every source kind x every destination set --
def test_the_random_blocks_reach_both_palette_modes():
    tex = np.frombuffer(random_layer("dxt1", 260, 12)[0], np.uint8).view("<u2").reshape(-1, 4)
    assert (tex[:, 0] <= tex[:, 1]).any() and (tex[:, 0] > tex[:, 1]).any()          # three- and four-colour DXT1
    for case, part in (("dxt5", 0), ("ycocg", 0), ("ycocg_alpha", 1)):
        blocks = np.frombuffer(random_layer(case, 260, 12)[part], np.uint8).reshape(-1, 16 if part == 0 else 8)
        assert (blocks[:, 0] <= blocks[:, 1]).any() and (blocks[:, 0] > blocks[:, 1]).any(), case   # both ramp orders


def stack_b(canvas_size):
    """Three layers: (cases, sizes, placements) -- a 64 x 16 layer with an alpha plane, a rectangle from inside it clipped
    at the canvas's left and top edges (a first block that is not 0, blocks per row of its own); a DXT5 layer that hangs
    over the right and the bottom edge; a layer wholly outside"""
    W, H = canvas_size
    cases = ("ycocg_alpha", "dxt5", "dxt1")
    sizes = ((64, 16), (16, 8), (8, 8))
    placements = ((8, 4, 32, 8, -8, -4), (0, 0, 16, 8, max(W - 8, 0), max(H - 4, 0)), (0, 0, 8, 8, W, 0))
    assert KP.visible(placements[0], canvas_size) and KP.visible(placements[1], canvas_size)
    assert placements[1][4] + 16 > W and placements[1][5] + 8 > H and KP.visible(placements[2], canvas_size) is None
    return cases, sizes, placements


@pytest.mark.parametrize("canvas_size", CANVASES, ids=lambda g: "%dx%d" % g)
def test_every_source_kind_to_every_destination_set(ctx, canvas_size):
    W, H = canvas_size
    turn = 0
    # stack A: a single whole layer of each source kind, of the canvas's size
    for case in SOURCES:
        pic = random_layer(case, W, H)[2]
        for dst in SETS:
            for background in BACKGROUNDS:
                for opacity in OPACITIES:
                    want = cpu_textures(canvas_size, [pic], None, [opacity], background, dst)
                    for where in ("cuda", "cpu"):
                        turn += 1
                        layer = device_layer(case, W, H) if turn % 3 else host_layer(case, W, H)
                        got = encoded(ctx, [layer], [canvas_size], canvas_size, None, [opacity], background, dst, where)
                        same(got, want, ("A", case, dst, background, opacity, where))
                    gpu = two_calls_textures(ctx, [device_layer(case, W, H)], [canvas_size], canvas_size, None, [opacity],
                                             background, dst)
                    same(gpu, want, ("A, two calls", case, dst, background, opacity))
    # stack B: three placed layers
    cases, sizes, placements = stack_b(canvas_size)
    pictures = [random_layer(c, w, h, 1)[2] for c, (w, h) in zip(cases, sizes)]
    for dst in SETS:
        for background in BACKGROUNDS:
            for k, opacity in enumerate(OPACITIES):
                opacities = [opacity, OPACITIES[(k + 2) % 4], 200]
                want = cpu_textures(canvas_size, pictures, placements, opacities, background, dst)
                for where in ("cuda", "cpu"):
                    turn += 1
                    layers = [device_layer(c, w, h, 1) if (turn + i) % 3 else host_layer(c, w, h, 1)
                              for i, (c, (w, h)) in enumerate(zip(cases, sizes))]
                    got = encoded(ctx, layers, sizes, canvas_size, placements, opacities, background, dst, where)
                    same(got, want, ("B", dst, background, opacities, where))
                layers = [device_layer(c, w, h, 1) for c, (w, h) in zip(cases, sizes)]
                gpu = two_calls_textures(ctx, layers, sizes, canvas_size, placements, opacities, background, dst)
                same(gpu, want, ("B, two calls", dst, background, opacities))
    # the textures the method allocates itself, and two calls give the same bytes
    layers = [host_layer(c, w, h, 1) for c, (w, h) in zip(cases, sizes)]
    r, first = ctx.composite_textures_encoded(layers, sizes, W, H, SETS["ycocg_alpha"], placements=placements, opacities=[255, 128, 7],
                                              background=BACKGROUNDS[1])
    r2, second = ctx.composite_textures_encoded(layers, sizes, W, H, SETS["ycocg_alpha"], placements=placements,
                                                opacities=[255, 128, 7], background=BACKGROUNDS[1])
    assert r == 0 and r2 == 0 and first == second
    same(first, cpu_textures(canvas_size, pictures, placements, [255, 128, 7], BACKGROUNDS[1], "ycocg_alpha"), "own outputs")


def test_short_and_missing_outputs_are_refused(ctx, hap):
    layer = device_layer("dxt5", 64, 32)
    need = texture_bytes(64, 32, SETS["ycocg_alpha"])
    for short in (0, 1):
        outs = [filled(n - (1 if i == short else 0), "cuda") for i, n in enumerate(need)]
        r, _used = ctx.composite_textures_encoded([layer], [(64, 32)], 64, 32, SETS["ycocg_alpha"], outputs=outs)
        assert r == hap.HapResult.Buffer_Too_Small and all((host(o) == SENTINEL).all() for o in outs), short
    outs = [filled(need[0], "cuda"), None]
    r, _used = ctx.composite_textures_encoded([layer], [(64, 32)], 64, 32, SETS["ycocg_alpha"], outputs=outs)
    assert r == hap.HapResult.Bad_Arguments and (host(outs[0]) == SENTINEL).all()
    # a layer the kernel does not read, and a short one
    outs = [filled(need[0], "cuda")]
    r, _used = ctx.composite_textures_encoded([(layer[0], L.FMT_BC7, None)], [(64, 32)], 64, 32, SETS["ycocg"], outputs=outs)
    assert r == hap.HapResult.Bad_Arguments and (host(outs[0]) == SENTINEL).all()
    r, _used = ctx.composite_textures_encoded([(layer[0][:-16], L.FMT_DXT5, None)], [(64, 32)], 64, 32, SETS["ycocg"], outputs=outs)
    assert r == hap.HapResult.Bad_Arguments and (host(outs[0]) == SENTINEL).all()


def test_everything_in_host_memory_is_everything_in_device_memory(ctx):
    """The textures form stages what lies in host memory: two layers of different sizes, one of them with an alpha plane,
    and a two-texture destination, all in host memory, give the bytes of the same call with all of them in device
    memory -- the CPU definition's"""
    canvas_size = (260, 12)
    cases, sizes, placements = (part[:2] for part in stack_b(canvas_size))
    assert cases == ("ycocg_alpha", "dxt5") and sizes[0] != sizes[1]
    opacities, background = [200, 255], BACKGROUNDS[1]
    on_host = encoded(ctx, [host_layer(c, w, h, 1) for c, (w, h) in zip(cases, sizes)], sizes, canvas_size, placements,
                      opacities, background, "ycocg_alpha", "cpu")
    on_device = encoded(ctx, [device_layer(c, w, h, 1) for c, (w, h) in zip(cases, sizes)], sizes, canvas_size, placements,
                        opacities, background, "ycocg_alpha", "cuda")
    assert len(on_host) == 2
    same(on_host, on_device, "host against device")
    pictures = [random_layer(c, w, h, 1)[2] for c, (w, h) in zip(cases, sizes)]
    same(on_host, cpu_textures(canvas_size, pictures, placements, opacities, background, "ycocg_alpha"), "host against the CPU")


# ------------------------------------------------------------------------------------------------- 2. the shortcuts --
def test_an_opaque_layer_replaces_what_is_below(ctx):
    """Opaque at opacity 255: the canvas is replaced, lane by lane, whatever lies below -- here every kind of layer at
    full opacity over a background that is not opaque"""
    size = (260, 12)
    below = [random_layer(c, 260, 12, 2) for c in ("dxt5", "ycocg_alpha", "ycocg")]
    for top in ("dxt1", "ycocg"):
        cover = random_layer(top, 260, 12, 3)
        layers = [device_layer(c, 260, 12, 2) for c in ("dxt5", "ycocg_alpha", "ycocg")] + [device_layer(top, 260, 12, 3)]
        pictures = [b[2] for b in below] + [cover[2]]
        for dst in SETS:
            got = encoded(ctx, layers, [size] * 4, size, None, [255, 200, 255, 255], BACKGROUNDS[1], dst, "cuda")
            same(got, cpu_textures(size, pictures, None, [255, 200, 255, 255], BACKGROUNDS[1], dst), (top, dst))
            # ... which is the encoder's texture of the top layer's picture alone
            same(got, [D.oracle_bc_encode(np.ascontiguousarray(cover[2]), f) for f in SETS[dst]], (top, dst, "alone"))
        # the replace is masked: a rectangle of the top layer, the stack below everywhere else
        placements = [KP.whole(size)] * 3 + [(4, 4, 128, 4, 68, 4)]
        got = encoded(ctx, layers, [size] * 4, size, placements, [255, 200, 255, 255], BACKGROUNDS[1], "ycocg_alpha", "cuda")
        same(got, cpu_textures(size, pictures, placements, [255, 200, 255, 255], BACKGROUNDS[1], "ycocg_alpha"), (top, "masked"))


def test_a_layer_of_opacity_0_is_not_looked_at(ctx):
    """Opacity 0 keeps every texel whatever the layer holds: device memory of the right size that nobody has written
    blocks into, here every byte 0xFF, stands for it"""
    size = (256, 8)
    pictures = [random_layer("dxt5", 256, 8, 4)[2], None, random_layer("ycocg_alpha", 64, 16, 4)[2]]
    for case in ("dxt5", "ycocg_alpha"):
        nb = (256 // 4) * (8 // 4)
        blank = torch.full((nb * 16,), 0xFF, dtype=torch.uint8, device="cuda")
        blank_plane = torch.full((nb * 8,), 0xFF, dtype=torch.uint8, device="cuda") if case == "ycocg_alpha" else None
        torch.cuda.synchronize()
        pictures[1] = cpu_picture(case, bytes([0xFF]) * (nb * 16), None if blank_plane is None else bytes([0xFF]) * (nb * 8), 256, 8)
        layers = [device_layer("dxt5", 256, 8, 4), (blank, FORMATS[case], blank_plane), device_layer("ycocg_alpha", 64, 16, 4)]
        sizes = [size, size, (64, 16)]
        placements = [KP.whole(size), KP.whole(size), (0, 0, 64, 16, 100, -4)]
        for dst in ("dxt5", "ycocg_alpha"):
            got = encoded(ctx, layers, sizes, size, placements, [255, 0, 99], BACKGROUNDS[1], dst, "cuda")
            same(got, cpu_textures(size, pictures, placements, [255, 0, 99], BACKGROUNDS[1], dst), (case, dst))
            same(got, cpu_textures(size, [pictures[0], pictures[2]], [placements[0], placements[2]], [255, 99], BACKGROUNDS[1], dst),
                 (case, dst, "without it"))


def test_sixteen_layers(ctx, hap):
    size = (68, 12)
    cases = [SOURCES[i % 4] for i in range(16)]
    sizes = [((16, 8), (68, 12), (8, 16), (128, 4))[i % 4] for i in range(16)]
    rng = np.random.default_rng(5)
    placements, opacities = [], []
    for (w, h) in sizes:
        rw, rh = 4 * int(rng.integers(1, w // 4 + 1)), 4 * int(rng.integers(1, h // 4 + 1))
        sx, sy = 4 * int(rng.integers(0, (w - rw) // 4 + 1)), 4 * int(rng.integers(0, (h - rh) // 4 + 1))
        placements.append((sx, sy, rw, rh, 4 * int(rng.integers(-4, 18)), 4 * int(rng.integers(-2, 4))))
        opacities.append(int(rng.integers(0, 256)))
    pictures = [random_layer(c, w, h, 5 + i)[2] for i, (c, (w, h)) in enumerate(zip(cases, sizes))]
    layers = [device_layer(c, w, h, 5 + i) for i, (c, (w, h)) in enumerate(zip(cases, sizes))]
    assert sum(KP.visible(p, size) is not None for p in placements) >= 8
    for dst in SETS:
        for background in BACKGROUNDS:
            got = encoded(ctx, layers, sizes, size, placements, opacities, background, dst, "cuda")
            same(got, cpu_textures(size, pictures, placements, opacities, background, dst), (dst, background))
    outs = [filled(texture_bytes(68, 12, SETS["dxt1"])[0], "cuda")]
    r, _used = ctx.composite_textures_encoded(layers + layers[:1], sizes + sizes[:1], 68, 12, SETS["dxt1"], outputs=outs)
    assert r == hap.HapResult.Bad_Arguments and (host(outs[0]) == SENTINEL).all()      # seventeen


# -------------------------------------------------------------------------------- 3. frames equal the two-call route --
FLAVOURS = {"hap": "dxt1", "hap_alpha": "dxt5", "hap_q": "ycocg", "hap_q_alpha": "ycocg_alpha"}
FRAME_CANVASES = ((64, 64), (516, 12))


@functools.lru_cache(maxsize=None)
def picture_layer(hap, case, w, h, i):
    """Picture i encoded by the CPU encoder, as one Hap frame: (frame, texture count, its CPU picture)"""
    textures = [D.oracle_bc_encode(D.rgba(w, h, i), f) for f in SETS[case]]
    r, frame = hap.HapEncode(textures, SETS[case], [L.COMP_SNAPPY] * len(textures), [1] * len(textures))
    assert r == 0
    pic = cpu_picture(case, textures[0], textures[1] if len(textures) == 2 else None, w, h)
    pic.setflags(write=False)
    return frame, len(textures), pic


def frame_stack(hap, canvas_size, layer_count, frames):
    """`frames` output frames of two or three layers: a Hap Q Alpha layer of the canvas's size, a Hap Alpha inset that moves
    and hangs over an edge, a Hap layer wider than the canvas of which a window is shown.
    (frames, texture counts, sizes, placements, opacities, pictures per output frame)"""
    W, H = canvas_size
    kinds = (("ycocg_alpha", (W, H)), ("dxt5", (32, 8)), ("dxt1", (W + 64, 8)))[:layer_count]
    sizes = [s for _c, s in kinds]
    made = [[picture_layer(hap, c, s[0], s[1], 10 * l + f) for l, (c, s) in enumerate(kinds)] for f in range(frames)]
    placements = [[None, (0, 0, 32, 8, W - 16 - 4 * f, 4 * f - 4), (32, 0, W, 8, 0, H - 8 if H > 8 else 0)][:layer_count]
                  for f in range(frames)]
    placements = [[KP.whole(sizes[l]) if p is None else p for l, p in enumerate(fr)] for fr in placements]
    opacities = [[255, 64 + 90 * f, 200][:layer_count] for f in range(frames)]
    return ([[m[0] for m in fr] for fr in made], [k[1] for k in made[0]], sizes, placements, opacities,
            [[m[2] for m in fr] for fr in made])


def two_call_route(ctx, stack, canvas_size, fmts, comps, chunks, outputs, flags, background):
    """composite_frames_placed into device pictures, then encode_frames_rgba: (result, used, results)"""
    frames, counts, sizes, placements, opacities, _pictures = stack
    W, H = canvas_size
    pics = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    r, res = ctx.composite_frames_placed(frames, None, counts, sizes, pics, W, H, placements=placements, opacities=opacities,
                                         background=background)
    assert r == 0 and res == [0] * (len(frames) * len(sizes)), res
    return ctx.encode_frames_rgba(pics, W, H, W * 4, fmts, comps, chunks, outputs, flags=flags)


@pytest.mark.parametrize("canvas_size", FRAME_CANVASES, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_frames_equal_the_two_call_route_and_the_cpu_definition(ctx, hap, flavour, canvas_size):
    W, H = canvas_size
    dst = FLAVOURS[flavour]
    fmts = SETS[dst]
    count = len(fmts)
    sizes_out = texture_bytes(W, H, fmts)
    n = 2
    combo = 0
    for layer_count in (2, 3):
        stack = frame_stack(hap, canvas_size, layer_count, n)
        frames, counts, sizes, placements, opacities, pictures = stack
        dframes = [[dev(b) for b in fr] for fr in frames]
        for background in BACKGROUNDS[: 1 if layer_count == 2 else 2]:
            want = [cpu_textures(canvas_size, pictures[f], placements[f], opacities[f], background, dst) for f in range(n)]
            for comp in (L.COMP_NONE, L.COMP_SNAPPY):
                for chunk in (1, 4):
                    for flags in (0, hap.ENCODE_FRAGMENT_INDEX):
                        comps, chunks = [comp] * count, [chunk] * count
                        cap = hap.HapMaxEncodedLength(sizes_out, fmts, chunks) + 4096
                        combo += 1
                        where = ("cuda", "cpu")[combo % 2]     # host and device outputs in turn, the layers' frames the other way
                        outs = [filled(cap + 64, where) for _ in range(n)]
                        r, used, res, layer_res = ctx.composite_frames_encoded(
                            frames if where == "cuda" else dframes, None, counts, sizes, W, H, fmts, comps, chunks,
                            [o[:cap] for o in outs], placements=placements, opacities=opacities, background=background,
                            encode_flags=flags)
                        what = (layer_count, background, comp, chunk, flags, where)
                        assert r == 0 and res == [0] * n and layer_res == [0] * (n * layer_count), (what, r, res, layer_res)
                        got = [host(o) for o in outs]
                        assert all((g[cap:] == SENTINEL).all() for g in got), what
                        got = [g[:u].tobytes() for g, u in zip(got, used)]
                        # (a) the frames of the two-call route
                        routes = [filled(cap, "cuda") for _ in range(n)]
                        r2, used2, res2 = two_call_route(ctx, stack, canvas_size, fmts, comps, chunks, routes, flags, background)
                        assert r2 == 0 and res2 == [0] * n and used == used2, (what, used, used2)
                        for f in range(n):
                            assert got[f] == host(routes[f])[: used2[f]].tobytes(), (what, f)
                        # (b) their textures, read by the reference's decoder: the CPU definition's
                        for f in range(n):
                            for t in range(count):
                                rr, tex, fmt = REF.decode(got[f], t, out_bytes=sizes_out[t])
                                assert (rr, fmt) == (0, fmts[t]), (what, f, t, rr, fmt)
                                same([tex], [want[f][t]], (what, f, t))
    # the flags the definition masks off change nothing
    outs = [filled(cap, "cuda") for _ in range(n)]
    r, used3, res, _layer_res = ctx.composite_frames_encoded(
        frames, None, counts, sizes, W, H, fmts, comps, chunks, outs, placements=placements, opacities=opacities,
        background=background, encode_flags=flags | hap.ENCODE_BPTC_BLOCKS | hap.ENCODE_REFINE_ENDPOINTS)
    assert r == 0 and res == [0] * n and used3 == used
    assert [host(o)[:u].tobytes() for o, u in zip(outs, used3)] == got


# ----------------------------------------------------------------------- 4. a mixed batch and its per-frame results --
MW, MH = 64, 64


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


@pytest.mark.parametrize("dst", ("dxt1", "ycocg_alpha"))
def test_a_mixed_batch_and_per_frame_results(ctx, hap, dst):
    ok, bad, bad_frame, too_small = 0, hap.HapResult.Bad_Arguments, hap.HapResult.Bad_Frame, hap.HapResult.Buffer_Too_Small
    fmts = SETS[dst]
    count = len(fmts)
    sizes_out = texture_bytes(MW, MH, fmts)
    cap = hap.HapMaxEncodedLength(sizes_out, fmts, [2] * count)
    sizes = [(MW, MH), (32, 32)]
    counts = [1, 1]
    bottoms = [picture_layer(hap, "ycocg", MW, MH, 50 + f) for f in range(8)]
    insets = [picture_layer(hap, "dxt5", 32, 32, 60 + f) for f in range(8)]
    frames = [[b[0], i[0]] for b, i in zip(bottoms, insets)]
    # 1: the inset's frame cut short; 2: an inset of another size; 3: a Hap R inset; 4: no output; 5: an output one byte
    # too small; 0, 6 and 7 good
    frames[1][1] = frames[1][1][:-3]
    frames[2][1] = picture_layer(hap, "dxt5", 16, 16, 70)[0]
    nb = (32 // 4) * (32 // 4)
    r, hap_r = hap.HapEncode([np.random.default_rng(9).integers(0, 256, nb * 16, dtype=np.uint8).tobytes()], [L.FMT_BC7],
                             [L.COMP_SNAPPY], [1])
    assert r == 0
    frames[3][1] = hap_r
    placements = [[KP.whole(sizes[0]), (0, 0, 32, 32, 8 * f, 40 - 4 * f)] for f in range(8)]
    opacities = [[255, 30 * f + 20] for f in range(8)]
    expect_layers = [ok, ok, ok, bad_frame, ok, bad, ok, bad] + [ok] * 8
    expect = [ok, bad_frame, bad, bad, bad, too_small, ok, ok]
    good = (0, 6, 7)
    limit = smallest_output(ctx, hap, MW, MH, fmts, cap)
    want = {f: cpu_textures((MW, MH), [bottoms[f][2], insets[f][2]], placements[f], opacities[f], None, dst) for f in good}
    # what the placed call sets for the same layers: the definition of layerResults
    pics = [torch.zeros(MW * MH * 4, dtype=torch.uint8, device="cuda") for _ in range(8)]
    _r, placed_res = ctx.composite_frames_placed(frames, None, counts, sizes, pics, MW, MH, placements=placements, opacities=opacities)
    assert placed_res == expect_layers
    # ... and what the encoder makes of its pictures
    routes = [filled(cap, "cuda") for _ in range(8)]
    _r, used2, res2 = ctx.encode_frames_rgba(pics, MW, MH, MW * 4, fmts, [L.COMP_SNAPPY] * count, [2] * count, routes)
    assert all(res2[f] == 0 for f in good)
    for decode_flags in (0, hap.DECODE_BPTC_PICTURES):
        for where in ("cuda", "cpu"):
            whole = [filled(cap + 64, where) for _ in range(8)]
            outs = [o[:cap] for o in whole]
            outs[4] = None
            outs[5] = outs[5][: limit - 1]
            r, used, res, layer_res = ctx.composite_frames_encoded(frames, None, counts, sizes, MW, MH, fmts, [L.COMP_SNAPPY] * count,
                                                                   [2] * count, outs, placements=placements, opacities=opacities,
                                                                   decode_flags=decode_flags)
            assert layer_res == expect_layers and res == expect and r == bad_frame, (where, decode_flags, r, res, layer_res)
            for f in range(8):
                got = host(whole[f])
                if f in good:
                    assert (got[cap:] == SENTINEL).all(), (where, f)
                    assert used[f] == used2[f] and got[: used[f]].tobytes() == host(routes[f])[: used2[f]].tobytes(), (where, f)
                    for t in range(count):
                        rr, tex, fmt = REF.decode(got[: used[f]].tobytes(), t, out_bytes=sizes_out[t])
                        assert (rr, fmt) == (0, fmts[t]) and tex == want[f][t], (where, f, t)
                else:
                    assert used[f] == 0 and (got == SENTINEL).all(), (where, f)
    # ... and an output of exactly the smallest size is taken
    outs = [filled(limit, "cuda")]
    r, used, res, layer_res = ctx.composite_frames_encoded(frames[:1], None, counts, sizes, MW, MH, fmts, [L.COMP_SNAPPY] * count,
                                                           [2] * count, outs, placements=placements[:1], opacities=opacities[:1])
    assert (r, res, layer_res) == (0, [0], [0, 0]) and 0 < used[0] <= limit


# --------------------------------------------------------------------------------------------------------- 5. slicing --
def test_more_output_frames_than_one_slice_holds(ctx, hap):
    """A call works through its output frames a slice at a time -- 32768 textures of the second stage, so 16384 output
    frames of two layers; outputs, their sizes, placements and opacities are the call's, not the slice's.  16384 + 40
    output frames of 8 x 4 texels, two Hap Alpha layers cycling through 5 frames of random blocks, 3 opacities and 7
    output sizes: 16384 is 4 modulo 5, 1 modulo 3 and 4 modulo 7, so anything looked up by an output frame's place in
    its slice is another frame's."""
    w, h, fmts = 8, 4, [L.FMT_DXT1]
    n = 16384 + 40
    made = []
    for i in range(5):
        r, frame = hap.HapEncode([np.random.default_rng(70 + i).integers(0, 256, 32, dtype=np.uint8).tobytes()], [L.FMT_DXT5],
                                 [L.COMP_SNAPPY], [1])
        assert r == 0
        made.append(frame)
    lens5 = [len(f) for f in made]
    fades = (64, 128, 255)
    room = (True, False, True, True, False, False, True)
    cap = hap.HapMaxEncodedLength(texture_bytes(w, h, fmts), fmts, [1])
    sizes = [(w, h), (w, h)]

    def layers_of(f):
        return f % 5, (f + 2) % 5

    def placement_of(f):
        return [KP.whole((w, h)), (0, 0, 4, 4, 4 * (f % 3 == 1), 0)]

    # what a call of the first fifteen makes of each combination, with room and with none
    small = filled(15 * cap, "cuda").reshape(15, cap)
    first = [[made[a] for a in layers_of(f)] for f in range(15)]
    r, used15, res15, lres15 = ctx.composite_frames_encoded(first, None, None, sizes, w, h, fmts, [L.COMP_SNAPPY], [1], list(small),
                                                            placements=[placement_of(f) for f in range(15)],
                                                            opacities=[[255, fades[f % 3]] for f in range(15)])
    assert r == 0 and res15 == [0] * 15 and lres15 == [0] * 30
    small = host(small)
    want = [small[i, : used15[i]].tobytes() for i in range(15)]
    assert len(set(want)) > 5 and all((small[i, used15[i]:] == SENTINEL).all() for i in range(15))
    # (the first of them against the CPU definition)
    pictures = [cpu_picture("dxt5", REF.decode(made[a], 0, out_bytes=32)[1], None, w, h) for a in layers_of(0)]
    assert REF.decode(want[0], 0, out_bytes=16)[1] == cpu_textures((w, h), pictures, placement_of(0), [255, fades[0]], None, "dxt1")[0]
    none = filled(15 * cap, "cuda").reshape(15, cap)
    _r, none_used, none_res, _l = ctx.composite_frames_encoded(first, None, None, sizes, w, h, fmts, [L.COMP_SNAPPY], [1],
                                                               [row[:0] for row in none],
                                                               placements=[placement_of(f) for f in range(15)],
                                                               opacities=[[255, fades[f % 3]] for f in range(15)])
    assert all(code != 0 for code in none_res) and none_used == [0] * 15 and (host(none) == SENTINEL).all()
    # the layers' frames in device memory, behind each other at 256-byte steps
    step = 256
    assert max(lens5) <= step
    store = np.zeros(5 * step, dtype=np.uint8)
    for i, f in enumerate(made):
        store[i * step: i * step + len(f)] = np.frombuffer(f, np.uint8)
    store = torch.from_numpy(store).cuda()
    slots = [store[i * step: (i + 1) * step] for i in range(5)]
    frames = [[slots[a] for a in layers_of(f)] for f in range(n)]
    frame_bytes = [[lens5[a] for a in layers_of(f)] for f in range(n)]
    out = filled(n * cap, "cuda").reshape(n, cap)
    outputs = [out[f] if room[f % 7] else out[f, :0] for f in range(n)]
    r, used, res, layer_res = ctx.composite_frames_encoded(frames, frame_bytes, None, sizes, w, h, fmts, [L.COMP_SNAPPY], [1], outputs,
                                                           placements=[placement_of(f) for f in range(n)],
                                                           opacities=[[255, fades[f % 3]] for f in range(n)])
    got = host(out)
    f = np.arange(n)
    has_room = np.array(room)[f % 7]
    assert r == none_res[int(np.argmin(has_room)) % 15]              # (the first frame that fails)
    assert layer_res == [0] * (2 * n)
    assert res == [0 if has_room[i] else none_res[i % 15] for i in range(n)]
    assert used == [used15[i % 15] if has_room[i] else 0 for i in range(n)]
    expect = np.full((15, cap), SENTINEL, dtype=np.uint8)
    for i in range(15):
        expect[i, : used15[i]] = np.frombuffer(want[i], np.uint8)
    wrong = np.argwhere((got != np.where(has_room[:, None], expect[f % 15], SENTINEL)).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()

"""Layers of sizes of their own, placed and clipped on a canvas, composited to one RGBA8 picture per output frame on the GPU
(HapGpuCompositeTexturesPlaced, HapGpuCompositeFramesPlaced).  The definition is exact integer arithmetic: the expected
bytes are tests/_composite_placed.py's composite_placed() of what decompress_rgba / decode_frames_rgba return for each
layer -- the code under test never supplies them -- and every comparison is by equality.  Pictures lie in sentinel-filled
buffers, and every byte outside the picture must stay sentinel."""
import functools
import itertools

import numpy as np
import pytest

import _composite as K
import _composite_placed as KP
import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
OPAQUE = ("dxt1", "ycocg")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
SENTINEL = K.SENTINEL
FAR = KP.DST_MAX


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


def dev_canvas(w, h, row_bytes=None):
    """A device picture of h rows row_bytes apart (+ 64 bytes behind the last), all sentinel"""
    row_bytes = row_bytes or w * 4
    t = torch.full((h * row_bytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def host_canvas(w, h, row_bytes=None):
    row_bytes = row_bytes or w * 4
    return np.full(h * row_bytes + 64, SENTINEL, dtype=np.uint8)


def rows_of(canvas, w, h, row_bytes=None):
    """(the picture as [h, w, 4], everything else of the buffer) of a canvas the call has written"""
    row_bytes = row_bytes or w * 4
    raw = canvas.cpu().numpy() if hasattr(canvas, "cpu") else canvas
    body = raw[: h * row_bytes].reshape(h, row_bytes)
    rest = np.concatenate([body[:, w * 4:].reshape(-1), raw[h * row_bytes:]])
    return body[:, : w * 4].reshape(h, w, 4), rest


@functools.lru_cache(maxsize=None)
def random_layer(ctx, hap, case, w, h, slot=0):
    """Seeded random bytes: any 8 / 16 bytes are a block, so every decode mode occurs.  The texture (and plane) as they
    are and as one Hap frame, and what the decoders make of them; made once.
    (texture, plane | None, frame, texture count of the frame, decoded [h, w, 4])"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([31, CASES.index(case), w, h, slot])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    r, out = ctx.decompress_rgba(tex, FORMATS[case], w, h, alpha=plane)
    assert r == 0
    decoded = np.frombuffer(out, dtype=np.uint8).reshape(h, w, 4).copy()
    decoded.setflags(write=False)
    if plane is None:
        r, frame = hap.HapEncode([tex], [FORMATS[case]], [1], [1])
    else:
        r, frame = hap.HapEncode([tex, plane], [L.FMT_YCOCG, L.FMT_RGTC1], [1, 1], [1, 1])
    assert r == 0
    count = 2 if plane is not None else 1
    # the frame road gives the texture road's picture: one reference for both forms
    again = np.zeros(h * w * 4, dtype=np.uint8)
    _r, res = ctx.decode_frames_rgba([frame], [len(frame)], count, [again], w, h)
    assert res == [0] and np.array_equal(again.reshape(h, w, 4), decoded)
    return tex, plane, frame, count, decoded


@functools.lru_cache(maxsize=None)
def device_layer(ctx, hap, case, w, h, slot=0):
    tex, plane, _frame, _count, _decoded = random_layer(ctx, hap, case, w, h, slot)
    return dev(tex), FORMATS[case], dev(plane)


def placed(ctx, layers, sizes, canvas_size, placements, opacities, background, on_device, row_bytes=None):
    """composite_textures_placed into a sentinel-filled host or device picture: the [h, w, 4] picture"""
    w, h = canvas_size
    canvas = dev_canvas(w, h, row_bytes) if on_device else host_canvas(w, h, row_bytes)
    r, out = ctx.composite_textures_placed(layers, sizes, w, h, placements=placements, opacities=opacities,
                                           background=background, rgba=canvas, row_bytes=row_bytes)
    assert r == 0 and out is None
    picture, rest = rows_of(canvas, w, h, row_bytes)
    assert (rest == SENTINEL).all()
    return picture


def edge_placements(canvas_size, layer_size):
    """(name, placement) of one rectangle of the layer -- from the layer's far corner, at most half the canvas a side and
    two blocks at least where the layer has them -- inside, flush with each edge, clipped by a block at each edge and
    corner, and wholly outside on each side: just touching, a block away, and as far as a call may say"""
    W, H = canvas_size
    lw, lh = layer_size
    rw = min(lw, max(8, W // 2 // 4 * 4))
    rh = min(lh, max(8, H // 2 // 4 * 4))
    sx, sy = lw - rw, lh - rh
    mx, my = (W - rw) // 2 // 4 * 4, (H - rh) // 2 // 4 * 4
    right, bottom = W - rw, H - rh
    at = {"inside": (mx, my), "flush left": (0, my), "flush right": (right, my), "flush top": (mx, 0), "flush bottom": (mx, bottom),
          "clipped left": (-4, my), "clipped right": (right + 4, my), "clipped top": (mx, -4), "clipped bottom": (mx, bottom + 4),
          "clipped top left": (-4, -4), "clipped top right": (right + 4, -4), "clipped bottom left": (-4, bottom + 4),
          "clipped bottom right": (right + 4, bottom + 4),
          "touching right": (W, my), "beyond right": (W + 4, my), "touching left": (-rw, my), "beyond left": (-rw - 4, my),
          "touching bottom": (mx, H), "beyond bottom": (mx, H + 4), "touching top": (mx, -rh), "beyond top": (mx, -rh - 4),
          "far right and down": (FAR, FAR), "far left and up": (-FAR, -FAR)}
    return [(name, (sx, sy, rw, rh, dx, dy)) for name, (dx, dy) in at.items()]


# ------------------------------------------------------------------------------------- 1. one layer at every edge --
# every canvas with two layers: one that fits it and one that does not
PAIRS = (((4, 4), (4, 4)), ((4, 4), (16, 16)), ((64, 32), (16, 16)), ((64, 32), (128, 64)), ((64, 32), (64, 32)),
         ((260, 8), (260, 8)), ((260, 8), (8, 68)), ((68, 64), (16, 16)), ((68, 64), (8, 68)), ((68, 64), (128, 64)))


def test_the_pairs_use_every_canvas_and_every_layer():
    assert {c for c, _l in PAIRS} == set(KP.CANVASES) and {l for _c, l in PAIRS} == set(KP.LAYERS)
    for canvas_size, layer_size in PAIRS:
        names = [n for n, _p in edge_placements(canvas_size, layer_size)]
        assert len(names) == 23
        for _name, p in edge_placements(canvas_size, layer_size):
            assert KP.valid(p, layer_size), (canvas_size, layer_size, p)
        shown = {n: KP.visible(p, canvas_size) for n, p in edge_placements(canvas_size, layer_size)}
        assert all(shown[n] is None for n in shown if n.startswith(("touching", "beyond", "far")))
        assert all(shown[n] is not None for n in shown if n.startswith(("inside", "flush")))


@pytest.mark.parametrize("canvas_size,layer_size", PAIRS, ids=lambda s: "%dx%d" % s)
def test_one_layer_at_every_edge(ctx, hap, canvas_size, layer_size):
    lw, lh = layer_size
    turn = 0
    for case in CASES:
        layer = device_layer(ctx, hap, case, lw, lh)
        decoded = random_layer(ctx, hap, case, lw, lh)[4]
        for name, placement in edge_placements(canvas_size, layer_size):
            for background in K.BACKGROUNDS:
                for opacity in (255, 128, 0):
                    want = KP.composite_placed(canvas_size, [decoded], [placement], [opacity], background)
                    turn += 1
                    got = placed(ctx, [layer], [layer_size], canvas_size, [placement], [opacity], background, turn % 2 == 0)
                    assert np.array_equal(got, want), (case, name, placement, background, opacity)
                    box = KP.visible(placement, canvas_size)
                    if opacity == 255 and case in OPAQUE:
                        # the masked replace: the rectangle is the decoder's bytes, everything else the background
                        outside = np.ones(got.shape[:2], dtype=bool)
                        if box:
                            x0, y0, x1, y1 = box
                            outside[y0:y1, x0:x1] = False
                            sx, sy, _w, _h, dx, dy = placement
                            assert np.array_equal(got[y0:y1, x0:x1], decoded[sy + y0 - dy: sy + y1 - dy, sx + x0 - dx: sx + x1 - dx])
                        assert (got[outside] == np.asarray(background, dtype=np.uint8)).all(), (case, name, background)
                    if box is None or opacity == 0:
                        assert (got == np.asarray(background, dtype=np.uint8)).all(), (case, name, background, opacity)


# -------------------------------------------------------------------- 2. a window of a layer larger than the canvas --
@pytest.mark.parametrize("canvas_size,layer_size,rect", (((64, 32), (128, 64), (32, 16, 64, 32)), ((4, 4), (16, 16), (8, 4, 4, 4)),
                                                         ((260, 8), (8, 68), (0, 28, 8, 8))),
                         ids=("64x32_of_128x64", "4x4_of_16x16", "260x8_of_8x68"))
def test_a_centred_window_is_the_crop(ctx, hap, canvas_size, layer_size, rect):
    W, H = canvas_size
    lw, lh = layer_size
    x, y, w, h = rect
    dx, dy = (W - w) // 2 // 4 * 4, (H - h) // 2 // 4 * 4
    for case in CASES:
        _tex, _plane, frame, count, decoded = random_layer(ctx, hap, case, lw, lh)
        crop = decoded[y: y + h, x: x + w]
        for background in K.BACKGROUNDS:
            for opacity in (255, 200):
                want = KP.composite_placed(canvas_size, [decoded], [(x, y, w, h, dx, dy)], [opacity], background)
                pictures = [dev_canvas(W, H)]
                r, res = ctx.composite_frames_placed([[frame]], None, [count], [layer_size], pictures, W, H,
                                                     placements=[[(x, y, w, h, dx, dy)]], opacities=[[opacity]], background=background)
                assert r == 0 and res == [0]
                got, rest = rows_of(pictures[0], W, H)
                assert (rest == SENTINEL).all() and np.array_equal(got, want), (case, background, opacity)
                if case in OPAQUE and opacity == 255:
                    assert np.array_equal(got[dy: dy + h, dx: dx + w], crop)
        if case in OPAQUE:
            # ... and the rectangle decoder's picture byte for byte
            region = np.zeros(h * w * 4, dtype=np.uint8)
            r, res = ctx.decode_frames_rgba_region([frame], [len(frame)], count, [region], lw, lh, rect)
            assert r == 0 and res == [0]
            r, out = ctx.composite_textures_placed([device_layer(ctx, hap, case, lw, lh)], [layer_size], w, h, placements=[(x, y, w, h, 0, 0)])
            assert r == 0 and out == region.tobytes()


# ------------------------------------------------------------------------------------ 3. three layers overlapping --
STACK = (("dxt5", (16, 16)), ("ycocg_alpha", (128, 64)), ("ycocg", (8, 68)))


def random_placement(rng, canvas_size, layer_size, focus=None):
    """a block-aligned rectangle of the layer: anywhere from just outside the canvas on one side to just outside on the
    other, or (more often than not) somewhere over the canvas block `focus`, so that layers meet"""
    W, H = canvas_size
    lw, lh = layer_size
    w = 4 * int(rng.integers(1, lw // 4 + 1))
    h = 4 * int(rng.integers(1, lh // 4 + 1))
    sx = 4 * int(rng.integers(0, (lw - w) // 4 + 1))
    sy = 4 * int(rng.integers(0, (lh - h) // 4 + 1))
    if focus is not None and rng.random() < 0.6:
        dx = 4 * (focus[0] - int(rng.integers(0, w // 4)))
        dy = 4 * (focus[1] - int(rng.integers(0, h // 4)))
    else:
        dx = 4 * int(rng.integers(-(w // 4), W // 4 + 1))
        dy = 4 * int(rng.integers(-(h // 4), H // 4 + 1))
        if focus is None and rng.random() < 0.5:
            dx = W if rng.random() < 0.5 else -w        # (just touching the canvas: outside)
    return (sx, sy, w, h, dx, dy)


def draws(canvas_size):
    rng = np.random.default_rng([33, canvas_size[0], canvas_size[1]])
    out = []
    for i in range(32):
        # (every fourth draw without a focus: layers that miss each other, and the canvas)
        focus = (int(rng.integers(0, canvas_size[0] // 4)), int(rng.integers(0, canvas_size[1] // 4))) if i % 4 else None
        placements = [random_placement(rng, canvas_size, size, focus) for _case, size in STACK]
        opacities = [int(o) for o in rng.choice(K.OPACITIES[1:], len(STACK))]
        out.append((placements, opacities))
    return out


def cover_counts(canvas_size, placements):
    """per canvas block, how many of the placements cover it"""
    W, H = canvas_size
    count = np.zeros((H // 4, W // 4), dtype=int)
    for p in placements:
        box = KP.visible(p, canvas_size)
        if box:
            count[box[1] // 4: box[3] // 4, box[0] // 4: box[2] // 4] += 1
    return count


@pytest.mark.parametrize("canvas_size", KP.CANVASES, ids=lambda s: "%dx%d" % s)
def test_three_layers_overlapping_partly(ctx, hap, canvas_size):
    sizes = [size for _case, size in STACK]
    layers = [device_layer(ctx, hap, case, *size) for case, size in STACK]
    hosts = [(random_layer(ctx, hap, case, *size)[0], FORMATS[case], random_layer(ctx, hap, case, *size)[1]) for case, size in STACK]
    decoded = [random_layer(ctx, hap, case, *size)[4] for case, size in STACK]
    seen = set()
    for i, (placements, opacities) in enumerate(draws(canvas_size)):
        seen.update(cover_counts(canvas_size, placements).ravel().tolist())
        background = K.BACKGROUNDS[i % len(K.BACKGROUNDS)]
        want = KP.composite_placed(canvas_size, decoded, placements, opacities, background)
        got = placed(ctx, hosts if i % 4 == 3 else layers, sizes, canvas_size, placements, opacities, background, i % 2 == 0)
        assert np.array_equal(got, want), (i, placements, opacities, background)
    # canvas blocks under none, one, two and all three of the layers
    assert seen == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------------ 4. identity --
def test_whole_layers_of_the_canvas_size_are_composite_frames(ctx, hap):
    W, H = 68, 64
    for i, (bottom, top) in enumerate(itertools.product(CASES, CASES)):
        made = [random_layer(ctx, hap, bottom, W, H, 0), random_layer(ctx, hap, top, W, H, 1)]
        frames = [[m[2] for m in made]]
        counts = [m[3] for m in made]
        opacities = [[K.OPACITIES[1:][i % 5], K.OPACITIES[1:][(i // 4 + 2) % 5]]]
        background = K.BACKGROUNDS[i % 4]
        plain, here = [dev_canvas(W, H)], [dev_canvas(W, H)]
        r, res = ctx.composite_frames(frames, None, counts, plain, W, H, opacities=opacities, background=background)
        assert r == 0 and res == [0, 0]
        r, res = ctx.composite_frames_placed(frames, None, counts, [(W, H)] * 2, here, W, H, placements=None, opacities=opacities,
                                             background=background)
        assert r == 0 and res == [0, 0]
        assert torch.equal(plain[0], here[0]), (bottom, top)
        picture, rest = rows_of(here[0], W, H)
        assert (rest == SENTINEL).all()
        assert np.array_equal(picture, K.composite([m[4] for m in made], opacities[0], background)), (bottom, top)
        # the textures form, and the default written out
        layers = [(m[0], FORMATS[case], m[1]) for m, case in zip(made, (bottom, top))]
        for placements in (None, [KP.whole((W, H))] * 2):
            assert np.array_equal(placed(ctx, layers, [(W, H)] * 2, (W, H), placements, opacities[0], background, True), picture)


# -------------------------------------------------------------------------------------------------------- 5. mosaic --
def test_four_tiles_side_by_side(ctx, hap):
    W, H, tw, th = 64, 32, 32, 16
    cases = ("dxt1", "ycocg", "ycocg", "dxt1")
    decoded = [random_layer(ctx, hap, case, tw, th, slot)[4] for slot, case in enumerate(cases)]
    layers = [device_layer(ctx, hap, case, tw, th, slot) for slot, case in enumerate(cases)]
    placements = [(0, 0, tw, th, tw * (i % 2), th * (i // 2)) for i in range(4)]
    want = np.concatenate([np.concatenate(decoded[:2], axis=1), np.concatenate(decoded[2:], axis=1)], axis=0)
    assert want.shape == (H, W, 4)
    assert np.array_equal(want, KP.composite_placed((W, H), decoded, placements, None, K.BACKGROUNDS[3]))
    for on_device in (False, True):
        assert np.array_equal(placed(ctx, layers, [(tw, th)] * 4, (W, H), placements, None, K.BACKGROUNDS[3], on_device), want)
    # tiles with an alpha of their own let the background through, by the definition
    cases = CASES
    decoded = [random_layer(ctx, hap, case, tw, th, 4 + slot)[4] for slot, case in enumerate(cases)]
    layers = [device_layer(ctx, hap, case, tw, th, 4 + slot) for slot, case in enumerate(cases)]
    want = KP.composite_placed((W, H), decoded, placements, [255, 254, 128, 200], K.BACKGROUNDS[2])
    assert np.array_equal(placed(ctx, layers, [(tw, th)] * 4, (W, H), placements, [255, 254, 128, 200], K.BACKGROUNDS[2], True), want)


# -------------------------------------------------------------------------------------------------------- 6. frames --
W, H = 68, 64
FRAMES, LAYERS = 3, 3
COUNTS = (1, 2, 1)
SIZES = ((16, 16), (128, 64), (8, 68))
# placements that move from output frame to output frame: an inset sliding in from the left, a window panning over a
# large clip, a strip taller than the canvas scrolling up
MOVES = [[(0, 0, 16, 16, -8, 4), (0, 0, 68, 64, 0, 0), (0, 0, 8, 68, 60, 0)],
         [(0, 0, 16, 16, 24, 24), (32, 0, 64, 64, 4, 0), (0, 4, 8, 64, 60, 0)],
         [(4, 4, 12, 12, 56, 52), (60, 0, 68, 32, 0, 16), (0, 0, 8, 68, 64, -4)]]
FADES = [[255, 255, 200], [128, 254, 255], [255, 127, 1]]


@pytest.fixture(scope="module")
def movie(ctx, hap):
    """3 output frames x 3 layers of sizes of their own, textureCounts (1, 2, 1): (frames[f][l], decoded[f][l]).  Layer 0 is
    Hap, Hap Alpha, Hap Q; layer 1 Hap Q Alpha; layer 2 Hap Q, Hap, and a Hap Q Alpha frame read with 1."""
    kinds = [("dxt1", "ycocg_alpha", "ycocg"), ("dxt5", "ycocg_alpha", "dxt1"), ("ycocg", "ycocg_alpha", "ycocg_alpha")]
    frames, decoded = [], []
    for f in range(FRAMES):
        made = [random_layer(ctx, hap, kinds[f][l], SIZES[l][0], SIZES[l][1], 10 + f) for l in range(LAYERS)]
        frames.append([m[2] for m in made])
        pictures = [m[4] for m in made]
        if kinds[f][2] == "ycocg_alpha":        # (read with 1: its colour texture alone)
            out = np.zeros(SIZES[2][0] * SIZES[2][1] * 4, dtype=np.uint8)
            _r, res = ctx.decode_frames_rgba([frames[f][2]], [len(frames[f][2])], 1, [out], SIZES[2][0], SIZES[2][1])
            assert res == [0]
            pictures[2] = out.reshape(SIZES[2][1], SIZES[2][0], 4)
            assert (pictures[2][:, :, 3] == 255).all()
        decoded.append(pictures)
    for f in range(FRAMES):
        for l in range(LAYERS):
            assert KP.valid(MOVES[f][l], SIZES[l])
    return frames, decoded


def canvases(kinds, row_bytes=None):
    return [dev_canvas(W, H, row_bytes) if k == "device" else host_canvas(W, H, row_bytes) if k == "host" else None for k in kinds]


def check_frames(pictures, decoded, placements, opacities, background, written, row_bytes=None):
    for f in range(FRAMES):
        if pictures[f] is None:
            continue
        picture, rest = rows_of(pictures[f], W, H, row_bytes)
        assert (rest == SENTINEL).all(), f
        if written[f]:
            want = KP.composite_placed((W, H), decoded[f], placements[f] if placements else None,
                                       opacities[f] if opacities else None, background)
            assert np.array_equal(picture, want), f
        else:
            assert (picture == SENTINEL).all(), f


@pytest.mark.parametrize("where", ("host", "device"))
def test_frames(ctx, movie, where):
    frames, decoded = movie
    given = frames if where == "host" else [[dev(b) for b in fr] for fr in frames]
    lens = [[len(b) for b in fr] for fr in frames]
    for kinds, background in ((("device", "host", "device"), K.BACKGROUNDS[3]), (("host", "device", "host"), None)):
        pictures = canvases(kinds)
        r, res = ctx.composite_frames_placed(given, lens, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES,
                                             background=background)
        assert r == 0 and res == [0] * (FRAMES * LAYERS)
        check_frames(pictures, decoded, MOVES, FADES, background, [True] * FRAMES)
    # rows longer than the picture
    row_bytes = W * 4 + 48
    pictures = canvases(("device", "host", "device"), row_bytes)
    r, res = ctx.composite_frames_placed(given, lens, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES,
                                         background=K.BACKGROUNDS[1], row_bytes=row_bytes)
    assert r == 0 and res == [0] * (FRAMES * LAYERS)
    check_frames(pictures, decoded, MOVES, FADES, K.BACKGROUNDS[1], [True] * FRAMES, row_bytes)
    # the defaults: every layer whole at (0, 0), clipped to the canvas; all 255
    pictures = canvases(("device",) * FRAMES)
    r, res = ctx.composite_frames_placed(given, lens, COUNTS, SIZES, pictures, W, H)
    assert r == 0 and res == [0] * (FRAMES * LAYERS)
    check_frames(pictures, decoded, None, None, None, [True] * FRAMES)


def test_frames_one_launch_per_slice(ctx, movie):
    frames, _decoded = movie
    pictures = canvases(("device",) * FRAMES)
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.composite_frames_placed(frames, None, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 1, prof["block_decode"]


@pytest.mark.parametrize("kinds", (("device",) * 3, ("host",) * 3), ids=("device", "host"))
def test_failures_stay_local(ctx, hap, movie, kinds):
    frames, decoded = movie
    bad = hap.HapResult.Bad_Arguments
    # one frame's texture of another size than its layer's: a 16 x 16 frame where the layer is 8 x 68, and (more blocks
    # than the layer has) a 128 x 64 one where it is 16 x 16
    # than the layer has) a 128 x 64 one where it is 16 x 16, and a 16 x 16 Hap Q Alpha one where it is 128 x 64
    for at, wrong in (((1, 2), random_layer(ctx, hap, "dxt1", 16, 16, 10)[2]), ((1, 0), random_layer(ctx, hap, "ycocg", 128, 64, 0)[2]),
                      ((1, 1), random_layer(ctx, hap, "ycocg_alpha", 16, 16, 0)[2])):
        other = [list(fr) for fr in frames]
        other[at[0]][at[1]] = wrong
        pictures = canvases(kinds)
        r, res = ctx.composite_frames_placed(other, None, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES,
                                             background=K.BACKGROUNDS[2])
        want = [0] * (FRAMES * LAYERS)
        want[at[0] * LAYERS + at[1]] = bad
        assert r == bad and res == want, (at, r, res)
        check_frames(pictures, decoded, MOVES, FADES, K.BACKGROUNDS[2], [True, False, True])
    # one output picture NULL: every entry of that output frame
    pictures = canvases((kinds[0], None, kinds[2]))
    r, res = ctx.composite_frames_placed(frames, None, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES)
    assert r == bad and res == [0, 0, 0, bad, bad, bad, 0, 0, 0]
    check_frames(pictures, decoded, MOVES, FADES, None, [True, False, True])


def test_a_placement_out_of_order_refuses_the_whole_call(ctx, hap, movie):
    frames, _decoded = movie
    bad = hap.HapResult.Bad_Arguments
    for wrong in ((0, 0, 8, 72, 60, 0), (0, 0, 8, 68, 62, 0), (0, 0, 8, 0, 60, 0), (0, 0, 8, 68, KP.DST_MAX + 4, 0)):
        moves = [list(fr) for fr in MOVES]
        moves[2][2] = wrong
        pictures = canvases(("device", "host", "device"))
        r, res = ctx.composite_frames_placed(frames, None, COUNTS, SIZES, pictures, W, H, placements=moves, opacities=FADES)
        assert r == bad and res == [bad] * (FRAMES * LAYERS), wrong
        for p in pictures:
            raw = p.cpu().numpy() if hasattr(p, "cpu") else p
            assert (raw == SENTINEL).all(), wrong


def test_the_same_call_twice_gives_the_same_bytes(ctx, movie):
    frames, _decoded = movie
    first, second = canvases(("device",) * FRAMES), canvases(("device",) * FRAMES)
    for pictures in (first, second):
        r, res = ctx.composite_frames_placed(frames, None, COUNTS, SIZES, pictures, W, H, placements=MOVES, opacities=FADES,
                                             background=K.BACKGROUNDS[3])
        assert r == 0 and res == [0] * (FRAMES * LAYERS)
    for a, b in zip(first, second):
        assert torch.equal(a, b)

"""Layers of textures and of Hap frames composited to one RGBA8 picture per output frame on the GPU
(HapGpuCompositeTextures, HapGpuCompositeFrames).  The definition is exact integer arithmetic: the expected bytes are
tests/_composite.py's composite() of what decompress_rgba / decode_frames_rgba return for each layer -- the code under
test never supplies them -- and every comparison is by equality."""
import functools
import itertools

import numpy as np
import pytest

import _composite as K
import _data as D
import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = ("dxt1", "dxt5", "ycocg", "ycocg_alpha")
FORMATS = {"dxt1": L.FMT_DXT1, "dxt5": L.FMT_DXT5, "ycocg": L.FMT_YCOCG, "ycocg_alpha": L.FMT_YCOCG}
PAIRS = tuple(itertools.product(CASES, CASES))         # every ordered pair (bottom, top)
SENTINEL = K.SENTINEL


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
def random_texture(ctx, case, w, h, slot=0):
    """Seeded random bytes: any 8 / 16 bytes are a block, so every decode mode occurs.  (texture, plane | None, what
    decompress_rgba makes of them); made once.  slot: a second, third ... texture of the same case"""
    nb = (w // 4) * (h // 4)
    rng = np.random.default_rng([21, CASES.index(case), w, h, slot])
    tex = rng.integers(0, 256, nb * D.BLOCK_BYTES[FORMATS[case]], dtype=np.uint8).tobytes()
    plane = rng.integers(0, 256, nb * 8, dtype=np.uint8).tobytes() if case == "ycocg_alpha" else None
    r, out = ctx.decompress_rgba(tex, FORMATS[case], w, h, alpha=plane)
    assert r == 0
    decoded = np.frombuffer(out, dtype=np.uint8).reshape(h, w, 4).copy()
    decoded.setflags(write=False)
    return tex, plane, decoded


def stack(ctx, cases, w, h):
    """layer l a texture of cases[l]: (host layers, device layers, decoded pictures)"""
    made = [random_texture(ctx, case, w, h, slot) for slot, case in enumerate(cases)]
    host = [(tex, FORMATS[case], plane) for case, (tex, plane, _d) in zip(cases, made)]
    device = [(dev(tex), fmt, dev(plane)) for tex, fmt, plane in host]
    return host, device, [d for _t, _p, d in made]


def composited(ctx, layers, w, h, opacities, background, on_device):
    """composite_textures into a host or a device picture: the [h, w, 4] picture"""
    if not on_device:
        r, out = ctx.composite_textures(layers, w, h, opacities=opacities, background=background)
        assert r == 0
        return np.frombuffer(out, dtype=np.uint8).reshape(h, w, 4)
    canvas = dev_canvas(w, h)
    r, out = ctx.composite_textures(layers, w, h, opacities=opacities, background=background, rgba=canvas)
    assert r == 0 and out is None
    picture, rest = rows_of(canvas, w, h)
    assert (rest == SENTINEL).all()
    return picture


# ---------------------------------------------------------------------------------- 1. textures: every pair of cases --
@pytest.mark.parametrize("size", K.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_every_ordered_pair_at_every_edge_of_the_grid(ctx, size):
    w, h = size
    rng = np.random.default_rng([22, w, h])
    seen = set()
    for bottom, top in PAIRS:
        host, device, decoded = stack(ctx, (bottom, top), w, h)
        for background in K.BACKGROUNDS:
            opacities = [int(o) for o in rng.choice(K.OPACITIES, 2)]
            seen.update(opacities)
            want = K.composite(decoded, opacities, background)
            for layers in (host, device):                   # textures in host and in device memory
                for on_device in (False, True):             # pictures in host and in device memory
                    got = composited(ctx, layers, w, h, opacities, background, on_device)
                    assert np.array_equal(got, want), (bottom, top, opacities, background, layers is device, on_device)
    assert seen == set(K.OPACITIES)


def test_every_pair_of_opacities(ctx):
    w, h = 8, 4
    _host, device, decoded = stack(ctx, ("dxt5", "ycocg_alpha"), w, h)
    for background in K.BACKGROUNDS:
        for opacities in itertools.product(K.OPACITIES, K.OPACITIES):
            got = composited(ctx, device, w, h, list(opacities), background, True)
            assert np.array_equal(got, K.composite(decoded, opacities, background)), (opacities, background)


# ------------------------------------------------------------------------------------------------- 2. layer counts --
@pytest.mark.parametrize("count", (3, 16))
def test_stacks_of_layers(ctx, count):
    w, h = 260, 8
    # (16: the four cases four times over with differing opacities)
    cases = ("ycocg", "dxt5", "ycocg_alpha") if count == 3 else CASES * 4
    assert len(cases) == count
    host, device, decoded = stack(ctx, cases, w, h)
    for shift, background in enumerate(K.BACKGROUNDS):
        # layer i is case i % 4 for the (i // 4)-th time: a case meets a different opacity each time, and only the first
        # four layers may be opaque ones without alpha, which would replace all below them
        opacities = [K.OPACITIES[1:][(i // 4 + i % 4 + shift) % 5] for i in range(count)]
        opacities = [min(o, 254) if i >= 4 else o for i, o in enumerate(opacities)]
        want = K.composite(decoded, opacities, background)
        for layers, on_device in ((host, True), (device, False)):
            assert np.array_equal(composited(ctx, layers, w, h, opacities, background, on_device), want), (background, opacities)
    # every layer matters: leaving any one out changes the picture
    opacities = [200] * count
    whole = K.composite(decoded, opacities, K.BACKGROUNDS[3])
    assert np.array_equal(composited(ctx, device, w, h, opacities, K.BACKGROUNDS[3], True), whole)
    for l in range(count):
        assert not np.array_equal(K.composite(decoded[:l] + decoded[l + 1:], opacities[1:], K.BACKGROUNDS[3]), whole), l


def test_more_layers_than_the_maximum_are_refused(ctx, hap):
    w, h = 8, 4
    host, _device, _decoded = stack(ctx, ("dxt1",), w, h)
    canvas = host_canvas(w, h)
    r, _out = ctx.composite_textures(host * 17, w, h, rgba=canvas)
    assert r == hap.HapResult.Bad_Arguments and (canvas == SENTINEL).all()
    r, _out = ctx.composite_textures([(host[0][0], L.FMT_BC7, None)], w, h, rgba=canvas)
    assert r == hap.HapResult.Bad_Arguments and (canvas == SENTINEL).all()
    r, _out = ctx.composite_textures([(host[0][0][:-1], L.FMT_DXT1, None)], w, h, rgba=canvas)
    assert r == hap.HapResult.Bad_Arguments and (canvas == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------ 3. anchor --
@pytest.mark.parametrize("case", ("dxt1", "ycocg"))
def test_one_opaque_layer_is_the_decoders_picture(ctx, case):
    for w, h in K.GEOMETRIES:
        host, device, decoded = stack(ctx, (case,), w, h)
        for background in K.BACKGROUNDS:
            for layers, on_device in ((host, False), (device, True)):
                got = composited(ctx, layers, w, h, [255], background, on_device)
                assert np.array_equal(got, decoded[0]), (w, h, background)


# ---------------------------------------------------------------------------------------- 4. rows and defaults --
@pytest.mark.parametrize("on_device", (False, True), ids=("host", "device"))
def test_rows_longer_than_the_picture(ctx, on_device):
    w, h = 260, 8
    row_bytes = w * 4 + 48
    host, _device, decoded = stack(ctx, ("ycocg", "ycocg_alpha", "dxt5"), w, h)
    opacities, background = [255, 127, 254], K.BACKGROUNDS[2]
    canvas = dev_canvas(w, h, row_bytes) if on_device else host_canvas(w, h, row_bytes)
    r, _out = ctx.composite_textures(host, w, h, opacities=opacities, background=background, rgba=canvas, row_bytes=row_bytes)
    assert r == 0
    picture, rest = rows_of(canvas, w, h, row_bytes)
    assert np.array_equal(picture, K.composite(decoded, opacities, background))
    # the sentinels between the rows and behind the last row survive
    assert rest.size == h * 48 + 64 and (rest == SENTINEL).all()


def test_defaults(ctx):
    w, h = 68, 64
    host, _device, decoded = stack(ctx, ("dxt5", "ycocg_alpha"), w, h)
    plain = composited(ctx, host, w, h, None, None, False)
    assert np.array_equal(plain, composited(ctx, host, w, h, [255, 255], (0, 0, 0, 255), False))
    assert np.array_equal(plain, K.composite(decoded))
    assert np.array_equal(composited(ctx, host, w, h, None, K.BACKGROUNDS[3], True),
                          K.composite(decoded, [255, 255], K.BACKGROUNDS[3]))
    assert np.array_equal(composited(ctx, host, w, h, [1, 128], None, True), K.composite(decoded, [1, 128], (0, 0, 0, 255)))


# ------------------------------------------------------------------------------------------------------- 5. frames --
W, H = 68, 64
COUNTS = (1, 2, 1)
FRAMES, LAYERS = 3, 3


def frames_of(ctx, hap, fmts, pictures, flags=0):
    """One Hap frame per RGBA picture (textures of `fmts`), made by encode_frames_rgba: list of bytes"""
    sizes = [(W // 4) * (H // 4) * D.BLOCK_BYTES[f] for f in fmts]
    chunks = [2] * len(fmts)
    bufs = [np.zeros(hap.HapMaxEncodedLength(sizes, fmts, chunks), dtype=np.uint8) for _ in pictures]
    r, used, res = ctx.encode_frames_rgba([np.ascontiguousarray(p) for p in pictures], W, H, W * 4, fmts, [1] * len(fmts),
                                          chunks, bufs, flags=flags)
    assert r == 0 and res == [0] * len(pictures), (r, res)
    return [b[:u].tobytes() for b, u in zip(bufs, used)]


def source_picture(seed):
    """a _data.py picture with an alpha channel that is neither opaque nor flat"""
    p = D.rgba(W, H, seed).copy()
    y, x = np.mgrid[0:H, 0:W]
    p[:, :, 3] = ((x * 5 + y * 3 + seed * 37) % 256).astype(np.uint8)
    return p


def decoded_with(ctx, frame, count):
    """what decode_frames_rgba writes for the frame with that texture count: (result, [H, W, 4])"""
    out = np.zeros(H * W * 4, dtype=np.uint8)
    _r, res = ctx.decode_frames_rgba([frame], [len(frame)], count, [out], W, H)
    return res[0], out.reshape(H, W, 4)


@pytest.fixture(scope="module", params=(False, True), ids=("plain", "fragment_table"))
def movie(request, ctx, hap):
    """3 output frames x 3 layers, textureCounts (1, 2, 1): (frames[f][l], decoded[f][l]).  Layer 0 is Hap in one output
    frame, Hap Q in another, Hap Alpha in the third; layer 1 is Hap Q Alpha; layer 2 is Hap Alpha, and in one output
    frame a Hap Q Alpha frame, read with 1 as its colour texture alone."""
    flags = hap.ENCODE_FRAGMENT_INDEX if request.param else 0
    qa = [L.FMT_YCOCG, L.FMT_RGTC1]
    layer0 = [frames_of(ctx, hap, [fmt], [source_picture(i)], flags)[0]
              for i, fmt in enumerate((L.FMT_DXT1, L.FMT_YCOCG, L.FMT_DXT5))]
    layer1 = frames_of(ctx, hap, qa, [source_picture(10 + i) for i in range(FRAMES)], flags)
    layer2 = frames_of(ctx, hap, [L.FMT_DXT5], [source_picture(20 + i) for i in range(2)], flags)
    layer2.append(frames_of(ctx, hap, qa, [source_picture(22)], flags)[0])
    frames = [[layer0[f], layer1[f], layer2[f]] for f in range(FRAMES)]
    decoded = []
    for f in range(FRAMES):
        pictures = []
        for l in range(LAYERS):
            res, picture = decoded_with(ctx, frames[f][l], COUNTS[l])
            assert res == 0
            pictures.append(picture)
        decoded.append(pictures)
    # (the alpha layers are neither opaque nor flat)
    assert len(np.unique(decoded[0][1][:, :, 3])) > 8 and len(np.unique(decoded[0][2][:, :, 3])) > 8
    assert (decoded[2][2][:, :, 3] == 255).all()
    return frames, decoded


DISSOLVE = [[255, 255, 0], [255, 128, 127], [254, 1, 255]]       # per output frame, as in a dissolve


def canvases(kinds):
    return [dev_canvas(W, H) if k == "device" else host_canvas(W, H) if k == "host" else None for k in kinds]


def check_frames(pictures, decoded, opacities, background, written):
    for f in range(FRAMES):
        if pictures[f] is None:
            continue
        picture, rest = rows_of(pictures[f], W, H)
        assert (rest == SENTINEL).all(), f
        if written[f]:
            assert np.array_equal(picture, K.composite(decoded[f], opacities[f] if opacities else None, background)), f
        else:
            assert (picture == SENTINEL).all(), f


def test_frames(ctx, movie):
    frames, decoded = movie
    for kinds, background in ((("device", "host", "device"), K.BACKGROUNDS[3]), (("host", "device", "host"), None)):
        pictures = canvases(kinds)
        r, res = ctx.composite_frames(frames, None, COUNTS, pictures, W, H, opacities=DISSOLVE, background=background)
        assert r == 0 and res == [0] * (FRAMES * LAYERS)
        check_frames(pictures, decoded, DISSOLVE, background, [True] * FRAMES)
    # the defaults: opacities None is all 255
    pictures = canvases(("device",) * FRAMES)
    r, res = ctx.composite_frames(frames, [[len(b) for b in fr] for fr in frames], COUNTS, pictures, W, H)
    assert r == 0 and res == [0] * (FRAMES * LAYERS)
    check_frames(pictures, decoded, None, None, [True] * FRAMES)


def test_frames_one_launch_per_slice(ctx, movie):
    frames, _decoded = movie
    pictures = canvases(("device",) * FRAMES)
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.composite_frames(frames, None, COUNTS, pictures, W, H, opacities=DISSOLVE)
    prof = ctx.collect_profile()
    ctx.set_profiling(False)
    assert prof["block_decode"][0] == 1, prof["block_decode"]


def test_frames_with_longer_rows(ctx, movie):
    frames, decoded = movie
    row_bytes = W * 4 + 48
    pictures = [dev_canvas(W, H, row_bytes), host_canvas(W, H, row_bytes), dev_canvas(W, H, row_bytes)]
    r, res = ctx.composite_frames(frames, None, COUNTS, pictures, W, H, opacities=DISSOLVE, background=K.BACKGROUNDS[1],
                                  row_bytes=row_bytes)
    assert r == 0 and res == [0] * (FRAMES * LAYERS)
    for f in range(FRAMES):
        picture, rest = rows_of(pictures[f], W, H, row_bytes)
        assert np.array_equal(picture, K.composite(decoded[f], DISSOLVE[f], K.BACKGROUNDS[1])), f
        assert (rest == SENTINEL).all(), f


# ------------------------------------------------------------------------------------------- 6. failures stay local --
@pytest.mark.parametrize("kinds", (("device",) * 3, ("host",) * 3), ids=("device", "host"))
def test_failures_stay_local(ctx, hap, movie, kinds):
    frames, decoded = movie
    bad = hap.HapResult.Bad_Arguments
    opacities = [[200, 255, 100]] * FRAMES
    # one layer's frame truncated: HapDecode's code for it, whatever that is for this frame
    cut = [list(fr) for fr in frames]
    cut[1][2] = cut[1][2][:-3]
    code, _p = decoded_with(ctx, cut[1][2], 1)
    assert code not in (0, bad)
    pictures = canvases(kinds)
    r, res = ctx.composite_frames(cut, None, COUNTS, pictures, W, H, opacities=opacities, background=K.BACKGROUNDS[2])
    assert r == code and res == [0, 0, 0, 0, 0, code, 0, 0, 0]
    check_frames(pictures, decoded, opacities, K.BACKGROUNDS[2], [True, False, True])
    # one layer's frame of another geometry, and one of a flavour its layer's count does not take
    other = [list(fr) for fr in frames]
    small = np.zeros(hap.HapMaxEncodedLength([(W // 4) * (H // 4 - 1) * 16], [L.FMT_DXT5], [1]), dtype=np.uint8)
    r, used, res = ctx.encode_frames_rgba([np.ascontiguousarray(source_picture(30)[: H - 4])], W, H - 4, W * 4, [L.FMT_DXT5],
                                          [1], [1], [small])
    assert r == 0 and res == [0]
    other[0][0] = small[: used[0]].tobytes()
    other[2][1] = frames[2][0]                               # a Hap Alpha frame where two textures are read
    pictures = canvases(kinds)
    r, res = ctx.composite_frames(other, None, COUNTS, pictures, W, H, opacities=opacities)
    code, _p = decoded_with(ctx, frames[2][0], 2)
    assert code != 0
    assert r == bad and res == [bad, 0, 0, 0, 0, 0, 0, code, 0]
    check_frames(pictures, decoded, opacities, None, [False, True, False])
    # one output picture NULL: every entry of that output frame
    pictures = canvases((kinds[0], None, kinds[2]))
    r, res = ctx.composite_frames(frames, None, COUNTS, pictures, W, H, opacities=opacities)
    assert r == bad and res == [0, 0, 0, bad, bad, bad, 0, 0, 0]
    check_frames(pictures, decoded, opacities, None, [True, False, True])


def test_a_misaligned_device_picture_fails_alone(ctx, hap, movie):
    frames, decoded = movie
    bad = hap.HapResult.Bad_Arguments
    off = dev_canvas(W, H)
    pictures = [dev_canvas(W, H), off[4:], dev_canvas(W, H)]
    r, res = ctx.composite_frames(frames, None, COUNTS, pictures, W, H)
    assert r == bad and res == [0, 0, 0, bad, bad, bad, 0, 0, 0]
    assert (off.cpu().numpy() == SENTINEL).all()
    check_frames([pictures[0], None, pictures[2]], decoded, None, None, [True, False, True])


@pytest.mark.parametrize("kinds", (("device",) * 3, ("host",) * 3), ids=("device", "host"))
def test_a_frame_with_more_blocks_than_the_canvas(ctx, hap, movie, kinds):
    """One layer's DXT5 frame a block row taller than the canvas: the second stage has no room for it, and the call hands
    its Buffer_Too_Small on for that entry; as a placed layer of the canvas's size the same frame is one of another size,
    Bad_Arguments.  The other output frames are written either way."""
    frames, decoded = movie
    bad, too_small = hap.HapResult.Bad_Arguments, hap.HapResult.Buffer_Too_Small
    tall_picture = np.ascontiguousarray(np.concatenate([source_picture(30), source_picture(31)[:4]]))
    tall = np.zeros(hap.HapMaxEncodedLength([(W // 4) * (H // 4 + 1) * 16], [L.FMT_DXT5], [1]), dtype=np.uint8)
    r, used, res = ctx.encode_frames_rgba([tall_picture], W, H + 4, W * 4, [L.FMT_DXT5], [1], [1], [tall])
    assert r == 0 and res == [0]
    other = [list(fr) for fr in frames]
    other[1][0] = tall[: used[0]].tobytes()
    pictures = canvases(kinds)
    r, res = ctx.composite_frames(other, None, COUNTS, pictures, W, H, opacities=DISSOLVE)
    assert r == too_small and res == [0, 0, 0, too_small, 0, 0, 0, 0, 0]
    check_frames(pictures, decoded, DISSOLVE, None, [True, False, True])
    pictures = canvases(kinds)
    r, res = ctx.composite_frames_placed(other, None, COUNTS, [(W, H)] * LAYERS, pictures, W, H, opacities=DISSOLVE)
    assert r == bad and res == [0, 0, 0, bad, 0, 0, 0, 0, 0]
    check_frames(pictures, decoded, DISSOLVE, None, [True, False, True])


# ------------------------------------------------------------------------------------------------ 7. repeatability --
def test_the_same_call_twice_gives_the_same_bytes(ctx, movie):
    frames, _decoded = movie
    first, second = canvases(("device",) * FRAMES), canvases(("device",) * FRAMES)
    for pictures in (first, second):
        r, res = ctx.composite_frames(frames, None, COUNTS, pictures, W, H, opacities=DISSOLVE, background=K.BACKGROUNDS[3])
        assert r == 0 and res == [0] * (FRAMES * LAYERS)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    w, h = 260, 8
    _host, device, _decoded = stack(ctx, CASES, w, h)
    once = composited(ctx, device, w, h, [254, 127, 128, 1], K.BACKGROUNDS[3], True)
    assert np.array_equal(once, composited(ctx, device, w, h, [254, 127, 128, 1], K.BACKGROUNDS[3], True))


# ------------------------------------------------------------------------------------------------------ 8. slicing --
def test_more_output_frames_than_one_slice_holds(ctx, hap):
    """A call stages its layers' textures 32768 at a time; opacities, inputs and pictures are the call's.  Two layers
    with texture counts (1, 2) are three entries an output frame, so a slice holds 10922 output frames: 10922 + 9 of
    8 x 4 texels, cycling through 5 layer pairs of random blocks and 7 opacity pairs -- 10922 is 2 modulo 7, so an
    opacity looked up by a frame's place in its slice is another frame's."""
    w, h, counts = 8, 4, (1, 2)
    n = 32768 // 3 + 9
    rng = np.random.default_rng(8)

    def blocks(nbytes):
        return rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()

    made = [[hap.HapEncode([blocks(32)], [L.FMT_DXT5], [1], [1]), hap.HapEncode([blocks(32), blocks(16)], [L.FMT_YCOCG, L.FMT_RGTC1], [1, 1], [1, 1])]
            for _ in range(5)]
    assert all(r == 0 for pair in made for r, _frame in pair)
    made = [[frame for _r, frame in pair] for pair in made]
    decoded = []
    for pair in made:
        pictures = []
        for frame, count in zip(pair, counts):
            out = np.zeros(h * w * 4, dtype=np.uint8)
            _r, res = ctx.decode_frames_rgba([frame], [len(frame)], count, [out], w, h)
            assert res == [0]
            pictures.append(out.reshape(h, w, 4))
        decoded.append(pictures)
    levels = [(255, 255), (254, 1), (128, 127), (0, 255), (127, 254), (1, 128), (255, 0)]
    background = K.BACKGROUNDS[3]
    want = np.stack([np.stack([K.composite(decoded[i], o, background) for o in levels]) for i in range(5)])    # [5, 7, h, w, 4]
    assert len({want[i, o].tobytes() for i in range(5) for o in range(7)}) == 35
    # the frames in device memory, behind each other at 256-byte steps
    step = 256
    assert max(len(f) for pair in made for f in pair) <= step
    store = np.zeros(10 * step, dtype=np.uint8)
    for i, pair in enumerate(made):
        for l, f in enumerate(pair):
            store[(2 * i + l) * step: (2 * i + l) * step + len(f)] = np.frombuffer(f, np.uint8)
    store = torch.from_numpy(store).cuda()
    frames = [[store[(2 * (f % 5) + l) * step: (2 * (f % 5) + l + 1) * step] for l in range(2)] for f in range(n)]
    lens = [[len(made[f % 5][l]) for l in range(2)] for f in range(n)]
    out = torch.full((n, h * w * 4), SENTINEL, dtype=torch.uint8, device="cuda")
    r, res = ctx.composite_frames(frames, lens, counts, list(out), w, h, opacities=[levels[f % 7] for f in range(n)],
                                  background=background)
    assert r == 0 and res == [0] * (2 * n)
    f = np.arange(n)
    got = out.cpu().numpy().reshape(n, h, w, 4)
    wrong = np.argwhere((got != want[f % 5, f % 7]).reshape(n, -1).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()

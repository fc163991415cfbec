"""HAPGPU_ENCODE_REFINE_ENDPOINTS on the GPU: every call that honours the flag makes the blocks of the numpy definition
(tests/_refined_endpoints.py), bit for bit, and every call and format that ignores it makes the default's.

Pictures of 272 x 16 texels, 68 x 4 blocks: a full wave plus a four-lane tail in every block row.  Two are crops of the
quality pictures, where the definition changes 233 (noisy) and 272 (hard_edge) of the 272 blocks, the third is made of
the blocks at the edges of the definition (R.edge_blocks()).  At least half the blocks of every picture differ from the
default's, so "the bytes are the definition's" cannot hold where the flag is ignored.
"""
import numpy as np
import pytest

import _data as D
import _libs as L
import _refined_endpoints as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H = 272, 16
BLOCKS = (W // 4) * (H // 4)
ORA = L.oracle_api()
REF = L.ref_api() or ORA              # the unmodified reference where oracle/_ref is built, else its restatement


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


@pytest.fixture(scope="module")
def pictures():
    """name -> (picture, default DXT1, default DXT5, refined DXT1, refined DXT5), made once and read-only"""
    q = D.quality_images()
    pics = {"noisy": np.ascontiguousarray(q["noisy"][:H, :W]), "hard_edge": np.ascontiguousarray(q["hard_edge"][:H, :W]),
            "edges": R.picture_of(R.edge_blocks(), W // 4)}
    out = {}
    for name, img in pics.items():
        d1, d5 = D.oracle_bc_encode(img, L.FMT_DXT1), D.oracle_bc_encode(img, L.FMT_DXT5)
        r1 = R.encode_dxt1(img)
        r5 = R.encode_dxt5(img, d5)
        changed = int(R.changed(r1, img).sum())
        print("%s: %d of %d blocks changed" % (name, changed, BLOCKS))
        assert changed >= BLOCKS // 2, name
        img.setflags(write=False)
        out[name] = (img, d1, d5, r1.tobytes(), r5.tobytes())
    assert int(R.changed(np.frombuffer(out["noisy"][3], np.uint8), out["noisy"][0]).sum()) == 233
    assert int(R.changed(np.frombuffer(out["hard_edge"][3], np.uint8), out["hard_edge"][0]).sum()) == 272
    return out


def placed(img, road, where):
    """the picture as the call gets it: (buffer, row_bytes).  wide: 16-byte aligned, rows of w * 4; narrow: at a 4-byte
    offset, rows 4 bytes longer (no multiple of 16)"""
    h, w = img.shape[:2]
    row_bytes = w * 4 + (4 if road == "narrow" else 0)
    raw = np.full(h * row_bytes + 32, 0xA7, np.uint8)
    start = (-raw.ctypes.data) % 16 + (4 if road == "narrow" else 0)
    view = raw[start:start + h * row_bytes]
    view.reshape(h, row_bytes)[:, :w * 4] = img.reshape(h, w * 4)
    if where == "host":
        return view, row_bytes, raw
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    start = (-t.data_ptr()) % 16 + (4 if road == "narrow" else 0)
    return t[start:start + h * row_bytes], row_bytes, t


def first_difference(got, want, block):
    g, w = np.frombuffer(got, np.uint8).reshape(-1, block), np.frombuffer(want, np.uint8).reshape(-1, block)
    bad = np.flatnonzero((g != w).any(1))
    return None if len(bad) == 0 else (len(bad), int(bad[0]), g[bad[0]].tobytes().hex(), w[bad[0]].tobytes().hex())


# ------------------------------------------------------------------------------------------------- textures --
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("road", ["wide", "narrow"])
@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5], ids=["dxt1", "dxt5"])
def test_compress_rgba_is_the_definition(ctx, hap, pictures, fmt, road, where):
    for name, (img, d1, d5, r1, r5) in pictures.items():
        src, row_bytes, _keep = placed(img, road, where)
        r, got = ctx.compress_rgba(src, W, H, row_bytes, fmt, flags=hap.ENCODE_REFINE_ENDPOINTS)
        want = r1 if fmt == L.FMT_DXT1 else r5
        assert r == 0 and first_difference(got, want, D.BLOCK_BYTES[fmt]) is None, (name, first_difference(got, want, D.BLOCK_BYTES[fmt]))
        r, plain = ctx.compress_rgba(src, W, H, row_bytes, fmt)
        assert r == 0 and plain == (d1 if fmt == L.FMT_DXT1 else d5), name
        if fmt == L.FMT_DXT5:              # the alpha halves are the unflagged call's
            a, b = np.frombuffer(got, np.uint8).reshape(-1, 16), np.frombuffer(plain, np.uint8).reshape(-1, 16)
            assert (a[:, :8] == b[:, :8]).all() and (a[:, 8:] != b[:, 8:]).any(1).sum() >= BLOCKS // 2, name


@pytest.mark.parametrize("fmt", [L.FMT_YCOCG, L.FMT_RGTC1], ids=["ycocg", "rgtc1"])
def test_other_formats_ignore_the_flag(ctx, hap, pictures, fmt):
    for name, (img, *_rest) in pictures.items():
        r, got = ctx.compress_rgba(img, W, H, W * 4, fmt, flags=hap.ENCODE_REFINE_ENDPOINTS)
        assert r == 0 and got == D.oracle_bc_encode(img, fmt), name


# --------------------------------------------------------------------------------------------------- frames --
def encode(ctx, hap, imgs, fmts, flags, halves=False, chunks=None):
    chunks = chunks or [1] * len(fmts)
    sizes = [BLOCKS * D.BLOCK_BYTES[f] for f in fmts]
    cap = hap.HapMaxEncodedLength(sizes, fmts, chunks)
    outs = [np.zeros(cap, np.uint8) for _ in imgs]
    args = (imgs, W, H, W * 4, fmts, [L.COMP_SNAPPY] * len(fmts), chunks, outs)
    if halves:
        assert ctx.encode_frames_rgba_begin(*args, flags=flags) == 0
        r, used, res = ctx.encode_finish()
    else:
        r, used, res = ctx.encode_frames_rgba(*args, flags=flags)
    assert r == 0 and res == [0] * len(imgs), (r, res)
    return [o[:u].tobytes() for o, u in zip(outs, used)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("index", [0, 1], ids=["plain", "fragment_index"])
@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5], ids=["hap", "hap_alpha"])
def test_frames_hold_the_refined_textures(ctx, hap, pictures, fmt, index, where):
    names = ["noisy", "edges"]
    imgs = [pictures[n][0] for n in names]
    want = [pictures[n][3 if fmt == L.FMT_DXT1 else 4] for n in names]
    if where == "device":
        imgs = [torch.from_numpy(i.copy()).cuda() for i in imgs]
        torch.cuda.synchronize()
    flags = hap.ENCODE_REFINE_ENDPOINTS | (hap.ENCODE_FRAGMENT_INDEX if index else 0)
    frames = encode(ctx, hap, imgs, [fmt], flags)
    assert frames == encode(ctx, hap, imgs, [fmt], flags, halves=True)
    size = BLOCKS * D.BLOCK_BYTES[fmt]
    # ... and the ...OnDevices form, dealt out over this one device
    cap = hap.HapMaxEncodedLength([size], [fmt], [1])
    dealt = [np.zeros(cap, np.uint8) for _ in imgs]
    r, used, res = hap.encode_frames_rgba_on_devices([ctx], imgs, W, H, W * 4, [fmt], [L.COMP_SNAPPY], [1], dealt, flags=flags)
    assert r == 0 and res == [0, 0] and [o[:u].tobytes() for o, u in zip(dealt, used)] == frames
    outs = [np.zeros(size, np.uint8) for _ in frames]
    r, used, fmts, res = ctx.decode_frame_textures(frames, [len(f) for f in frames], 1, outs)
    assert r == 0 and res == [0, 0] and list(fmts) == [fmt, fmt] and list(used) == [size, size]
    for o, w, n in zip(outs, want, names):
        assert first_difference(o.tobytes(), w, D.BLOCK_BYTES[fmt]) is None, (n, first_difference(o.tobytes(), w, D.BLOCK_BYTES[fmt]))
    assert REF.decode(frames[0], 0, size) == (0, want[0], fmt)
    # and without the flag the same call makes the default's
    plain = encode(ctx, hap, imgs, [fmt], flags & ~hap.ENCODE_REFINE_ENDPOINTS)
    assert ORA.decode(plain[0], 0, size) == (0, pictures["noisy"][1 if fmt == L.FMT_DXT1 else 2], fmt)


@pytest.mark.parametrize("fmts", [[L.FMT_YCOCG], [L.FMT_YCOCG, L.FMT_RGTC1]], ids=["hap_q", "hap_q_alpha"])
def test_hap_q_frames_ignore_the_flag(ctx, hap, pictures, fmts):
    imgs = [pictures["noisy"][0], pictures["hard_edge"][0]]
    for index in (0, hap.ENCODE_FRAGMENT_INDEX):
        assert encode(ctx, hap, imgs, fmts, index | hap.ENCODE_REFINE_ENDPOINTS) == encode(ctx, hap, imgs, fmts, index)


def test_sequence_frames_hold_the_refined_textures(ctx, hap, pictures, tmp_path):
    imgs = [pictures[n][0] for n in ("noisy", "hard_edge", "edges")]
    flags = hap.ENCODE_REFINE_ENDPOINTS | hap.ENCODE_FRAGMENT_INDEX
    want = encode(ctx, hap, imgs, [L.FMT_DXT1], flags)
    path = str(tmp_path / "refined.hapseq")
    with hap.SequenceWriter(path, W, H) as writer:
        r, nbytes, res = ctx.encode_sequence(writer, imgs, W, H, W * 4, [L.FMT_DXT1], [L.COMP_SNAPPY], [1], flags=flags, batch=2)
        assert (r, res) == (0, [0] * 3) and nbytes == [len(f) for f in want]
    reader = hap.SequenceReader(path)
    assert reader.read(0, 3) == (0, want)
    reader.close()


@pytest.mark.parametrize("fmt", [L.FMT_DXT1, L.FMT_DXT5], ids=["hap", "hap_alpha"])
def test_planes_with_the_flag_are_the_pictures_with_the_flag(ctx, hap, pictures, fmt):
    """three half planes holding the bytes themselves, identity scale: alpha is 255"""
    names = ["hard_edge", "edges"]
    imgs = []
    for n in names:
        img = pictures[n][0].copy()
        img[..., 3] = 255
        imgs.append(img)
    flags = hap.ENCODE_REFINE_ENDPOINTS | hap.ENCODE_FRAGMENT_INDEX
    want = encode(ctx, hap, imgs, [fmt], flags)
    tensor = torch.from_numpy(np.ascontiguousarray(np.stack([i[..., :3].transpose(2, 0, 1) for i in imgs]), np.float16)).cuda()
    size = BLOCKS * D.BLOCK_BYTES[fmt]
    cap = hap.HapMaxEncodedLength([size], [fmt], [1])
    outs = [np.zeros(cap, np.uint8) for _ in imgs]
    r, used, res = ctx.encode_frames_planes(tensor, W, H, [fmt], [L.COMP_SNAPPY], [1], outs, scale=[1.0] * 3, bias=[0.0] * 3,
                                            flags=flags)
    assert r == 0 and res == [0, 0]
    assert [o[:u].tobytes() for o, u in zip(outs, used)] == want
    refined = R.encode_dxt1(imgs[0]).tobytes() if fmt == L.FMT_DXT1 else R.encode_dxt5(imgs[0], D.oracle_bc_encode(imgs[0], fmt)).tobytes()
    assert ORA.decode(want[0], 0, size) == (0, refined, fmt)
    outs2 = [np.zeros(cap, np.uint8) for _ in imgs]
    assert ctx.encode_frames_planes_begin(tensor, W, H, [fmt], [L.COMP_SNAPPY], [1], outs2, scale=[1.0] * 3, bias=[0.0] * 3,
                                          flags=flags) == 0
    r, used2, res = ctx.encode_finish()
    assert r == 0 and res == [0, 0] and [o[:u].tobytes() for o, u in zip(outs2, used2)] == want


# ----------------------------------------------------------------------------------------------- measurement --
def test_measured_error_is_the_definitions_and_smaller(ctx, hap, pictures):
    names = ["noisy", "hard_edge"]
    imgs = [pictures[n][0] for n in names]
    refs = [torch.from_numpy(i.copy()).cuda() for i in imgs]
    torch.cuda.synchronize()
    totals = {}
    for flagged in (False, True):
        frames = encode(ctx, hap, imgs, [L.FMT_DXT1], hap.ENCODE_REFINE_ENDPOINTS if flagged else 0)
        r, res, errors = ctx.measure_frames(frames, [len(f) for f in frames], 1, refs, W, H)
        assert r == 0 and res == [0, 0]
        totals[flagged] = [sum(e.sse[:3]) for e in errors]
    print("sse default -> refined:", totals[False], "->", totals[True])
    for k, img in enumerate(imgs):
        px = R.blocks_of(img)
        assert totals[True][k] == int(R.err(px, *R.refined_block(px)).sum())
        assert totals[False][k] == int(R.err(px, *R.default_block(px)).sum())
        assert totals[True][k] < totals[False][k]
    assert (totals[False], totals[True]) == ([626928, 9497616], [545794, 5578552])


# ------------------------------------------------------------------------------------------------- transcode --
def test_transcode_ignores_the_flag(ctx, hap, pictures):
    """the documented ignore: the destination blocks stay as the default encode would make them"""
    imgs = [pictures["noisy"][0], pictures["hard_edge"][0]]
    sources = encode(ctx, hap, imgs, [L.FMT_YCOCG], hap.ENCODE_FRAGMENT_INDEX)
    size = BLOCKS * 8
    cap = hap.HapMaxEncodedLength([size], [L.FMT_DXT1], [1])
    got = {}
    for flags in (0, hap.ENCODE_REFINE_ENDPOINTS):
        outs = [np.zeros(cap, np.uint8) for _ in sources]
        r, used, res = ctx.transcode_frames(sources, [len(f) for f in sources], 1, W, H, 0, [L.FMT_DXT1], [L.COMP_SNAPPY], [1],
                                            outs, encode_flags=flags)
        assert r == 0 and res == [0, 0]
        got[flags] = [o[:u].tobytes() for o, u in zip(outs, used)]
    assert got[0] == got[hap.ENCODE_REFINE_ENDPOINTS]

"""The BC7 reference encoder (tests/_bc7_encode.py), the definition bptc_encode.hip reproduces: every block decodes
through the scalar decoder of tests/_bptc.py to exactly the texels the encoder measured, only modes 1, 5 and 6 appear,
opaque input stays opaque, solid blocks come back within 1, and the quality on the pinned pictures is recorded."""
import numpy as np
import pytest

import _bc7_encode as E
import _bptc as B
import _data as D

# PSNR (colour, alpha) through _bptc.decode on _data.quality_images(), as given ("alpha") and with alpha forced to 255
# ("opaque"); each value may not fall more than 0.3 dB.
QUALITY_BC7 = {
    ("smooth", "alpha"): (50.07, 58.63),
    ("smooth", "opaque"): (50.99, 99.00),
    ("noisy", "alpha"): (31.51, 41.42),
    ("noisy", "opaque"): (33.75, 99.00),
    ("hard_edge", "alpha"): (22.35, 31.64),
    ("hard_edge", "opaque"): (29.43, 99.00),
}
# the project's DXT5 (colour) and scaled YCoCg-DXT5 on the same pictures: what Hap R has to beat
DXT5_RGB = {"smooth": 43.9, "noisy": 30.8, "hard_edge": 19.8}
YCOCG_RGB = {"smooth": 46.5, "hard_edge": 27.2}


def opaque(img):
    o = img.copy()
    o[..., 3] = 255
    return o


def sample_blocks():
    rng = np.random.default_rng(0xB7)
    out = [E.to_blocks(img) for img in D.quality_images().values()]
    out += [E.to_blocks(opaque(img)) for img in D.quality_images().values()]
    noise = rng.integers(0, 256, (3000, 16, 4), dtype=np.uint8)
    binary = noise.copy()
    binary[..., 3] = rng.integers(0, 2, (3000, 16)) * 255
    flat = noise.copy()
    flat[..., 3] = 255
    # few distinct values per block: two-colour blocks, blocks of two nearby colours
    pal = rng.integers(0, 256, (3000, 2, 4), dtype=np.uint8)
    two = np.take_along_axis(pal, rng.integers(0, 2, (3000, 16, 1)).repeat(4, -1), 1)
    out += [noise, binary, flat, two]
    return np.concatenate(out)


def test_every_block_decodes_to_what_the_encoder_measured():
    texels = sample_blocks()
    blocks, pred, _modes = E.encode_blocks(texels)
    uniq, first = np.unique(blocks, axis=0, return_index=True)
    for i in first:
        got = np.array(B.decode_block(blocks[i].tobytes()), dtype=np.uint8)
        assert np.array_equal(got, pred[i]), (i, blocks[i].tobytes().hex())
    # the predicted texels are what the error was measured on: the winner is never worse than mode 6 alone
    x = texels.astype(np.int64)
    _b6, _d6, e6 = E._mode6(x, (x[..., 3] == 255).all(1))
    err = ((pred.astype(np.int64) - x) ** 2).sum((1, 2))
    assert (err <= e6).all()


def test_only_the_documented_modes_appear():
    texels = sample_blocks()
    blocks, _pred, modes = E.encode_blocks(texels)
    first = blocks[:, 0]
    assert (first != 0).all()                                          # no reserved block
    mode_of = np.array([(int(b) & -int(b)).bit_length() - 1 for b in first])
    assert np.array_equal(mode_of, modes)
    assert set(np.unique(modes)) <= set(E.MODES_USED)
    op = (texels[..., 3] == 255).all(1)
    assert set(np.unique(modes[op])) <= {1, 6} and set(np.unique(modes[~op])) <= {5, 6}
    # mode 5 blocks use rotation 0
    m5 = modes == 5
    assert ((blocks[m5, 0] >> 6) == 0).all()


def test_anchor_indices_have_their_top_bit_clear():
    texels = sample_blocks()
    blocks, _pred, modes = E.encode_blocks(texels)
    for i in np.nonzero(modes == 1)[0][:3000]:
        v = int.from_bytes(blocks[i].tobytes(), "little")
        part = (v >> 2) & 63
        anchor = B.ANCHORS_2[part]
        # indices start at bit 82, 3 bits each, 2 at texels 0 and `anchor`; the anchor's field is read one bit short,
        # so its stored value is its index: both below 4
        pos, idx = 82, []
        for t in range(16):
            nb = 2 if t in (0, anchor) else 3
            idx.append((v >> pos) & ((1 << nb) - 1))
            pos += nb
        assert pos == 128
        dec = B.decode_block(blocks[i].tobytes())
        assert idx[0] < 4 and idx[anchor] < 4 and len(dec) == 16
    # the rule on the encoder's own mode-6 indices: texel 0's top bit is clear after it, and it does swap sometimes
    x = texels.astype(np.int64)
    for b, fn in ((4, lambda: E._fit(x, np.ones(x.shape[:2], bool), 4, lambda a, c: E.quantize_mode6(a, c, np.zeros(len(x), bool)))),):
        _r, idx = fn()
        n = len(x)
        fixed, swapped, _ = E._swap_for_anchor(idx, b, np.zeros(n, np.int64), np.ones((n, 16), bool), [])
        assert ((fixed[:, 0] >> (b - 1)) == 0).all()
        assert swapped.any() and (~swapped).any()


def test_opaque_input_decodes_opaque_and_solid_blocks_within_one():
    rng = np.random.default_rng(5)
    texels = sample_blocks()
    op = texels.copy()
    op[..., 3] = 255
    _b, pred, _m = E.encode_blocks(op)
    assert (pred[..., 3] == 255).all()
    colours = rng.integers(0, 256, (4096, 4), dtype=np.uint8)
    colours[:1024, 3] = 255
    colours[1024:1040] = [[0, 0, 0, 0], [255, 255, 255, 255], [0, 0, 0, 255], [255, 255, 255, 0]] * 4
    solid = np.repeat(colours[:, None, :], 16, 1)
    blocks, pred, _m = E.encode_blocks(solid)
    for i in range(0, len(blocks), 37):
        assert np.array_equal(np.array(B.decode_block(blocks[i].tobytes()), dtype=np.uint8), pred[i])
    assert (np.abs(pred.astype(int) - solid.astype(int)) <= 1).all()
    assert (pred[:1024, :, 3] == 255).all()


def test_the_output_is_deterministic():
    img = D.quality_images()["noisy"]
    assert E.encode(img) == E.encode(img.copy())
    t = E.to_blocks(img)
    assert np.array_equal(E.encode_blocks(t)[0], E.encode_blocks(t[::-1])[0][::-1])


@pytest.mark.parametrize("name", ["smooth", "noisy", "hard_edge"])
def test_quality_is_pinned(name):
    img = D.quality_images()[name]
    h, w = img.shape[:2]
    for label, im in (("alpha", img), ("opaque", opaque(img))):
        dec = B.decode(E.encode(im), w, h)
        rgb, a = D.psnr(dec[..., :3], im[..., :3]), D.psnr(dec[..., 3], im[..., 3])
        want_rgb, want_a = QUALITY_BC7[(name, label)]
        assert rgb >= want_rgb - 0.3 and a >= want_a - 0.3, (name, label, rgb, a)
        assert rgb > DXT5_RGB[name], (name, label, rgb)
        if label == "opaque" and name in YCOCG_RGB:
            assert rgb > YCOCG_RGB[name], (name, rgb)

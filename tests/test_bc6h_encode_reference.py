"""The BC6H reference encoder (tests/_bc6h_encode.py), the definition bc6h_encode.hip reproduces, in both formats: every
block decodes through the scalar decoder of tests/_bc6h.py to exactly the texels the encoder predicted and measured, only
the documented modes appear, anchors keep their top bit clear, the winner is never worse than mode 0x03 alone, solid
blocks come back exactly, specials encode as their normalised values, and the quality on the pinned pictures is recorded.

Hard edges: the full encoder against the one-region modes alone is 46.08 against 42.07 dB (unsigned) and 45.80 against
42.05 dB (signed) on the hard-edge picture: +4.0 and +3.8 dB from the two-region modes."""
import numpy as np
import pytest

import _bc6h as H
import _bc6h_encode as E
import _hdr_data as HD

# psnr_half = 10 log10(0x7BFF^2 / mse) over the integer half patterns, from the definition on the CPU, per picture and
# (unsigned, signed) format; each value may not fall more than 0.3 dB.
QUALITY_BC6H = {
    "smooth": (65.75, 64.60),
    "noisy": (60.39, 60.20),
    "hard_edge": (46.08, 45.80),
    "signed": (60.05, 55.68),
    "specials": (19.86, 15.35),
}
ONE_REGION_HARD_EDGE = (42.07, 42.05)


def sample_blocks():
    rng = np.random.default_rng(0xBC6)
    out = [E.to_blocks(pic) for pic in HD.hdr_images().values()]
    noise = rng.integers(0, 65536, (2000, 16, 4), dtype=np.uint16)
    pal = rng.integers(0, 65536, (2000, 2, 4), dtype=np.uint16)
    two = np.take_along_axis(pal, rng.integers(0, 2, (2000, 16, 1)).repeat(4, -1), 1)
    solid = np.repeat(rng.integers(0, 65536, (1000, 1, 4), dtype=np.uint16), 16, 1)
    near = (rng.integers(0x2000, 0x5000, (1000, 1, 4)) + rng.integers(0, 48, (1000, 16, 4))).astype(np.uint16)
    return np.concatenate(out + [noise, two, solid, near])


def error_of(pred, texels, signed):
    d = E.normalise(pred, True) - E.normalise(texels, signed)
    return (d * d).sum((1, 2))


@pytest.mark.parametrize("signed", [False, True])
def test_every_block_decodes_to_what_the_encoder_predicted(signed):
    texels = sample_blocks()
    blocks, pred, _modes = E.encode_blocks(texels, signed)
    _uniq, first = np.unique(blocks, axis=0, return_index=True)
    for i in first:
        got = np.array(H.decode_block(blocks[i].tobytes(), signed), dtype=np.uint16)
        assert np.array_equal(got, pred[i]), (i, blocks[i].tobytes().hex())
    # the predicted texels are what the error was measured on: the winner is never worse than mode 0x03 alone
    h = E.normalise(texels, signed)
    _mode, _w, _d, e03, _v = E._one_region(E.to_working(h, signed), h, signed)[0]
    assert (error_of(pred, texels, signed) <= e03).all()


@pytest.mark.parametrize("signed", [False, True])
def test_only_the_documented_modes_appear(signed):
    texels = sample_blocks()
    blocks, _pred, modes = E.encode_blocks(texels, signed)
    values = np.array([H.mode_index(b.tobytes())[1] for b in blocks])
    assert np.array_equal(values, modes)
    assert not set(np.unique(values)) & set(H.RESERVED)
    assert set(np.unique(values)) <= set(E.MODES_USED)
    assert set(E.ONE_REGION) <= set(np.unique(values))                   # every one-region mode wins somewhere
    assert {0x1E, 0x00} <= set(np.unique(values))
    # one region alone: the same blocks, one-region modes only
    _b, _p, m1 = E.encode_blocks(texels, signed, two_regions=False)
    assert set(np.unique(m1)) <= set(E.ONE_REGION)


@pytest.mark.parametrize("signed", [False, True])
def test_anchor_indices_have_their_top_bit_clear(signed):
    texels = sample_blocks()[::3]
    blocks, pred, modes = E.encode_blocks(texels, signed)
    for i in range(0, len(blocks), 5):
        v = int.from_bytes(blocks[i].tobytes(), "little")
        two = int(modes[i]) in E.TWO_REGION
        ib, pos = (3, 82) if two else (4, 65)
        anchors = (0, H.ANCHORS_2[(v >> 77) & 31]) if two else (0,)
        # an anchor's field is one bit short, so what is stored there is its whole index: re-insert a zero top bit for
        # every anchor and the decoder's picture must not change
        idx = []
        for t in range(16):
            n = ib - 1 if t in anchors else ib
            idx.append((v >> pos) & ((1 << n) - 1))
            pos += n
        assert pos == 128
        assert all(idx[a] < (1 << (ib - 1)) for a in anchors)
    # the rule does swap sometimes and not always
    h = E.normalise(texels, signed)
    x = E.to_working(h, signed)
    m = np.ones(x.shape[:2], bool)
    fp = E._first_pass(x, m, 4, 10, signed)
    q0, _q1, _d0, _d1, idx = E._final(x, m, 4, fp, 10, signed, np.zeros(len(x), np.int64))
    assert ((idx[:, 0] >> 3) == 0).all()
    raw0, _ = E.quantise(fp[0], 10, signed)
    swapped = (raw0 != q0).any(1)
    assert swapped.any() and (~swapped).any()


@pytest.mark.parametrize("signed", [False, True])
def test_solid_blocks_decode_to_exactly_their_normalised_colour(signed):
    rng = np.random.default_rng(6)
    colours = rng.integers(0, 65536, (4096, 1, 4), dtype=np.uint16)
    colours[:len(HD.SPECIALS), 0, :3] = np.array(HD.SPECIALS, np.uint16)[:, None]
    solid = np.repeat(colours, 16, 1)
    blocks, pred, _modes = E.encode_blocks(solid, signed)
    want = E.to_pattern(E.normalise(solid, signed))
    assert np.array_equal(pred[..., :3], want)
    assert (pred[..., 3] == 0x3C00).all()
    for i in range(0, len(blocks), 29):
        assert np.array_equal(np.array(H.decode_block(blocks[i].tobytes(), signed), dtype=np.uint16), pred[i])


def test_specials_encode_as_their_normalised_values_and_alpha_changes_no_byte():
    inf, ninf, nan, nnan, nzero, neg, big = 0x7C00, 0xFC00, 0x7E01, 0xFE01, 0x8000, 0xBC00, 0x7BFF
    t = np.zeros((7, 16, 4), np.uint16)
    for i, v in enumerate((inf, ninf, nan, nnan, nzero, neg, big)):
        t[i, :, :3] = v
    want = {False: (big, 0, 0, 0, 0, 0, big), True: (big, 0x8000 | big, 0, 0, 0, neg, big)}
    for signed in (False, True):
        _b, pred, _m = E.encode_blocks(t, signed)
        assert [int(pred[i, 0, 0]) for i in range(7)] == list(want[signed])
        assert all((pred[i, :, :3] == pred[i, 0, 0]).all() for i in range(7))
        # a special next to ordinary values is the same block as its normalised value there
        pic = HD.specials()
        norm = pic.copy()
        norm[..., :3] = E.to_pattern(E.normalise(pic, signed))
        assert E.encode(pic, signed) == E.encode(norm, signed)
        garbage = pic.copy()
        garbage[..., 3] = np.arange(256, dtype=np.uint16).reshape(16, 16) * 257
        assert E.encode(pic, signed) == E.encode(garbage, signed)


def test_the_output_is_deterministic_and_independent_of_block_order():
    pic = HD.hdr_images()["noisy"]
    for signed in (False, True):
        assert E.encode(pic, signed) == E.encode(pic.copy(), signed)
        t = E.to_blocks(pic)[:2048]
        assert np.array_equal(E.encode_blocks(t, signed)[0], E.encode_blocks(t[::-1], signed)[0][::-1])
        assert np.array_equal(E.encode_blocks(t, signed)[0][100:164], E.encode_blocks(t[100:164], signed)[0])


@pytest.mark.parametrize("name", sorted(QUALITY_BC6H))
def test_quality_is_pinned(name):
    pic = HD.hdr_images()[name]
    h, w = pic.shape[:2]
    for signed in (False, True):
        dec = H.decode(E.encode(pic, signed), w, h, signed)
        got = E.psnr_half(dec, pic, signed)
        assert got >= QUALITY_BC6H[name][int(signed)] - 0.3, (name, signed, got)
        if name == "hard_edge":
            one = H.decode(E.encode(pic, signed, two_regions=False), w, h, signed)
            got_one = E.psnr_half(one, pic, signed)
            assert got_one >= ONE_REGION_HARD_EDGE[int(signed)] - 0.3 and got > got_one, (signed, got, got_one)


def test_a_float16_cast_picture_encodes_and_the_trigger_is_per_wave():
    import _data as D
    pic = HD.from_float16(D.quality_images()["smooth"])[:64, :256]
    h, w = pic.shape[:2]
    dec = H.decode(E.encode(pic, False), w, h, False)
    one = H.decode(E.encode(pic, False, two_regions=False), w, h, False)
    assert E.psnr_half(dec, pic, False) >= E.psnr_half(one, pic, False)      # (more candidates never lose)
    # a wave of solid blocks does not ask for the two-region modes; one block of three colours that lie on no line (two
    # endpoints cannot reach them) makes it ask
    t = np.repeat(np.arange(64, dtype=np.uint16).reshape(64, 1, 1) * 100 + 0x3000, 16, 1).repeat(4, 2)
    assert not E.wave_tries_two_regions(t, False)
    t[7, :5, 0] = 0x5000
    t[7, 5:10, 1] = 0x5000
    assert E.wave_tries_two_regions(t, False)

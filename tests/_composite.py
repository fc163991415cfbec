"""numpy's form of the compositing definition (include/hap_gpu.h: HapGpuCompositeTextures, HapGpuCompositeFrames), in
int64, and the constants the compositing tests share.

The canvas is RGBA8 with its colour premultiplied by its alpha; layers are straight alpha.  For a layer's texel
(Rs, Gs, Bs, As), its opacity byte o and the canvas (Rd, Gd, Bd, Ad):
    a  = rdiv255(As * o)
    Cd = rdiv255(Cs * a + Cd * (255 - a))      for C = R, G, B
    Ad = a + rdiv255(Ad * (255 - a))
rdiv255(x): the integer nearest to x / 255 for 0 <= x <= 65025 -- t = x + 128; (t + (t >> 8)) >> 8.

TEST INFRASTRUCTURE ONLY: nothing in hap_amd/ imports this module."""
import numpy as np

MAX_LAYERS = 16
OPACITIES = (0, 1, 127, 128, 254, 255)
BACKGROUNDS = ((0, 0, 0, 255), (0, 0, 0, 0), (200, 100, 50, 255), (17, 34, 51, 128))
DEFAULT_BACKGROUND = (0, 0, 0, 255)
# one lane; two lanes; 65 blocks a row (a block row ends inside a wave); 272 blocks (a second workgroup with 16 live lanes)
GEOMETRIES = ((4, 4), (8, 4), (260, 8), (68, 64))
SENTINEL = 0xA7


def rdiv255(x):
    t = np.asarray(x, dtype=np.int64) + 128
    return (t + (t >> 8)) >> 8


def layer_alpha(As, o):
    return rdiv255(np.asarray(As, dtype=np.int64) * np.asarray(o, dtype=np.int64))


def blend_colour(Cs, Cd, a):
    Cs, Cd, a = (np.asarray(v, dtype=np.int64) for v in (Cs, Cd, a))
    return rdiv255(Cs * a + Cd * (255 - a))


def blend_alpha(Ad, a):
    Ad, a = (np.asarray(v, dtype=np.int64) for v in (Ad, a))
    return a + rdiv255(Ad * (255 - a))


def composite(pictures, opacities=None, background=None):
    """The canvas after `pictures` ([h, w, 4] uint8 arrays, bottom to top) have gone over `background` with `opacities`
    (None: all 255; background None: 0, 0, 0, 255): an [h, w, 4] uint8 array"""
    h, w, _ = pictures[0].shape
    opacities = [255] * len(pictures) if opacities is None else list(opacities)
    assert len(opacities) == len(pictures)
    canvas = np.empty((h, w, 4), dtype=np.int64)
    canvas[:] = np.asarray(DEFAULT_BACKGROUND if background is None else background, dtype=np.int64)
    for picture, o in zip(pictures, opacities):
        assert picture.shape == (h, w, 4) and picture.dtype == np.uint8
        s = picture.astype(np.int64)
        a = layer_alpha(s[:, :, 3], o)
        for c in range(3):
            canvas[:, :, c] = blend_colour(s[:, :, c], canvas[:, :, c], a)
        canvas[:, :, 3] = blend_alpha(canvas[:, :, 3], a)
    assert canvas.min() >= 0 and canvas.max() <= 255
    return canvas.astype(np.uint8)

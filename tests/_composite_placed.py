"""numpy's form of the placed compositing definition (include/hap_gpu.h: HapGpuPlacement, HapGpuCompositeTexturesPlaced,
HapGpuCompositeFramesPlaced), and the geometries the placed compositing tests share.

A placement (srcX, srcY, width, height, dstX, dstY) puts a rectangle of a layer's picture on the canvas: canvas texel
(x, y) is covered when dstX <= x < dstX + width and dstY <= y < dstY + height, and takes the layer's texel at
(srcX + x - dstX, srcY + y - dstY) by _composite.py's three formulas; a texel that is not covered is left alone, and
what falls outside the canvas is clipped.  Here that is slicing: the visible part of the rectangle, cut out of the
picture, blended into the same part of the canvas.

TEST INFRASTRUCTURE ONLY: nothing in hap_amd/ imports this module."""
import numpy as np

import _composite as K

DST_MAX = 1 << 20
# one lane; 16 blocks a row (a wave spans four block rows: coverage differs lane by lane); a block row ends inside a
# wave; a second workgroup with 16 live lanes
CANVASES = ((4, 4), (64, 32), (260, 8), (68, 64))
# smallest; smaller than the canvas; equal to the 64 x 32 canvas; wider and taller than every canvas (its blocks per row
# differ from the canvas's); as wide as the widest canvas; narrow and taller than every canvas
LAYERS = ((4, 4), (16, 16), (64, 32), (128, 64), (260, 8), (8, 68))


def whole(layer_size):
    """the placement placements=None stands for"""
    return (0, 0, layer_size[0], layer_size[1], 0, 0)


def valid(placement, layer_size):
    """the definition's rules for one placement of a layer of layer_size"""
    sx, sy, w, h, dx, dy = placement
    lw, lh = layer_size
    return (all(v % 4 == 0 for v in placement) and w > 0 and h > 0 and sx >= 0 and sy >= 0 and sx + w <= lw and sy + h <= lh
            and abs(dx) <= DST_MAX and abs(dy) <= DST_MAX)


def visible(placement, canvas_size):
    """(x0, y0, x1, y1) of the canvas texels the placement covers; None: none"""
    _sx, _sy, w, h, dx, dy = placement
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + w, canvas_size[0]), min(dy + h, canvas_size[1])
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


def composite_placed(canvas_size, pictures, placements, opacities=None, background=None):
    """The canvas_size = (width, height) canvas after `pictures` ([h_l, w_l, 4] uint8 arrays of sizes of their own, bottom
    to top) have gone over `background` with `placements` (None, or None entries: the layer whole at (0, 0)) and
    `opacities` (None: all 255): an [height, width, 4] uint8 array"""
    width, height = canvas_size
    opacities = [255] * len(pictures) if opacities is None else list(opacities)
    placements = [None] * len(pictures) if placements is None else list(placements)
    assert len(opacities) == len(pictures) == len(placements)
    canvas = np.empty((height, width, 4), dtype=np.int64)
    canvas[:] = np.asarray(K.DEFAULT_BACKGROUND if background is None else background, dtype=np.int64)
    for picture, placement, o in zip(pictures, placements, opacities):
        assert picture.ndim == 3 and picture.shape[2] == 4 and picture.dtype == np.uint8
        size = (picture.shape[1], picture.shape[0])
        placement = whole(size) if placement is None else tuple(placement)
        assert valid(placement, size), (placement, size)
        box = visible(placement, canvas_size)
        if box is None:
            continue
        x0, y0, x1, y1 = box
        sx, sy, _w, _h, dx, dy = placement
        s = picture[sy + y0 - dy: sy + y1 - dy, sx + x0 - dx: sx + x1 - dx].astype(np.int64)
        d = canvas[y0:y1, x0:x1]                       # (a view: the canvas is blended in place)
        a = K.layer_alpha(s[:, :, 3], o)
        for c in range(3):
            d[:, :, c] = K.blend_colour(s[:, :, c], d[:, :, c], a)
        d[:, :, 3] = K.blend_alpha(d[:, :, 3], a)
    assert canvas.min() >= 0 and canvas.max() <= 255
    return canvas.astype(np.uint8)

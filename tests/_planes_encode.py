"""What the planar encode tests share: the definition of HapGpuCompressPlanes' quantiser in numpy, the constants the
issue names, and the float set of the sweeps.  No GPU, no library."""
import numpy as np

F16, BF16, F32 = 0, 1, 2                                   # HapGpuPlaneElement

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# (scale, bias) pairs every sweep runs under; the last three are the ImageNet inverse per channel: a model's
# (x / 255 - mean) / std undone, scale = 255 * std, bias = 255 * mean
CONSTANTS = [(255.0, 0.0), (127.5, 127.5), (1.0, 0.0), (float(2 ** 24), 0.0)] + [
    (float(np.float32(255.0 * s)), float(np.float32(255.0 * m))) for s, m in zip(IMAGENET_STD, IMAGENET_MEAN)]


def values_of(kind, bits):
    """the elements' values as float32 (exact for all three kinds; subnormals kept)"""
    bits = np.asarray(bits)
    if kind == F16:
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    if kind == BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.astype(np.uint32).view(np.float32)


def quantise(x, scale, bias):
    """The definition: one float32 multiply, one float32 add, NaN -> 0, rint (halves to even), clip."""
    with np.errstate(all="ignore"):
        r = x.astype(np.float32) * np.float32(scale) + np.float32(bias)
        assert r.dtype == np.float32
        return np.where(np.isnan(r), 0, np.clip(np.rint(r), 0, 255)).astype(np.uint8)


def float_set(seed=20261019, random=100000):
    """float32 bit patterns: every k + 0.5 for k in 0..255 with both neighbours, the neighbours of 0 and 255, +-0, +-Inf,
    quiet and signalling NaNs, subnormals, and seeded random patterns"""
    ties = (np.arange(256, dtype=np.float32) + np.float32(0.5))
    edge = np.concatenate([ties, np.nextafter(ties, np.float32(-np.inf)), np.nextafter(ties, np.float32(np.inf)),
                           np.nextafter(np.float32([0, 0, 255, 255]), np.float32([-np.inf, np.inf, -np.inf, np.inf])),
                           np.float32([0.0, 255.0, 1.0, 254.0, 256.0, -1.0, -255.0, 1e30, -1e30])]).view(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                  # +-0, +-Inf
                        0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7FFFFFFF,                  # quiet NaNs
                        0x7F800001, 0xFF800001, 0x7FA00000, 0x7FBFFFFF,                  # signalling NaNs
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,      # subnormals
                        0x00000020, 0x00001000, 0x00012345, 0x00800000, 0x80800000], dtype=np.uint32)
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 2 ** 32, size=random, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([edge, special, rnd])


def picture_of(tensor, scale, bias):
    """The picture of a (C, H, W) float tensor given as float32 values: (H, W, 4) uint8, A 255 with three planes"""
    c, h, w = tensor.shape
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    for i in range(c):
        out[..., i] = quantise(tensor[i], scale[i], bias[i])
    return out

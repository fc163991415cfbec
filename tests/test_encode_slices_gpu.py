"""Encode calls of more frames than one launch sequence holds.  A blocking encode call works through its frames 32768 at
a time, whatever they are made from: RGBA8 pictures, planar float tensors, RGBA16F pictures, A8 pictures, or textures the
client made.  The pictures, outputs, sizes and results are the call's, so every slice looks them up from where it
begins.  The definition is the same entry point called with a handful of frames: a frame of the long call is byte for
byte, in `used` and in its result the frame the short call makes of the same picture.  A ...Begin call takes no more than
one slice and refuses a longer one before it looks at anything else."""
import ctypes as C

import numpy as np
import pytest

import _libs as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA7
SLICE = 32768
N = SLICE + 40                      # 32768 is 3 modulo 5: a picture looked up by a slice-relative index is another one
NULL_AT = SLICE + 3                 # a frame of the second slice without a picture
W = H = 4                           # one block: the smallest frames the offsets between slices can go wrong with
STEP = 256                          # from one picture to the next in device memory
SNAPPY = L.COMP_SNAPPY
F32 = 2                             # HapGpuPlaneElement_F32


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


def random_store(seed):
    """5 x STEP random bytes in device memory"""
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.integers(0, 256, 5 * STEP, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def pictures(seed, nbytes):
    """5 pictures of nbytes random bytes each, STEP bytes apart"""
    store = random_store(seed)
    return [store[i * STEP: i * STEP + nbytes] for i in range(5)]


def plane_tensors(seed):
    """5 (3, H, W) float32 tensors of random bytes that share their strides"""
    return [p.view(torch.float32).reshape(3, H, W) for p in pictures(seed, 3 * H * W * 4)]


def texture_pairs(seed):
    """5 [YCoCg-DXT5, RGTC1] pairs of random blocks"""
    store = random_store(seed)
    return [[store[i * STEP: i * STEP + 16], store[i * STEP + 128: i * STEP + 136]] for i in range(5)]


# name: (the 5 sources, the source that is none, the texture formats, the blocking call)
SOURCES = {
    "rgba8": (lambda: pictures(11, W * H * 4), None, [L.FMT_DXT1],
              lambda c, src, outs: c.encode_frames_rgba(src, W, H, W * 4, [L.FMT_DXT1], [SNAPPY], [1], outs, 0)),
    "planes_f32": (lambda: plane_tensors(12), None, [L.FMT_DXT1],
                   lambda c, src, outs: c.encode_frames_planes(src, W, H, [L.FMT_DXT1], [SNAPPY], [1], outs, flags=0)),
    "rgba16f": (lambda: pictures(13, W * H * 8), None, [L.FMT_BC6U],
                lambda c, src, outs: c.encode_frames_rgba_half(src, W, H, W * 8, L.FMT_BC6U, SNAPPY, 1, outs, 0)),
    "a8": (lambda: pictures(14, W * H), None, [L.FMT_RGTC1],
           lambda c, src, outs: c.encode_frames_alpha(src, W, H, W, SNAPPY, 1, outs, 0)),
    # (two textures a frame: a slice's textures begin at its first frame times two)
    "textures": (lambda: texture_pairs(15), [None, None], [L.FMT_YCOCG, L.FMT_RGTC1],
                 lambda c, src, outs: c.encode_frames(src, [L.FMT_YCOCG, L.FMT_RGTC1], [SNAPPY] * 2, [1, 1], outs, 0)),
}
BLOCK_BYTES = {L.FMT_DXT1: 8, L.FMT_RGTC1: 8, L.FMT_YCOCG: 16, L.FMT_BC6U: 16}


def host_slots(n, cap):
    return torch.full((n, cap), SENTINEL, dtype=torch.uint8)


@pytest.mark.parametrize("name", list(SOURCES))
def test_more_frames_than_one_slice_holds(ctx, hap, name):
    make, none, fmts, call = SOURCES[name]
    five = make()
    cap = hap.HapMaxEncodedLength([BLOCK_BYTES[f] for f in fmts], fmts, [1] * len(fmts))
    # what one short call makes of the five, and of a frame without a picture
    small = host_slots(6, cap)
    r6, used6, res6 = call(ctx, five + [none], list(small))
    bad = hap.HapResult.Bad_Arguments
    print(name, "short call:", r6, used6, res6)
    assert res6 == [0] * 5 + [bad] and r6 == bad
    small = small.numpy()
    assert len({small[i, : used6[i]].tobytes() for i in range(5)}) == 5
    assert all((small[i, used6[i]:] == SENTINEL).all() for i in range(5))
    # the long call: frame i is picture i % 5, every frame has a slot of its own in one host buffer
    which = np.arange(N) % 5
    which[NULL_AT] = 5
    out = host_slots(N, cap)
    r, used, res = call(ctx, [(five + [none])[k] for k in which], list(out))
    print(name, "long call:", r, "results that are not 0:", [(i, code) for i, code in enumerate(res) if code][:8])
    assert r == r6
    assert res == [res6[k] for k in which]                          # (Bad_Arguments at NULL_AT and nowhere else)
    assert used == [used6[k] for k in which]
    wrong = np.argwhere((out.numpy() != small[which]).any(axis=1)).ravel()
    assert wrong.size == 0, wrong[:8].tolist()


def test_a_begin_call_takes_one_slice_at_most(hap):
    """Each ...Begin with 32769 frames: Bad_Arguments, no result written, and the context takes the next call."""
    lib = hap._lib.lib
    n = SLICE + 1
    bad = hap.HapResult.Bad_Arguments
    c = hap.Context(0)
    try:
        for name, (make, _none, fmts, call) in SOURCES.items():
            five = make()
            cap = hap.HapMaxEncodedLength([BLOCK_BYTES[f] for f in fmts], fmts, [1] * len(fmts))
            room = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
            count = len(fmts)
            first = five[0] if count == 2 else [five[0]]
            ptrs = (C.c_void_p * (n * count))(*[t.data_ptr() for t in first] * n)
            optrs = (C.c_void_p * n)(*[room.data_ptr()] * n)
            olens = (C.c_ulong * n)(*[cap] * n)
            used = (C.c_ulong * n)()
            results = (C.c_uint * n)(*[0xA7A7A7A7] * n)
            tail = (optrs, olens, used, results, 0)
            formats, snappy, ones = (C.c_uint * count)(*fmts), (C.c_uint * count)(*[SNAPPY] * count), (C.c_uint * count)(*[1] * count)
            if name == "rgba8":
                r = lib.HapGpuEncodeFramesRGBABegin(c.handle, n, ptrs, W, H, W * 4, 1, formats, snappy, ones, *tail)
            elif name == "planes_f32":
                unit = (C.c_float * 3)(255.0, 255.0, 255.0)
                zero = (C.c_float * 3)(0.0, 0.0, 0.0)
                r = lib.HapGpuEncodeFramesPlanesBegin(c.handle, n, ptrs, 3, F32, H * W * 4,
                                                      W * 4, unit, zero, W, H, 1, formats, snappy, ones, *tail)
            elif name == "rgba16f":
                r = lib.HapGpuEncodeFramesRGBAHalfBegin(c.handle, n, ptrs, W, H, W * 8, L.FMT_BC6U, SNAPPY, 1, *tail)
            elif name == "a8":
                r = lib.HapGpuEncodeFramesAlphaBegin(c.handle, n, ptrs, W, H, W, SNAPPY, 1, *tail)
            else:
                lens = (C.c_ulong * 2)(16, 8)
                r = lib.HapGpuEncodeFramesBegin(c.handle, n, 2, ptrs, lens, formats, snappy, ones, *tail)
            assert r == bad, name
            assert (np.frombuffer(results, np.uint32) == 0xA7A7A7A7).all(), name
            # nothing is in flight: a blocking call of two frames goes through
            r2, _used2, res2 = call(c, five[:2], list(host_slots(2, cap)))
            assert r2 == 0 and res2 == [0, 0], name
    finally:
        c.close()

"""The taps and the blend of the resized-crop road (hap_amd/csrc/resample_taps.hpp) against their definition
(tests/_resample.py), without a GPU.

The header is __host__ __device__: tests/c/resample_taps_host.hip compiles it for the host (no device pass).  The taps
of every element of every axis pair up to 64 x 64 and of the sizes where the arithmetic is nearest its limits; the blend
over all 256 x 256 x 257 (a, b, w) of one axis, along x and along y, and over 2^20 random texel quadruples with both
weights -- once as the definition's function and once as the packed form the kernel runs.  The numpy definition itself
is pinned against rational arithmetic."""
import ctypes
import fractions
import os
import subprocess

import numpy as np
import pytest

import _resample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"definition": 0, "kernel": 1}
LARGE = (1, 2, 3, 223, 224, 1080, 4097, 16383, 16384)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resample_taps") / "libresample_taps_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "resample_taps_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.resample_taps.argtypes = [ctypes.c_uint, ctypes.c_uint] + [ctypes.c_void_p] * 3
    lib.resample_taps.restype = None
    lib.resample_blend_axis_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.resample_blend_axis_sweep.restype = None
    lib.resample_blend_texels.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 7
    lib.resample_blend_texels.restype = None
    return lib


def host_taps(host, o, c):
    out = [np.full(o, 0xEEEEEEEE, dtype=np.uint32) for _ in range(3)]
    host.resample_taps(o, c, *[a.ctypes.data for a in out])
    return [a.astype(np.int64) for a in out]


def same_taps(host, o, c):
    for name, got, want in zip(("i0", "i1", "w"), host_taps(host, o, c), S.taps(o, c)):
        wrong = np.argwhere(got != want).ravel()
        assert wrong.size == 0, (o, c, name, [(int(i), int(got[i]), int(want[i])) for i in wrong[:4]])


def test_the_numpy_definition_is_the_rational_one():
    """Pixel centres: element i samples at s = (i + 1/2) * c / o - 1/2, clamped at 0; i0 = floor(s), the weight is
    s - i0 in 256ths rounded to nearest, halves up; taps stay inside the crop"""
    F = fractions.Fraction
    for o in list(range(1, 40)) + [224]:
        for c in list(range(1, 40)) + [223]:
            i0, i1, w = S.taps(o, c)
            for i in range(o):
                s = max(F(2 * i + 1, 2) * F(c, o) - F(1, 2), F(0))
                floor = s.numerator // s.denominator
                assert i0[i] == min(floor, c - 1) and i1[i] == min(i0[i] + 1, c - 1), (o, c, i)
                assert w[i] == ((s - floor) * 256 + F(1, 2)).__floor__(), (o, c, i)
            assert w.min() >= 0 and w.max() <= 256
            if o == c:                                         # the identity: every weight 0, every tap its own texel
                assert (w == 0).all() and np.array_equal(i0, np.arange(o))
    # the blend: weight 0 keeps the first texel, 256 takes the second, and the rounding is to nearest, halves up
    v = np.arange(256)
    assert np.array_equal(S.blend(v, 255 - v, 7, 9, 0, 0), v) and np.array_equal(S.blend(3, v, 7, 9, 256, 0), v)
    assert np.array_equal(S.blend(3, 5, v, 9, 0, 256), v) and np.array_equal(S.blend(3, 5, 7, v, 256, 256), v)
    assert S.blend(0, 1, 0, 1, 128, 0) == 1 and S.blend(0, 1, 0, 1, 127, 0) == 0 and S.blend(0, 255, 0, 255, 128, 77) == 128


def test_every_tap_of_the_small_axes(host):
    for o in range(1, 65):
        for c in range(1, 65):
            same_taps(host, o, c)


def test_every_tap_where_the_arithmetic_is_nearest_its_limits(host):
    for o in LARGE:
        for c in LARGE:
            same_taps(host, o, c)
            i0, i1, w = S.taps(o, c)
            assert w.min() >= 0 and w.max() <= 256 and i0.max() <= c - 1 and i1.max() <= c - 1
    # the widest crop a call takes: four times the largest output -- (2 i + 1) c stays below 2^32
    same_taps(host, 16384, 65536)
    assert (2 * 16383 + 1) * 65536 < 1 << 32


@pytest.mark.parametrize("axis", ("x", "y"))
@pytest.mark.parametrize("form", list(FORMS))
def test_every_blend_of_one_axis(host, form, axis):
    out = np.full(256 * 256 * 257, 0xEEEE, dtype=np.uint16)
    host.resample_blend_axis_sweep(FORMS[form], axis == "y", out.ctypes.data)
    got = out.reshape(256, 256, 257).astype(np.int64)
    a, b, w = np.meshgrid(np.arange(256), np.arange(256), np.arange(257), indexing="ij")
    want = (a * (256 - w) + b * w) * 256 + 32768 >> 16
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, [(int(i), int(j), int(k), int(got[i, j, k]), int(want[i, j, k])) for i, j, k in wrong[:8]]
    # ... which is what the definition gives with the other axis's weight 0, whatever the other two texels hold
    some = np.random.default_rng(3).integers(0, 256 * 256 * 257, 4096)
    sa, sb, sw = a.ravel()[some], b.ravel()[some], w.ravel()[some]
    if axis == "x":
        assert np.array_equal(S.blend(sa, sb, 99, 200, sw, 0), want.ravel()[some])
    else:
        assert np.array_equal(S.blend(sa, 99, sb, 200, 0, sw), want.ravel()[some])


@pytest.mark.parametrize("form", list(FORMS))
def test_random_texels_with_both_weights(host, form):
    n = 1 << 20
    rng = np.random.default_rng(20)
    p = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    # (byte extremes among them: every eighth quadruple is made of 0x00 and 0xFF bytes only)
    for q in p:
        q[::8] = np.where(rng.integers(0, 2, (n // 8, 4)) == 1, 255, 0).astype(np.uint32) @ np.array([1, 1 << 8, 1 << 16, 1 << 24],
                                                                                                      dtype=np.uint32)
    wx = rng.integers(0, 257, n).astype(np.uint32)
    wy = rng.integers(0, 257, n).astype(np.uint32)
    wx[:1024], wy[:1024] = np.repeat([0, 256, 0, 256], 256), np.repeat([0, 0, 256, 256], 256)
    out = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    host.resample_blend_texels(FORMS[form], n, *[a.ctypes.data for a in p + [wx, wy, out]])
    for k in range(4):
        want = S.blend(*[(q >> (8 * k)) & 255 for q in p], wx, wy)
        got = (out >> (8 * k)) & 255
        wrong = np.argwhere(got != want).ravel()
        assert wrong.size == 0, (k, [(int(j), int(got[j]), int(want[j])) for j in wrong[:4]])

"""The quantiser of the planar encode road (hap_amd/csrc/plane_quantise.hpp) against its definition, without a GPU.

quantise() and the three element loads are __host__ __device__: tests/c/plane_quantise_host.hip compiles them for the host
(no device pass) and every bit pattern of the sweeps comes out as numpy's
    r = x.astype(float32) * float32(s) + float32(b);  v = where(isnan(r), 0, clip(rint(r), 0, 255))
makes it: all 65536 halves, all 65536 bfloat16s, and a float set around the ties, the ends, the NaNs and the subnormals.
The device's own instructions (v_cvt_f32_f16, v_rndne_f32, the denormal mode) are tests/test_planes_encode_gpu.py's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _planes_encode as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plane_quantise") / "libplane_quantise_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "plane_quantise_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.plane_quantise.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_void_p]
    lib.plane_values.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def run(lib, kind, bits, scale, bias):
    bits = np.ascontiguousarray(bits, dtype=np.uint32 if kind == P.F32 else np.uint16)
    out = np.empty(bits.size, dtype=np.uint8)
    assert lib.plane_quantise(kind, bits.ctypes.data, bits.size, scale, bias, out.ctypes.data) == 0
    return out


SETS = {"f16": (P.F16, np.arange(65536, dtype=np.uint16)), "bf16": (P.BF16, np.arange(65536, dtype=np.uint16)),
        "f32": (P.F32, P.float_set())}


@pytest.mark.parametrize("name", list(SETS))
def test_the_loads_are_exact(host, name):
    kind, bits = SETS[name]
    out = np.empty(bits.size, dtype=np.uint32)
    assert host.plane_values(kind, bits.ctypes.data, bits.size, out.ctypes.data) == 0
    want = P.values_of(kind, bits).view(np.uint32)
    nan = np.isnan(want.view(np.float32))
    assert np.array_equal(out[~nan], want[~nan])
    assert np.isnan(out.view(np.float32)[nan]).all()
    if kind == P.F16:
        # the 1023 positive subnormal halves are k * 2^-24, not zero
        assert np.array_equal(out.view(np.float32)[1:1024], np.arange(1, 1024, dtype=np.float32) * np.float32(2.0 ** -24))


@pytest.mark.parametrize("constants", P.CONSTANTS, ids=lambda c: "%g,%g" % c)
@pytest.mark.parametrize("name", list(SETS))
def test_quantise_is_the_definition(host, name, constants):
    kind, bits = SETS[name]
    scale, bias = constants
    got = run(host, kind, bits, scale, bias)
    want = P.quantise(P.values_of(kind, bits), scale, bias)
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, [(hex(int(bits[i])), int(got[i]), int(want[i])) for i in wrong[:8]]


def test_the_definition_says_what_the_issue_says():
    """numpy's form against the cases the definition spells out"""
    x = np.float32([0.5, 1.5, 2.5, 254.5, 253.5, -0.0, 0.0, np.nan, np.inf, -np.inf, -3.0, 255.0, 254.49, 300.0])
    assert list(P.quantise(x, 1.0, 0.0)) == [0, 2, 2, 254, 254, 0, 0, 0, 255, 0, 0, 255, 254, 255]


def test_subnormal_halves_count(host):
    """(2^24, 0) turns the 1023 subnormal halves into the integers 1 .. 1023: flushing them would give zeros"""
    got = run(host, P.F16, np.arange(0, 1024, dtype=np.uint16), float(2 ** 24), 0.0)
    assert np.array_equal(got, np.minimum(np.arange(1024), 255).astype(np.uint8))


def decoded(kind, scale, bias):
    """bc_decode_planes.hip's element for every byte, as the element kind's bit patterns"""
    r = np.arange(256, dtype=np.float32) * np.float32(scale) + np.float32(bias)
    if kind == P.F32:
        return r.view(np.uint32)
    if kind == P.F16:
        return r.astype(np.float16).view(np.uint16)
    # bfloat16, to nearest even: the upper half of the binary32 pattern, rounded on the lower (no NaN among these)
    b = r.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize("kind,there,back", [
    (P.F32, (1.0 / 255.0, 0.0), (255.0, 0.0)), (P.F16, (1.0 / 255.0, 0.0), (255.0, 0.0)),
    (P.BF16, (1.0 / 255.0, 0.0), (255.0, 0.0)),
    (P.F32, (2.0 / 255.0, -1.0), (127.5, 127.5)), (P.F16, (2.0 / 255.0, -1.0), (127.5, 127.5))])
def test_every_byte_comes_back(host, kind, there, back):
    """The decode road's element of a byte, quantised with the inverse constants, is the byte: all 256, through the kinds
    the pair holds for"""
    bits = decoded(kind, *there)
    assert np.array_equal(run(host, kind, bits, *back), np.arange(256, dtype=np.uint8))
    assert np.array_equal(P.quantise(P.values_of(kind, bits), *back), np.arange(256, dtype=np.uint8))

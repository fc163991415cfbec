"""The blend of the compositing road (hap_amd/csrc/composite_blend.hpp) against its definition, without a GPU.

The header is __host__ __device__: tests/c/composite_blend_host.hip compiles it for the host (no device pass) and sweeps
it completely -- all 256 x 256 (As, o) -> a, all 256^3 (Cs, Cd, a) -> Cd, all 256 x 256 (Ad, a) -> Ad -- once as the
definition's functions and once as the packed 16-bit forms the kernel runs; both come out as tests/_composite.py's numpy
makes them.  Outputs are 16 bits wide, so a value above 255 would show."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _composite as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"definition": 0, "kernel": 1}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("composite_blend") / "libcomposite_blend_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "composite_blend_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.composite_rdiv255.argtypes = [ctypes.c_void_p]
    for name in ("composite_layer_alpha", "composite_blend_colour", "composite_blend_alpha"):
        getattr(lib, name).argtypes = [ctypes.c_int, ctypes.c_void_p]
        getattr(lib, name).restype = None
    lib.composite_rdiv255.restype = None
    return lib


def sweep(function, form, n):
    out = np.full(n, 0xEEEE, dtype=np.uint16)
    function(form, out.ctypes.data)
    return out.astype(np.int64)


def test_rdiv255_is_the_nearest_integer(host):
    out = np.full(65026, 0xEEEE, dtype=np.uint16)
    host.composite_rdiv255(out.ctypes.data)
    x = np.arange(65026, dtype=np.int64)
    assert np.array_equal(out, (2 * x + 255) // 510)
    assert np.array_equal(K.rdiv255(x), (2 * x + 255) // 510)
    # no x lies on a tie: 2 x is never an odd multiple of 255
    assert not ((2 * x) % 510 == 255).any()


@pytest.mark.parametrize("form", list(FORMS))
def test_every_layer_alpha(host, form):
    got = sweep(host.composite_layer_alpha, FORMS[form], 1 << 16).reshape(256, 256)
    As, o = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = K.layer_alpha(As, o)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in wrong[:8]]


@pytest.mark.parametrize("form", list(FORMS))
def test_every_colour(host, form):
    got = sweep(host.composite_blend_colour, FORMS[form], 1 << 24).reshape(256, 256, 256)
    Cd, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for Cs in range(256):               # (a plane at a time: 65536 values each)
        want = K.blend_colour(Cs, Cd, a)
        wrong = np.argwhere(got[Cs] != want)
        assert wrong.size == 0, [(Cs, int(i), int(j), int(got[Cs, i, j]), int(want[i, j])) for i, j in wrong[:8]]


@pytest.mark.parametrize("form", list(FORMS))
def test_every_canvas_alpha(host, form):
    got = sweep(host.composite_blend_alpha, FORMS[form], 1 << 16).reshape(256, 256)
    Ad, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = K.blend_alpha(Ad, a)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in wrong[:8]]


def test_the_definition_says_what_the_issue_says():
    """numpy's form against the cases the definition spells out"""
    v = np.arange(256, dtype=np.int64)
    s, d = np.meshgrid(v, v, indexing="ij")
    # a = 255 replaces the texel: colour and alpha
    assert np.array_equal(K.blend_colour(s, d, 255), s)
    assert (K.blend_alpha(v, 255) == 255).all()
    # a = 0 keeps it
    assert np.array_equal(K.blend_colour(s, d, 0), d)
    assert np.array_equal(K.blend_alpha(v, 0), v)
    # an opaque source at full opacity has a = 255, at none a = 0; a transparent source a = 0 at any opacity
    assert K.layer_alpha(255, 255) == 255 and (K.layer_alpha(v, 0) == 0).all() and (K.layer_alpha(0, v) == 0).all()
    assert np.array_equal(K.layer_alpha(v, 255), v) and np.array_equal(K.layer_alpha(255, v), v)
    # rdiv255 is the nearest integer, written three ways
    x = np.arange(65026, dtype=np.int64)
    assert np.array_equal(K.rdiv255(x), (2 * x + 255) // 510)
    assert np.array_equal(K.rdiv255(x), np.rint(x / 255.0).astype(np.int64))
    # alpha never exceeds 255 and never falls
    Ad, a = np.meshgrid(v, v, indexing="ij")
    out = K.blend_alpha(Ad, a)
    assert out.max() == 255 and (out >= Ad).all() and (out >= a).all()
    # one whole picture: an opaque layer at full opacity is the layer, whatever the background
    rng = np.random.default_rng(1)
    layer = rng.integers(0, 256, (4, 8, 4), dtype=np.uint8)
    layer[:, :, 3] = 255
    for background in K.BACKGROUNDS:
        assert np.array_equal(K.composite([layer], [255], background), layer)
        assert (K.composite([layer], [0], background) == np.asarray(background, dtype=np.uint8)).all()
    assert np.array_equal(K.composite([layer]), K.composite([layer], [255], K.DEFAULT_BACKGROUND))

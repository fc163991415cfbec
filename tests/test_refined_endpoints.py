"""HAPGPU_ENCODE_REFINE_ENDPOINTS on the CPU: the numpy definition (tests/_refined_endpoints.py) against the oracle, its
consequences, its arithmetic, and the kernels' per-block functions (hap_amd/csrc/bc_refine_core.hpp, __host__ __device__)
compiled for the host by tests/c/refine_endpoints_host.hip.  The device-only parts (v_rcp_f32, the 24-bit multiplies, the
byte dot products, partial waves) are tests/test_refined_endpoints_gpu.py's.

For the record, colour PSNR of DXT1 through the oracle's decoder, default -> refined, and the blocks the flag changes:
smooth 43.943 -> 44.039 dB (362 of 8192), noisy 30.824 -> 31.428 dB (7392), hard_edge 19.775 -> 22.114 dB (8192).
"""
import ctypes
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _data as D
import _libs as L
import _refined_endpoints as R

ROOT = L.ROOT


@pytest.fixture(scope="module")
def pictures():
    out = {}
    for name, img in D.quality_images().items():
        px = R.blocks_of(img)
        out[name] = (img, px, R.pack(*R.default_block(px)), R.pack(*R.refined_block(px)))
    return out


def _decoded_errors(blocks, img):
    """per block, the squared error of the oracle decoder's picture of DXT1 `blocks` against img's R, G, B"""
    h, w = img.shape[:2]
    dec = D.oracle_bc_decode(blocks.tobytes(), L.FMT_DXT1, w, h)
    return ((R.blocks_of(dec) - R.blocks_of(img)) ** 2).sum((1, 2))


# ------------------------------------------------------------------------------------ the definition itself --
@pytest.mark.parametrize("name", ["smooth", "noisy", "hard_edge"])
def test_restated_default_is_the_oracles(pictures, name):
    img, _px, default, _refined = pictures[name]
    assert default.tobytes() == D.oracle_bc_encode(img, L.FMT_DXT1)


@pytest.mark.parametrize("name", ["smooth", "noisy", "hard_edge"])
def test_no_block_gets_worse_and_the_picture_gets_better(pictures, name):
    img, px, default, refined = pictures[name]
    e_default, e_refined = _decoded_errors(default, img), _decoded_errors(refined, img)
    # (the definition's own err is the decoder's)
    assert (e_refined == R.err(px, *R.unpack(refined))).all() and (e_default == R.err(px, *R.unpack(default))).all()
    assert (e_refined <= e_default).all()
    same = ~R.changed(refined, img)
    assert (refined[same] == default[same]).all() and (e_refined[~same] < e_default[~same]).all()
    print("%s: sse %d -> %d, %d of %d blocks changed, %.3f -> %.3f dB" % (
        name, e_default.sum(), e_refined.sum(), (~same).sum(), len(same),
        D.block_quality(default.tobytes(), L.FMT_DXT1, img)[0], D.block_quality(refined.tobytes(), L.FMT_DXT1, img)[0]))
    assert e_refined.sum() < e_default.sum()


def test_a_round_that_does_not_win_ends_the_refinement(pictures):
    """two unconditional rounds are "stop at the first failure": a block the first round leaves alone is left alone by
    the second"""
    _img, px, default, _refined = pictures["noisy"]
    once = R.pack(*R.refined_block(px, rounds=1))
    twice = R.pack(*R.refined_block(px, rounds=2))
    lost = (once == default).all(1)
    assert lost.any() and (~lost).any() and (twice[lost] == default[lost]).all()


def test_rounded_quotient_is_the_exact_rounding():
    rng = np.random.default_rng(7)
    px = rng.integers(0, 256, (2000, 16, 3)).astype(np.int64)
    idx = rng.integers(0, 4, (2000, 16))
    idx[:100] = rng.integers(0, 2, (100, 16)) * 2                         # few entries in use: small determinants
    na, nb, det = R.numerators(px, idx)
    checked = 0
    for num in (na, nb):
        got = R.rounded_quotient(num, np.maximum(det, 1)[:, None])
        for i in np.flatnonzero(det):
            for c in range(3):
                exact = Fraction(3 * int(num[i, c]), int(det[i]))
                want = min(max((2 * exact.numerator + exact.denominator) // (2 * exact.denominator), 0), 255)     # halves up
                assert got[i, c] == want, (i, c, num[i, c], det[i])
                checked += 1
    assert checked > 10000


def test_numerator_is_exact_as_a_float():
    """|2 * 3 * num + det| < 2^24 on the extremes: pixels all 0 or all 255 on the entries of every index histogram"""
    worst = 0
    for n0, n1, n2 in itertools.product(range(17), repeat=3):
        n3 = 16 - n0 - n1 - n2
        if n3 < 0:
            continue
        idx = np.repeat(np.arange(4), (n0, n1, n2, n3))[None, :]
        w = R.WEIGHT[idx]
        # the numerators are linear in the pixels: their extremes lie where every pixel is 0 or 255, by the sign of its
        # coefficient C w - B v (A v - B w)
        A, B, C, det = (int(v[0]) for v in R.moments(idx))
        for coeff in (C * w - B * (3 - w), A * (3 - w) - B * w):
            for sign in (1, -1):
                px = np.where(sign * coeff > 0, 255, 0).astype(np.int64)[..., None].repeat(3, 2)
                na, nb, _ = R.numerators(px, idx)
                worst = max(worst, int(np.abs(6 * na + det).max()), int(np.abs(6 * nb + det).max()))
    assert 0 < worst < 1 << 24, worst


# ------------------------------------------------------------------- the kernels' block arithmetic on the host --
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_host") / "librefine_endpoints_host.so")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-host-only",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "refine_endpoints_host.hip"), "-o", so]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.refine_candidates.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.refine_ranks.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    lib.refine_quotients.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.refine_candidates.restype = lib.refine_ranks.restype = lib.refine_quotients.restype = None
    return lib


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _words(idx):
    return _u32((idx << (2 * np.arange(16))[None, :]).sum(1))


def _host_candidate(host, px, idx):
    packed = _u32(px[..., 0] | px[..., 1] << 8 | px[..., 2] << 16)
    words, out = _words(idx), np.zeros((len(px), 3), np.uint32)
    host.refine_candidates(packed.ctypes.data, words.ctypes.data, len(px), out.ctypes.data)
    return out[:, 0] != 0, out[:, 1].astype(np.int64), out[:, 2].astype(np.int64)


def _host_err(host, px, c0, c1, idx):
    packed = _u32(px[..., 0] | px[..., 1] << 8 | px[..., 2] << 16)
    a, b, words, out = _u32(c0), _u32(c1), _words(idx), np.zeros(len(px), np.int32)
    host.refine_ranks(packed.ctypes.data, a.ctypes.data, b.ctypes.data, words.ctypes.data, len(px), out.ctypes.data)
    return out.astype(np.int64) + (px * px).sum((1, 2))


def _host_is_the_definition(host, px, what):
    """both rounds of the definition, with the host functions in the places of candidate() and err()"""
    c0, c1, idx = R.default_block(px)
    assert (_host_err(host, px, c0, c1, idx) == R.err(px, c0, c1, idx)).all(), what
    for rnd in range(R.ROUNDS):
        valid, n0, n1 = R.candidate(px, idx)
        h_valid, h0, h1 = _host_candidate(host, px, idx)
        assert (h_valid == valid).all(), (what, rnd)
        bad = np.flatnonzero(valid & ((h0 != n0) | (h1 != n1)))
        assert len(bad) == 0, (what, rnd, len(bad), px[bad[0]].tolist(), idx[bad[0]].tolist(), (h0[bad[0]], h1[bad[0]]), (n0[bad[0]], n1[bad[0]]))
        nidx = R.pick_indices(px, n0, n1)
        assert (_host_err(host, px, n0, n1, nidx) == R.err(px, n0, n1, nidx)).all(), (what, rnd)
        c0, c1, idx = R.one_round(px, c0, c1, idx)
    assert (R.pack(c0, c1, idx) == R.pack(*R.refined_block(px))).all()


def test_host_block_functions_on_random_blocks(host):
    rng = np.random.default_rng(11)
    px = rng.integers(0, 256, (20000, 16, 3)).astype(np.int64)
    px[10000:] = np.clip(rng.integers(0, 256, (10000, 1, 3)) + rng.integers(-24, 25, (10000, 16, 3)), 0, 255)
    _host_is_the_definition(host, px, "random")


def test_host_block_functions_on_the_edges(host):
    px = R.edge_blocks()
    cls = R.classes(px)
    print({k: int(v.sum()) for k, v in cls.items()})
    for name, mask in cls.items():
        assert mask.any(), name
        _host_is_the_definition(host, px[mask], name)
    _host_is_the_definition(host, px, "all")
    # what the classes are for: no candidate where the default's end points fall together; candidates that fall
    # together never win over a default that tells two colours apart
    refined = R.pack(*R.refined_block(px))
    default = R.pack(*R.default_block(px))
    assert (refined[cls["default_c0_equals_c1"]] == default[cls["default_c0_equals_c1"]]).all()


def test_host_quotient_is_the_exact_rounding(host):
    rng = np.random.default_rng(13)
    px = rng.integers(0, 256, (20000, 16, 3)).astype(np.int64)
    px[:4000] = rng.integers(0, 2, (4000, 16, 3)) * 255
    idx = rng.integers(0, 4, (20000, 16))
    idx[:2000] = rng.integers(0, 2, (2000, 16)) * 3
    na, nb, det = R.numerators(px, idx)
    ok = det != 0
    num = np.ascontiguousarray(np.concatenate([na[ok], nb[ok]]).reshape(-1), dtype=np.int32)
    d = np.ascontiguousarray(np.concatenate([det[ok], det[ok]])[:, None].repeat(3, 1).reshape(-1), dtype=np.int32)
    out = np.zeros(len(num), np.int32)
    host.refine_quotients(num.ctypes.data, d.ctypes.data, len(num), out.ctypes.data)
    want = R.rounded_quotient(num.astype(np.int64), d.astype(np.int64))
    assert (out == want).all() and (want == 0).any() and (want == 255).any() and len(num) > 100000


# ----------------------------------------------------------------------------------------------- the flag --
def test_flag_value_is_the_headers():
    import hap_amd
    text = open(os.path.join(ROOT, "include", "hap_gpu.h")).read()
    found = re.search(r"#define\s+HAPGPU_ENCODE_REFINE_ENDPOINTS\s+(0x[0-9A-Fa-f]+)u", text)
    assert found and int(found.group(1), 16) == 0x20 == hap_amd.ENCODE_REFINE_ENDPOINTS

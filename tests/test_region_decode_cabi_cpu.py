"""The region decode without a GPU: HapGpuDecodeFramesRGBARegion, HapGpuDecompressRGBARegion, HapGpuRegionNeedsBytes and
HapGpuSkippedTextureBytes are declared in the header, let out by the export map, exported by the built library and bound
by hap_amd._lib with the header's argument counts; the predicate agrees with a numpy brute force over every small texture,
region and byte range; the decode calls refuse a missing context and a bad region before they touch a device or a client's
array; the Python methods exist."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

import _libs as L

NAMES = {"HapGpuDecodeFramesRGBARegion": 15, "HapGpuDecompressRGBARegion": 14, "HapGpuRegionNeedsBytes": 8,
         "HapGpuSkippedTextureBytes": 1}


@pytest.fixture(scope="module")
def hap():
    from hap_amd.build import build
    build()
    import hap_amd
    return hap_amd


def test_the_four_functions_are_declared_listed_exported_and_bound(hap):
    text = open(os.path.join(L.ROOT, "include", "hap_gpu.h")).read()
    exports = open(os.path.join(L.ROOT, "hap_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[A-Za-z_*][A-Za-z0-9_*]*(?=;)", exports.split("global:")[1].split("local:")[0])
    lib = C.CDLL(os.path.join(L.ROOT, "hap_amd", "libhap_amd.so"))
    for name, count in NAMES.items():
        declared = re.search(r"unsigned (?:int|long) %s\(([^;]*)\);" % name, text)
        assert declared, name
        assert len(declared.group(1).split(",")) == count, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert hasattr(lib, name), name
        bound = getattr(hap._lib.lib, name)
        assert len(bound.argtypes) == count, name
    assert hap._lib.lib.HapGpuSkippedTextureBytes.restype is C.c_ulong
    for name in ("HapGpuDecodeFramesRGBARegion", "HapGpuDecompressRGBARegion", "HapGpuRegionNeedsBytes"):
        assert getattr(hap._lib.lib, name).restype is C.c_uint, name
        args = re.search(r"unsigned int %s\(([^;]*)\);" % name, text).group(1)
        assert all(word in args for word in ("regionX", "regionY", "regionWidth", "regionHeight")), name


def test_there_is_one_definition_of_the_predicate():
    """One small plain-C header that the host code, the kernel and HapGpuRegionNeedsBytes share."""
    csrc = os.path.join(L.ROOT, "hap_amd", "csrc")
    defined, users = [], []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".c", ".h", ".hip", ".hpp")):
            continue
        text = open(os.path.join(csrc, name)).read()
        if re.search(r"\bint hap_region_needs_bytes\(", text):
            defined.append(name)
        if '#include "hap_region.h"' in text:
            users.append(name)
    assert defined == ["hap_region.h"]
    assert {"hap_api.c", "hap_pictures.c", "snappy_decode.hip"} <= set(users)
    header = open(os.path.join(csrc, "hap_region.h")).read()
    assert "static inline" in header and "template" not in header and "::" not in header      # plain C


def brute(blocks_x, blocks_y, block_bytes, region):
    """needed[b] for every byte b of the texture: b belongs to a block of the region (in blocks)"""
    bx, by, bw, bh = region
    need = np.zeros((blocks_y, blocks_x, block_bytes), dtype=bool)
    need[by: by + bh, bx: bx + bw] = True
    return need.ravel()


def test_the_predicate_against_a_brute_force(hap):
    f = hap._lib.lib.HapGpuRegionNeedsBytes
    checked = 0
    for block_bytes in (8, 16):
        for blocks_x in range(1, 6):
            for blocks_y in range(1, 5):
                total = blocks_x * blocks_y * block_bytes
                for bx in range(blocks_x):
                    for bw in range(1, blocks_x - bx + 1):
                        for by in range(blocks_y):
                            for bh in range(1, blocks_y - by + 1):
                                need = brute(blocks_x, blocks_y, block_bytes, (bx, by, bw, bh))
                                # prefix[i]: needed bytes before byte i
                                prefix = np.concatenate([[0], np.cumsum(need)])
                                args = (4 * blocks_x, block_bytes, 4 * bx, 4 * by, 4 * bw, 4 * bh)
                                for first in range(0, total, 4):
                                    for count in range(4, total - first + 1, 4):
                                        want = int(prefix[first + count] > prefix[first])
                                        assert f(*args, first, count) == want, (args, first, count)
                                        checked += 1
                                # the edges of every region row, byte by byte
                                row = blocks_x * block_bytes
                                for r in range(by, by + bh):
                                    lo, hi = r * row + bx * block_bytes, r * row + (bx + bw) * block_bytes
                                    assert f(*args, lo, 1) == 1 and f(*args, hi - 1, 1) == 1
                                    # a range ending exactly at the row's first byte / beginning exactly behind its last
                                    if lo > 0:
                                        assert f(*args, lo - 1, 1) == int(need[lo - 1]), (args, r)
                                        assert f(*args, 0, lo) == int(prefix[lo] > 0), (args, r)
                                        assert f(*args, 0, lo + 1) == 1
                                    assert f(*args, hi - 1, total) == 1                # beginning exactly at its last byte
                                    if hi < total:
                                        assert f(*args, hi, 1) == int(need[hi]), (args, r)
                                        assert f(*args, hi, total - hi) == int(prefix[total] > prefix[hi]), (args, r)
                                # empty ranges, ranges behind the texture
                                assert f(*args, 0, 0) == 0 and f(*args, bx * block_bytes + by * row, 0) == 0
                                assert f(*args, total, 64) == 0 and f(*args, total + 4096, 1 << 40) == 0
                                assert f(*args, 0, (1 << 64) - 1) == 1 and f(*args, (1 << 64) - 1, (1 << 64) - 1) == 0
    assert checked > 100000


def test_the_predicate_refuses_what_the_region_rules_refuse(hap):
    f = hap._lib.lib.HapGpuRegionNeedsBytes
    assert f(16, 16, 4, 4, 8, 4, 0, 1 << 20) == 1
    for args in ((16, 16, 4, 4, 0, 4), (16, 16, 4, 4, 8, 0),                 # empty
                 (16, 16, 2, 4, 8, 4), (16, 16, 4, 2, 8, 4), (16, 16, 4, 4, 6, 4), (16, 16, 4, 4, 8, 6),   # off the grid
                 (16, 16, 12, 4, 8, 4), (16, 16, 16, 0, 4, 4), (16, 16, 20, 0, 4, 4),        # past the right edge
                 (16, 16, 0xFFFFFFFC, 0, 8, 4), (16, 16, 8, 0, 0xFFFFFFFC, 4),               # x + w wraps 2^32
                 (16, 16, 0, 0xFFFFFFFC, 4, 8),                                              # y + h wraps 2^32
                 (0, 16, 0, 0, 4, 4), (18, 16, 0, 0, 4, 4),                                  # no such texture
                 (16, 0, 0, 0, 4, 4), (16, 4, 0, 0, 4, 4), (16, 32, 0, 0, 4, 4)):            # no such block
        assert f(*args, 0, 1 << 20) == 0, args
    # the largest texture row and the last row a region can name
    assert f(0xFFFFFFFC, 16, 0xFFFFFFF8, 0xFFFFFFF8, 4, 4, (1 << 64) - 2, 1) == 0
    row = (0xFFFFFFFC // 4) * 16
    last = (0xFFFFFFF8 // 4) * row + (0xFFFFFFF8 // 4) * 16
    assert f(0xFFFFFFFC, 16, 0xFFFFFFF8, 0xFFFFFFF8, 4, 4, last, 1) == 1
    assert f(0xFFFFFFFC, 16, 0xFFFFFFF8, 0xFFFFFFF8, 4, 4, last - 1, 1) == 0
    assert f(0xFFFFFFFC, 16, 0xFFFFFFF8, 0xFFFFFFF8, 4, 4, last + 16, 1) == 0


def test_the_python_predicate(hap):
    assert hap.region_needs_bytes(16, 8, (4, 0, 4, 4), 8, 8) is True
    assert hap.region_needs_bytes(16, 8, (4, 0, 4, 4), 0, 8) is False


BAD_REGIONS = ((0, 0, 0, 4), (0, 0, 4, 0), (2, 0, 4, 4), (0, 0, 6, 4), (0, 2, 4, 4), (0, 0, 4, 6), (4, 0, 8, 4),
               (0, 4, 4, 8), (8, 0, 4, 4), (0, 8, 4, 4), (0xFFFFFFFC, 0, 8, 4), (0, 0xFFFFFFFC, 4, 8))


def test_they_refuse_before_touching_a_device(hap):
    """8 x 8 textures and frames: a missing context and every bad region, as the scaled calls' ABI test does it"""
    lib = hap._lib.lib
    bad = hap.HapResult.Bad_Arguments
    pic = (C.c_ubyte * 64)(*([0x5A] * 64))
    tex = (C.c_ubyte * 64)()
    for region in ((0, 0, 4, 4), (4, 4, 4, 4), (0, 0, 8, 8)) + BAD_REGIONS:
        assert lib.HapGpuDecompressRGBARegion(None, tex, 64, L.FMT_DXT5, None, 0, 8, 8, *region, pic, 16) == bad
        assert lib.HapGpuDecompressRGBARegion(None, None, 0, L.FMT_DXT5, None, 0, 8, 8, *region, None, 16) == bad
    assert bytes(pic) == b"\x5a" * 64
    frames = (C.c_void_p * 2)(C.addressof(tex), C.addressof(tex))
    lens = (C.c_ulong * 2)(64, 64)
    pics = (C.c_void_p * 2)(C.addressof(pic), C.addressof(pic))
    res = (C.c_uint * 2)(77, 77)
    for region in ((0, 0, 4, 4), (0, 0, 8, 8)) + BAD_REGIONS:
        assert lib.HapGpuDecodeFramesRGBARegion(None, 2, frames, lens, 1, pics, 8, 8, *region, 16, res, 0) == bad
        assert lib.HapGpuDecodeFramesRGBARegion(None, 2, None, None, 1, None, 8, 8, *region, 16, None, 0) == bad
    assert list(res) == [77, 77] and bytes(pic) == b"\x5a" * 64
    assert lib.HapGpuSkippedTextureBytes(None) == 0


def test_the_python_methods_exist(hap):
    want = {"decompress_rgba_region": ["texture", "texture_format", "width", "height", "region", "rgba", "alpha",
                                       "row_bytes"],
            "decode_frames_rgba_region": ["frames", "frame_bytes", "texture_count", "rgba_frames", "width", "height",
                                          "region", "row_bytes", "flags"],
            "skipped_texture_bytes": []}
    for name, params in want.items():
        sig = inspect.signature(getattr(hap.Context, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(hap.Context.decompress_rgba_region)
    assert [sig.parameters[p].default for p in ("rgba", "alpha", "row_bytes")] == [None, None, None]
    sig = inspect.signature(hap.Context.decode_frames_rgba_region)
    assert sig.parameters["row_bytes"].default is None and sig.parameters["flags"].default == 0
    assert list(inspect.signature(hap.region_needs_bytes).parameters) == ["width", "block_bytes", "region", "first_byte",
                                                                          "byte_count"]

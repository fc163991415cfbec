"""Prints digests of encoded frames (deterministic encoder): used to confirm that a kernel rewrite that is
meant to be output-neutral really leaves every byte of the compressed streams unchanged."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import hap_amd
from hap_amd import synth
import _data as D

ctx = hap_amd.Context(0)
h = hashlib.sha256()
for (w, hgt, fmts, chunks) in [(1920, 1080, [0x83F0], [1]), (1920, 1080, [0x83F3], [8]), (3840, 2160, [0x01], [24]),
                               (2048, 2048, [0x01, 0x8DBB], [16, 16])]:
    for lg in (10, 13, 16):
        ctx.set_fragment_log2(lg)
        for fr in range(2):
            img = synth.rgba_frame(w, hgt, fr, device="cuda")
            tb = [(w // 4) * (hgt // 4) * (8 if f in (0x83F0, 0x8DBB) else 16) for f in fmts]
            out = torch.zeros(hap_amd.HapMaxEncodedLength(tb, fmts, chunks) + 65536, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r, used, res = ctx.encode_frames_rgba([img], w, hgt, w * 4, fmts, [1] * len(fmts), chunks, [out], flags=1)
            assert r == 0
            b = out[: used[0]].cpu().numpy().tobytes()
            d = hashlib.sha256(b).hexdigest()[:16]
            h.update(b)
            print(w, hgt, [hex(f) for f in fmts], "F=2^%d" % lg, "frame", fr, used[0], d)
# byte streams with odd sizes (byte-granular path) and raw textures
ctx.set_fragment_log2(13)
for n, kind, fmt, ch in [(100001, "mixed", 0x83F3, 3), (65536 * 3 + 2, "runs", 0x8E8C, 1), (16 * 7919, "mixed", 0x8DBB, 7), (999, "zero", 0x83F0, 2)]:
    tex = D.stream_bytes(n, kind, seed=n)
    out = np.zeros(hap_amd.HapMaxEncodedLength([n], [fmt], [ch]) + 65536, dtype=np.uint8)
    r, used, res = ctx.encode_frames([[tex]], [fmt], [1], [ch], [out], flags=1)
    assert r == 0
    b = out[: used[0]].tobytes(); h.update(b)
    print("bytes", n, kind, hex(fmt), ch, used[0], hashlib.sha256(b).hexdigest()[:16])
# what a call decides before it looks at a frame (hap_encode_plan.h): frames from RGBA8 pictures at 1, 8 and 16 a call
# (placing off below 8 frames, on from there), with each flag that changes the plan; a tensor call and an NV12 call; a
# BC7 texture and an RGTC1 plane of 2 MiB
INDEX = hap_amd.ENCODE_FRAGMENT_INDEX


def digest_call(label, outs, r, used, res):
    assert r == 0 and all(x == 0 for x in res), (label, r, res)
    for o, u in zip(outs, used):
        h.update(o[:u].cpu().numpy().tobytes())
    print(label, list(used), hashlib.sha256(b"".join(o[:u].cpu().numpy().tobytes() for o, u in zip(outs, used))).hexdigest()[:16])


def buffers(n, w, hgt, fmts, chunks):
    tb = [(w // 4) * (hgt // 4) * (8 if f in (0x83F0, 0x8DBB) else 16) for f in fmts]
    cap = 2 * hap_amd.HapMaxEncodedLength(tb, fmts, chunks) + 65536
    return [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]


w, hgt = 1024, 512
pictures = [synth.rgba_frame(w, hgt, fr, device="cuda") for fr in range(16)]
torch.cuda.synchronize()
for fmts, chunks in [([0x01], [4]), ([0x83F3], [4]), ([0x83F0], [3]), ([0x01, 0x8DBB], [4, 2])]:
    for n in (1, 8, 16):
        for flags in (INDEX, INDEX | hap_amd.ENCODE_COARSE_MATCHES, INDEX | hap_amd.ENCODE_FINE_CHUNKS,
                      INDEX | hap_amd.ENCODE_SMALLER_FILES, INDEX | hap_amd.ENCODE_REFINE_ENDPOINTS, 0):
            outs = buffers(n, w, hgt, fmts, chunks)
            r, used, res = ctx.encode_frames_rgba(pictures[:n], w, hgt, w * 4, fmts, [1] * len(fmts), chunks, outs, flags=flags)
            digest_call("pictures %s x%d flags 0x%x" % ([hex(f) for f in fmts], n, flags), outs, r, used, res)
# tensors and NV12 pictures made of the same pictures
tensor = torch.stack([p[..., :3].permute(2, 0, 1) for p in pictures[:8]]).to(torch.float16).contiguous()
lumas = [p[..., 1].contiguous() for p in pictures[:8]]
chromas = [p[::2, ::2, :2].contiguous() for p in pictures[:8]]
torch.cuda.synchronize()
for fmts, flags in [([0x01], INDEX), ([0x83F0], INDEX | hap_amd.ENCODE_REFINE_ENDPOINTS)]:
    outs = buffers(8, w, hgt, fmts, [4])
    r, used, res = ctx.encode_frames_planes(tensor, w, hgt, fmts, [1], [4], outs, scale=[1.0] * 3, bias=[0.0] * 3, flags=flags)
    digest_call("tensors %s flags 0x%x" % (hex(fmts[0]), flags), outs, r, used, res)
    outs = buffers(8, w, hgt, fmts, [4])
    r, used, res = ctx.encode_frames_nv12(lumas, chromas, w, hgt, fmts, [1], [4], outs, flags=flags)
    digest_call("NV12 %s flags 0x%x" % (hex(fmts[0]), flags), outs, r, used, res)
# BC7 (position lanes, and the block compressor with COARSE_MATCHES) and an RGTC1 plane of 2 MiB (its [2, 6] layout)
for flags in (INDEX, INDEX | hap_amd.ENCODE_COARSE_MATCHES):
    outs = buffers(2, w, hgt, [0x8E8C], [4])
    r, used, res = ctx.encode_frames_rgba(pictures[:2], w, hgt, w * 4, [0x8E8C], [1], [4], outs, flags=flags | hap_amd.ENCODE_BPTC_BLOCKS)
    digest_call("pictures BC7 flags 0x%x" % flags, outs, r, used, res)
big = [synth.rgba_frame(2048, 2048, fr, device="cuda") for fr in range(8)]
torch.cuda.synchronize()
for n in (1, 8):
    outs = buffers(n, 2048, 2048, [0x8DBB], [8])
    r, used, res = ctx.encode_frames_rgba(big[:n], 2048, 2048, 2048 * 4, [0x8DBB], [1], [8], outs, flags=INDEX)
    digest_call("pictures RGTC1 2 MiB x%d" % n, outs, r, used, res)
print("TOTAL", h.hexdigest())

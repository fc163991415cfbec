"""GPU measurement of the BC7 -> RGBA8 kernel (hap_amd/csrc/bptc_decode.hip) on 8K (8192 x 4320) textures.

    python tools/bench_bptc_decode.py [--reps N] [--frames F]

Reports, per 8K texture -> picture in HBM (HapGpuDecompressRGBA): the kernel time (HIP events of the block_decode
profile class) and the call time (HapGpuTimerStart/Stop around the calls) for mode-6-only textures, mixed-mode
textures and, in the same run on the same geometry, the DXT5 kernel; then F Hap R frames -> pictures through
HapGpuDecodeFramesRGBA.  Roofline bytes: 16 read + 64 written per block (177 MB per 8K frame, as DXT5).

Mode-6 textures come from hap_amd.synth pictures through a minimal vectorised encoder (per-block min / max endpoints
with p-bits 0 / 1, nearest of the 16 weights along the endpoint line); mixed-mode textures are the generated blocks of
tests/_bptc.py (every mode, all partitions, random bits) tiled over the picture.  A block row of each texture is checked
against the CPU reference.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _bptc as B  # noqa: E402
import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

W, H = 8192, 4320
BX, BY = W // 4, H // 4
FMT_BC7, FMT_DXT5 = 0x8E8C, 0x83F3
HBM_PEAK_GBS = 8000.0


def mode6_encode(rgba):
    """uint8 [H, W, 4] cuda tensor -> BC7 mode-6 blocks (uint8 [BY * BX * 16])."""
    h, w, _ = rgba.shape
    blk = rgba.view(h // 4, 4, w // 4, 4, 4).permute(0, 2, 1, 3, 4).reshape(-1, 16, 4).to(torch.int64)
    lo = blk.min(1).values & ~1                           # endpoint 0: p-bit 0
    hi = blk.max(1).values | 1                            # endpoint 1: p-bit 1
    d = (hi - lo).unsqueeze(1)
    num = ((blk - lo.unsqueeze(1)) * d).sum(-1)
    den = (d * d).sum(-1).clamp(min=1)
    idx = torch.clamp((num * 15 + den // 2) // den, 0, 15)  # nearest of 16 evenly spaced weights along the line
    swap = idx[:, 0] >= 8                                   # texel 0's index has 3 bits: swap the endpoints
    lo, hi = torch.where(swap.unsqueeze(1), hi, lo), torch.where(swap.unsqueeze(1), lo, hi)
    idx = torch.where(swap.unsqueeze(1), 15 - idx, idx)
    p0, p1 = lo[:, 0] & 1, hi[:, 0] & 1
    q0, q1 = lo >> 1, hi >> 1
    low = torch.full_like(p0, 1 << 6)
    for c in range(4):
        low |= q0[:, c] << (7 + 14 * c)
        low |= q1[:, c] << (14 + 14 * c)
    low |= p0 << 63
    high = p1 | (idx[:, 0] << 1)
    for t in range(1, 16):
        high |= idx[:, t] << (4 * t)
    return torch.stack([low, high], 1).contiguous().view(torch.uint8).reshape(-1)


def mixed_texture():
    sets = B.block_sets()
    pool = sets["mixed"] + B.random_blocks(4096, 0xB7)
    pool = torch.frombuffer(bytearray(pool), dtype=torch.uint8).view(-1, 16).cuda()
    sel = (torch.arange(BX * BY, device="cuda", dtype=torch.int64) * 7919) % pool.shape[0]
    return pool[sel].reshape(-1).contiguous()


def check_row(tex, out):
    """First block row of the picture against the CPU reference."""
    t = tex[: BX * 16].cpu().numpy().tobytes()
    want = B.decode(t, W, 4)
    got = out[: W * 4 * 4].cpu().numpy().reshape(4, W, 4)
    return bool(np.array_equal(got, want))


def time_decompress(ctx, tex, fmt, out, reps):
    for _ in range(3):
        assert ctx.decompress_rgba(tex, fmt, W, H, rgba=out)[0] == 0
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.timer_start()
    for _ in range(reps):
        assert ctx.decompress_rgba(tex, fmt, W, H, rgba=out)[0] == 0
    call_ms = ctx.timer_stop()
    n, ms = ctx.collect_profile()["block_decode"]
    ctx.set_profiling(False)
    kernel_us = ms / n * 1e3
    gbs = BX * BY * 80 / (kernel_us * 1e-6) / 1e9
    return {"kernel_us": round(kernel_us, 2), "call_us": round(call_ms / reps * 1e3, 2), "launches": n,
            "GBps": round(gbs, 0), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bptc_decode.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"geometry": [W, H], "bytes_per_frame": BX * BY * 80}
    out = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
    pic = synth.rgba_frame(W, H, 0, device="cuda")
    m6 = mode6_encode(pic)
    mixed = mixed_texture()
    dxt5 = torch.empty(BX * BY * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compress_rgba(pic, W, H, W * 4, FMT_DXT5, dxt5)[0] == 0
    # the three kernels alternated twice: the spread between the rounds is the noise
    for rnd in range(2):
        for name, tex, fmt in (("bc7_mode6", m6, FMT_BC7), ("bc7_mixed", mixed, FMT_BC7), ("dxt5", dxt5, FMT_DXT5)):
            res.setdefault(name, []).append(time_decompress(ctx, tex, fmt, out, args.reps))
            if rnd == 0 and fmt == FMT_BC7:
                res[name + "_row_bit_exact"] = check_row(tex, out)
                if name == "bc7_mode6":
                    err = (out.view(H, W, 4).to(torch.float32) - pic.to(torch.float32)).pow(2).mean().item()
                    res["bc7_mode6_psnr"] = round(10 * np.log10(255.0 ** 2 / max(err, 1e-9)), 2)
    best = {k: min(r["kernel_us"] for r in res[k]) for k in ("bc7_mode6", "bc7_mixed", "dxt5")}
    res["mixed_over_dxt5"] = round(best["bc7_mixed"] / best["dxt5"], 3)
    res["mixed_over_mode6"] = round(best["bc7_mixed"] / best["bc7_mode6"], 3)
    del out
    # F Hap R frames -> pictures in one call
    nf = args.frames
    tex_bytes = BX * BY * 16
    cap = hap_amd.HapMaxEncodedLength([tex_bytes], [FMT_BC7], [16])
    frames = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(nf)]
    used = []
    for i in range(nf):
        t = mode6_encode(synth.rgba_frame(W, H, i, device="cuda"))
        r, u, rr = ctx.encode_frames([[t]], [FMT_BC7], [1], [16], [frames[i]], flags=hap_amd.ENCODE_FRAGMENT_INDEX)
        assert r == 0 and rr == [0], (r, rr)
        used.append(u[0])
    del t
    pics = [torch.empty(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(nf)]
    torch.cuda.synchronize()
    flag = hap_amd.DECODE_BPTC_PICTURES
    for _ in range(2):
        r, rr = ctx.decode_frames_rgba(frames, used, 1, pics, W, H, flags=flag)
        assert r == 0 and rr == [0] * nf, (r, rr)
    calls = []
    for _ in range(5):
        ctx.timer_start()
        r, rr = ctx.decode_frames_rgba(frames, used, 1, pics, W, H, flags=flag)
        calls.append(ctx.timer_stop())
        assert r == 0
    res["frames_rgba"] = {"frames": nf, "ratio": round(sum(used) / (nf * tex_bytes), 3),
                          "call_ms_best": round(min(calls), 3), "call_ms_all": [round(c, 3) for c in calls]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

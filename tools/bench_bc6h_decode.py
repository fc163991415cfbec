"""GPU measurement of the BC6H -> RGBA16F kernel (hap_amd/csrc/bc6h_decode.hip) on 8K (8192 x 4320) textures.

    python tools/bench_bc6h_decode.py [--reps N] [--frames F]

Reports, per 8K texture -> picture in HBM (HapGpuDecompressRGBAHalf): the kernel time (HIP events of the
block_decode profile class) and the call time (HapGpuTimerStart/Stop around the calls) for a one-mode texture (mode
0x03 blocks), a mixed-mode BC6U texture and a mixed-mode BC6S texture, and, in the same run on the same geometry,
the BC7 kernel on mixed-mode blocks; then F Hap HDR frames -> pictures through HapGpuDecodeFramesRGBAHalf.
Algorithmic bytes: 16 read + 128 written per block (318.5 MB per 8K picture).

Mixed-mode textures are the generated blocks of tests/_bc6h.py (every mode, all partitions, reserved blocks) and random
blocks, tiled over the picture.  A block row of each texture is checked against the CPU reference.
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

import _bc6h as B  # noqa: E402
import _bptc  # noqa: E402
import hap_amd  # noqa: E402

W, H = 8192, 4320
BX, BY = W // 4, H // 4
FMT_BC6U, FMT_BC6S, FMT_BC7 = 0x8E8F, 0x8E8E, 0x8E8C
BYTES_PER_BLOCK = {FMT_BC6U: 144, FMT_BC6S: 144, FMT_BC7: 80}
HBM_PEAK_GBS = 8000.0


def tiled(pool):
    pool = torch.frombuffer(bytearray(pool), dtype=torch.uint8).view(-1, 16).cuda()
    sel = (torch.arange(BX * BY, device="cuda", dtype=torch.int64) * 7919) % pool.shape[0]
    return pool[sel].reshape(-1).contiguous()


def one_mode_texture():
    """Mode 0x03 blocks (one region, raw 10-bit endpoints) of the generator, band-biased and random."""
    rng = B.SplitMix64(0x03)
    mode = B.MODE_OF_VALUE[0x03]
    return tiled(b"".join(B.make_block(mode, rng, band=i % 2 == 0) for i in range(4096)))


def mixed_texture(signed):
    sets = B.block_sets()
    return tiled(sets["mixed_s" if signed else "mixed_u"] + B.random_blocks(4096, 0xB6 + signed))


def check_row(tex, out, fmt):
    """First block row of the picture against the CPU reference."""
    t = tex[: BX * 16].cpu().numpy().tobytes()
    if fmt == FMT_BC7:
        return bool(np.array_equal(out[: W * 4 * 4].cpu().numpy().reshape(4, W, 4), _bptc.decode(t, W, 4)))
    got = out[: W * 8 * 4].cpu().numpy().view(np.uint16).reshape(4, W, 4)
    return bool(np.array_equal(got, B.decode(t, W, 4, fmt == FMT_BC6S)))


def time_decompress(ctx, tex, fmt, out, reps):
    if fmt == FMT_BC7:
        def call():
            return ctx.decompress_rgba(tex, fmt, W, H, rgba=out)[0]
    else:
        def call():
            return ctx.decompress_rgba_half(tex, fmt, W, H, out=out)[0]
    for _ in range(3):
        assert call() == 0
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.timer_start()
    for _ in range(reps):
        assert call() == 0
    call_ms = ctx.timer_stop()
    n, ms = ctx.collect_profile()["block_decode"]
    ctx.set_profiling(False)
    kernel_us = ms / n * 1e3
    gbs = BX * BY * BYTES_PER_BLOCK[fmt] / (kernel_us * 1e-6) / 1e9
    return {"kernel_us": round(kernel_us, 2), "call_us": round(call_ms / reps * 1e3, 2), "launches": n,
            "GBps": round(gbs, 0), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bc6h_decode.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"geometry": [W, H], "bytes_per_frame": BX * BY * 144}
    out = torch.empty(W * H * 8, dtype=torch.uint8, device="cuda")
    textures = (("bc6u_mode03", one_mode_texture(), FMT_BC6U), ("bc6u_mixed", mixed_texture(False), FMT_BC6U),
                ("bc6s_mixed", mixed_texture(True), FMT_BC6S), ("bc7_mixed", tiled(_bptc.block_sets()["mixed"] +
                                                                                    _bptc.random_blocks(4096, 0xB7)), FMT_BC7))
    torch.cuda.synchronize()
    # the kernels alternated twice: the spread between the rounds is the noise
    for rnd in range(2):
        for name, tex, fmt in textures:
            res.setdefault(name, []).append(time_decompress(ctx, tex, fmt, out, args.reps))
            if rnd == 0:
                res[name + "_row_bit_exact"] = check_row(tex, out, fmt)
    best = {name: min(r["kernel_us"] for r in res[name]) for name, _t, _f in textures}
    res["bc6u_mixed_over_mode03"] = round(best["bc6u_mixed"] / best["bc6u_mode03"], 3)
    res["bc6s_mixed_over_bc7_mixed"] = round(best["bc6s_mixed"] / best["bc7_mixed"], 3)
    del out
    # F Hap HDR frames -> pictures in one call
    nf = args.frames
    tex_bytes = BX * BY * 16
    cap = hap_amd.HapMaxEncodedLength([tex_bytes], [FMT_BC6U], [16])
    frames = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(nf)]
    used = []
    src = textures[1][1]
    for i in range(nf):
        r, u, rr = ctx.encode_frames([[src]], [FMT_BC6U], [1], [16], [frames[i]], flags=hap_amd.ENCODE_FRAGMENT_INDEX)
        assert r == 0 and rr == [0], (r, rr)
        used.append(u[0])
    pics = [torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(nf)]
    torch.cuda.synchronize()
    for _ in range(2):
        r, rr = ctx.decode_frames_rgba_half(frames, used, pics, W, H)
        assert r == 0 and rr == [0] * nf, (r, rr)
    calls = []
    for _ in range(5):
        ctx.timer_start()
        r, rr = ctx.decode_frames_rgba_half(frames, used, pics, W, H)
        calls.append(ctx.timer_stop())
        assert r == 0
    res["frames_rgba_half"] = {"frames": nf, "ratio": round(sum(used) / (nf * tex_bytes), 3),
                               "call_ms_best": round(min(calls), 3), "call_ms_all": [round(c, 3) for c in calls],
                               "row_bit_exact": check_row(src, pics[-1].view(torch.uint8).reshape(-1), FMT_BC6U)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""GPU measurement of the RGBA16F -> BC6H encoder (hap_amd/csrc/bc6h_encode.hip) on 8K (8192 x 4320) half pictures.
    python tools/bench_bc6h_encode.py [--reps N] [--frames F]
Reports, for a synthetic HDR picture (hap_amd.synth pictures scaled to 0 .. 16 with a dark floor, half floats) in the
unsigned and the signed format: the kernel time per picture (HIP events of the block_encode profile class) and the call
time of HapGpuCompressRGBAHalf (device picture to device texture); for scale, in the same run on same-sized pictures,
the BC7 encoder on the opaque RGBA8 picture and the BC6H decoder on the texture just made; then F pictures -> Hap HDR
frames per HapGpuEncodeFramesRGBAHalf call (default second stage and HAPGPU_ENCODE_COARSE_MATCHES) with the compressed
size over the texture size.  One block row of each texture is checked against tests/_bc6h_encode.py.
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

import _bc6h_encode as E  # noqa: E402
import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

W, H = 8192, 4320
BX, BY = W // 4, H // 4
FMT_BC7, FMT_BC6U, FMT_BC6S = 0x8E8C, 0x8E8F, 0x8E8E


def half_picture(i):
    """uint8 synth picture -> float16 [H, W, 4] on the GPU: (v / 255)^2 * 16 + 1 / 256, alpha 1"""
    p = synth.rgba_frame(W, H, i, device="cuda").view(H, W, 4).to(torch.float32) / 255.0
    p = (p * p * 16.0 + 1.0 / 256.0).to(torch.float16)
    p[..., 3] = 1.0
    return p.contiguous()


def timed(ctx, call, cls, reps):
    for _ in range(2):
        assert call() == 0
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.timer_start()
    for _ in range(reps):
        assert call() == 0
    call_ms = ctx.timer_stop()
    n, ms = ctx.collect_profile()[cls]
    ctx.set_profiling(False)
    return {"kernel_us": round(ms / n * 1e3, 1), "call_us": round(call_ms / reps * 1e3, 1), "launches": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bc6h_encode.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"geometry": [W, H], "blocks": BX * BY}
    pic = half_picture(0)
    opaque = synth.rgba_frame(W, H, 0, device="cuda").clone()
    opaque.view(H, W, 4)[..., 3] = 255
    out = torch.empty(BX * BY * 16, dtype=torch.uint8, device="cuda")
    back = torch.empty(H * W * 4, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    for rnd in range(2):
        for name, fmt in (("bc6h_unsigned", FMT_BC6U), ("bc6h_signed", FMT_BC6S)):
            res.setdefault(name, []).append(
                timed(ctx, lambda: ctx.compress_rgba_half(pic, W, H, W * 8, fmt, out)[0], "block_encode", args.reps))
            if rnd == 0:
                want = E.encode(pic[:4].cpu().numpy().view(np.uint16), fmt == FMT_BC6S)
                res[name + "_row_bit_exact"] = out[: BX * 16].cpu().numpy().tobytes() == want
            res.setdefault(name + "_decode", []).append(
                timed(ctx, lambda: ctx.decompress_rgba_half(out, fmt, W, H, out=back)[0], "block_decode", args.reps))
        res.setdefault("bc7_opaque", []).append(
            timed(ctx, lambda: ctx.compress_rgba(opaque, W, H, W * 4, FMT_BC7, out, flags=hap_amd.ENCODE_BPTC_BLOCKS)[0],
                  "block_encode", args.reps))
    best = {k: min(r["kernel_us"] for r in v) for k, v in res.items() if isinstance(v, list) and k != "geometry"}
    for name in ("bc6h_unsigned", "bc6h_signed"):
        res[name + "_over_bc7"] = round(best[name] / best["bc7_opaque"], 2)
    del out, back, opaque
    nf = args.frames
    tex_bytes = BX * BY * 16
    cap = hap_amd.HapMaxEncodedLength([tex_bytes], [FMT_BC6U], [16])
    frames = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(nf)]
    pics = [pic] + [half_picture(i) for i in range(1, nf)]
    torch.cuda.synchronize()
    for name, extra in (("frames_default", 0), ("frames_coarse", hap_amd.ENCODE_COARSE_MATCHES)):
        flags = extra | hap_amd.ENCODE_FRAGMENT_INDEX
        r, used, rr = ctx.encode_frames_rgba_half(pics, W, H, W * 8, FMT_BC6U, 1, 16, frames, flags=flags)
        assert r == 0 and rr == [0] * nf, (r, rr)
        ctx.timer_start()
        for _ in range(2):
            r, used, rr = ctx.encode_frames_rgba_half(pics, W, H, W * 8, FMT_BC6U, 1, 16, frames, flags=flags)
            assert r == 0
        ms = ctx.timer_stop() / 2
        res[name] = {"frames": nf, "ms_per_call": round(ms, 2), "ratio": round(sum(used) / (nf * tex_bytes), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

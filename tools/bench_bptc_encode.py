"""GPU measurement of the RGBA8 -> BC7 encoder (hap_amd/csrc/bptc_encode.hip) on 8K (8192 x 4320) pictures.
    python tools/bench_bptc_encode.py [--reps N] [--frames F]
Reports, for hap_amd.synth pictures as they are (with alpha) and with alpha forced to 255 (opaque): the kernel time per
picture (HIP events of the block_encode profile class) and the call time of HapGpuCompressRGBAFlags (device picture to
device texture); the DXT5 encoder on the same pictures in the same run for scale; then F pictures -> Hap R frames per
HapGpuEncodeFramesRGBA call (HAPGPU_ENCODE_BPTC_BLOCKS, default second stage and HAPGPU_ENCODE_COARSE_MATCHES) with the
compressed size over the texture size.  One block row of each texture is checked against tests/_bc7_encode.py.
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

import _bc7_encode as E  # noqa: E402
import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

W, H = 8192, 4320
BX, BY = W // 4, H // 4
FMT_BC7, FMT_DXT5 = 0x8E8C, 0x83F3


def time_compress(ctx, pic, fmt, flags, out, reps):
    for _ in range(2):
        assert ctx.compress_rgba(pic, W, H, W * 4, fmt, out, flags=flags)[0] == 0
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.timer_start()
    for _ in range(reps):
        assert ctx.compress_rgba(pic, W, H, W * 4, fmt, out, flags=flags)[0] == 0
    call_ms = ctx.timer_stop()
    n, ms = ctx.collect_profile()["block_encode"]
    ctx.set_profiling(False)
    return {"kernel_us": round(ms / n * 1e3, 1), "call_us": round(call_ms / reps * 1e3, 1), "launches": n}


def check_row(pic, out):
    """the first block row against the reference encoder"""
    want = E.encode(pic[:4].cpu().numpy())
    return out[: BX * 16].cpu().numpy().tobytes() == want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bptc_encode.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"geometry": [W, H], "blocks": BX * BY}
    alpha = synth.rgba_frame(W, H, 0, device="cuda")
    opaque = alpha.clone()
    opaque.view(H, W, 4)[..., 3] = 255
    out = torch.empty(BX * BY * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bptc = hap_amd.ENCODE_BPTC_BLOCKS
    for rnd in range(2):
        for name, pic, fmt, flags in (("bc7_alpha", alpha, FMT_BC7, bptc), ("bc7_opaque", opaque, FMT_BC7, bptc),
                                      ("dxt5", alpha, FMT_DXT5, 0)):
            res.setdefault(name, []).append(time_compress(ctx, pic, fmt, flags, out, args.reps))
            if rnd == 0 and fmt == FMT_BC7:
                res[name + "_row_bit_exact"] = check_row(pic.view(H, W, 4), out)
    for name in ("bc7_alpha", "bc7_opaque"):
        res[name + "_over_dxt5"] = round(min(r["kernel_us"] for r in res[name]) / min(r["kernel_us"] for r in res["dxt5"]), 2)
    del out
    nf = args.frames
    tex_bytes = BX * BY * 16
    cap = hap_amd.HapMaxEncodedLength([tex_bytes], [FMT_BC7], [16])
    frames = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(nf)]
    pics = [synth.rgba_frame(W, H, i, device="cuda") for i in range(nf)]
    torch.cuda.synchronize()
    for name, extra in (("frames_default", 0), ("frames_coarse", hap_amd.ENCODE_COARSE_MATCHES)):
        flags = bptc | extra | hap_amd.ENCODE_FRAGMENT_INDEX
        r, used, rr = ctx.encode_frames_rgba(pics, W, H, W * 4, [FMT_BC7], [1], [16], frames, flags=flags)
        assert r == 0 and rr == [0] * nf, (r, rr)
        ctx.timer_start()
        for _ in range(2):
            r, used, rr = ctx.encode_frames_rgba(pics, W, H, W * 4, [FMT_BC7], [1], [16], frames, flags=flags)
            assert r == 0
        ms = ctx.timer_stop() / 2
        res[name] = {"frames": nf, "ms_per_call": round(ms, 2), "ratio": round(sum(used) / (nf * tex_bytes), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

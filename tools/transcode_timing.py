"""GPU timing of the transcode call (HapGpuTranscodeFrames) against the two calls it replaces, HapGpuDecodeFramesRGBA[Scaled]
followed by HapGpuEncodeFramesRGBA.

    python tools/transcode_timing.py [--reps N] [--out FILE] [--shrink K]

Cases, frames and pictures in HBM, sources made here from hap_amd.synth pictures (hap.h sections only, 16 chunks a texture):

  hap_q_8k_x60_to_hap_q_alpha   60 Hap Q frames of 7680 x 4320 -> Hap Q Alpha at the same size with the fragment table
                                (HAPGPU_ENCODE_FRAGMENT_INDEX): every frame is encoded anew, none passes through
  hap_q_8k_x60_to_quarter_hap   the same frames -> quarter-size Hap (DXT1) proxies
  hap_q_alpha_16k_x4_to_half    4 Hap Q Alpha frames of 15360 x 8640 -> half-size Hap Q Alpha

Per case and route, the median of N calls after warm-up by the context's own timer (HIP events on its stream around the
whole route, both calls of the two-call route in one bracket), the kernel time by profile class (taken in separate calls;
the transcode kernel counts as block_encode), and the bytes of RGBA pictures the two-call route holds and the transcode
call does not.  The frames of the two routes are compared byte for byte.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

FMT_DXT1, FMT_YCOCG, FMT_RGTC1 = 0x83F0, 0x01, 0x8DBB
BLOCK_BYTES = {FMT_DXT1: 8, FMT_YCOCG: 16, FMT_RGTC1: 8}
# name, width, height, frames, source formats, scale_log2, destination formats, encode flags
CASES = (("hap_q_8k_x60_to_hap_q_alpha", 7680, 4320, 60, (FMT_YCOCG,), 0, (FMT_YCOCG, FMT_RGTC1), "index"),
         ("hap_q_8k_x60_to_quarter_hap", 7680, 4320, 60, (FMT_YCOCG,), 2, (FMT_DXT1,), ""),
         ("hap_q_alpha_16k_x4_to_half", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1), 1, (FMT_YCOCG, FMT_RGTC1), ""))
CHUNKS = 16


def bound(w, h, fmts):
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    return hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))


def make_frames(ctx, w, h, count, fmts):
    cap = bound(w, h, fmts)
    distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(min(count, 4))]
    frames, used = [], []
    for first in range(0, count, 4):
        n = min(4, count - first)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        r, u, res = ctx.encode_frames_rgba([distinct[(first + i) % len(distinct)] for i in range(n)], w, h, w * 4, list(fmts),
                                           [1] * len(fmts), [CHUNKS] * len(fmts), bufs)
        assert r == 0 and res == [0] * n, (r, res)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
    del distinct
    torch.cuda.empty_cache()
    return frames, used


def measure(ctx, call, reps):
    """median ms of the route by the context's timer, median kernel ms per profile class"""
    for _ in range(2):
        call()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        times.append(ctx.timer_stop())
    kernel = {c: [] for c in hap_amd.KERNEL_CLASSES}
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        prof = ctx.collect_profile()
        for c in hap_amd.KERNEL_CLASSES:
            kernel[c].append(prof[c][1])
    ctx.set_profiling(False)
    out = {"call_ms": round(statistics.median(times), 3)}
    out["kernels_ms"] = {c: round(statistics.median(v), 4) for c, v in kernel.items() if statistics.median(v) > 0}
    out["kernels_total_ms"] = round(sum(out["kernels_ms"].values()), 4)
    return out


def one_case(ctx, w, h, count, src, s, dst, flag, reps):
    flags = hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0
    ow, oh = w >> s, h >> s
    frames, used = make_frames(ctx, w, h, count, src)
    cap = bound(ow, oh, dst) + (1 << 20)
    n_dst = len(dst)
    args = (list(dst), [1] * n_dst, [CHUNKS] * n_dst)
    outs = {route: [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)] for route in ("transcode", "two_call")}
    pics = [torch.zeros(ow * oh * 4, dtype=torch.uint8, device="cuda") for _ in range(count)]
    torch.cuda.synchronize()
    sizes = {}

    def transcode():
        r, u, res = ctx.transcode_frames(frames, used, len(src), w, h, s, *args, outs["transcode"], encode_flags=flags)
        assert r == 0 and not any(res), (r, res)
        sizes["transcode"] = u

    def two_call():
        if s:
            r, res = ctx.decode_frames_rgba_scaled(frames, used, len(src), pics, w, h, s)
        else:
            r, res = ctx.decode_frames_rgba(frames, used, len(src), pics, w, h)
        assert r == 0 and not any(res), (r, res)
        r, u, res = ctx.encode_frames_rgba(pics, ow, oh, ow * 4, *args, outs["two_call"], flags=flags)
        assert r == 0 and not any(res), (r, res)
        sizes["two_call"] = u

    blocks_src, blocks_dst = (w // 4) * (h // 4), (ow // 4) * (oh // 4)
    out = {"source_geometry": [w, h], "frames": count, "scale_log2": s, "source_formats": list(src),
           "destination_formats": list(dst), "encode_flags": flag or "none", "source_frame_bytes_per_step": sum(used),
           "source_texture_bytes_per_step": count * blocks_src * sum(BLOCK_BYTES[f] for f in src),
           "destination_texture_bytes_per_step": count * blocks_dst * sum(BLOCK_BYTES[f] for f in dst),
           "picture_bytes_the_two_calls_hold": count * ow * oh * 4}
    out["transcode"] = measure(ctx, transcode, reps)
    out["two_call"] = measure(ctx, two_call, reps)
    out["destination_frame_bytes_per_step"] = sum(sizes["transcode"])
    out["frames_equal_byte_for_byte"] = bool(sizes["transcode"] == sizes["two_call"] and all(
        torch.equal(a[:u], b[:u]) for a, b, u in zip(outs["transcode"], outs["two_call"], sizes["transcode"])))
    out["call_over_two_call"] = round(out["transcode"]["call_ms"] / out["two_call"]["call_ms"], 3)
    out["kernels_over_two_call"] = round(out["transcode"]["kernels_total_ms"] / out["two_call"]["kernels_total_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "transcode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps}
    for name, w, h, count, src, s, dst, flag in CASES:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        res[name] = one_case(ctx, w, h, count, src, s, dst, flag, args.reps)
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

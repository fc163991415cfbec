"""GPU measurement of the half- and quarter-size picture decoders (bc_decode.hip's scaled kernels) against the road the
library offered before them: the full-size decode followed by a box filter.

    python tools/bench_scaled_decode.py [--reps N] [--out FILE]

Two workloads, frames and pictures in HBM: 60 Hap Q frames of 7680 x 4320 and 4 Hap Q Alpha frames of 15360 x 8640 (made
here from hap_amd.synth pictures by HapGpuEncodeFramesRGBA).  Per workload, in one process, alternated over two rounds
(the spread between rounds is the noise), medians of N calls each:

  full      HapGpuDecodeFramesRGBA: the pictures at full size
  long_way  the same call, then every picture box-filtered by torch.nn.functional.avg_pool2d (uint8 -> float sums, which
            are exact, -> the rounded mean as uint8, channels first): what a client had to do for a small picture
  half      HapGpuDecodeFramesRGBAScaled, scaleLog2 1
  quarter   HapGpuDecodeFramesRGBAScaled, scaleLog2 2

call_ms is a host clock around the call and a device synchronise; block_decode_ms the HIP-event time of the block_decode
profile class per call (taken in separate calls: events around the launches serialise them); bytes_per_block what the
block-decode stage must move (Hap Q: 16 read + 64 / 16 / 4 written; Hap Q Alpha 8 more read) and GBps that over the
kernel time.  The scaled pictures of the first frame are compared with the box filter of its full-size picture.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

FMT_YCOCG, FMT_RGTC1 = 0x01, 0x8DBB
HBM_PEAK_GBS = 8000.0
WORKLOADS = (("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,)), ("hap_q_alpha_16k_x4", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1)))


def box(picture, w, h, s):
    """[h * w * 4] uint8 -> [4, h >> s, w >> s] uint8: (sum + half) >> 2s per channel, the sums exact in float32"""
    k = 1 << s
    x = picture.view(h, w, 4).permute(2, 0, 1).unsqueeze(0).float()
    sums = F.avg_pool2d(x, k, divisor_override=1)
    return ((sums + (k * k // 2)) * (1.0 / (k * k))).floor_().to(torch.uint8).squeeze(0)


def make_frames(ctx, w, h, count, fmts):
    blocks = (w // 4) * (h // 4)
    sizes = [blocks * (16 if f == FMT_YCOCG else 8) for f in fmts]
    chunks = [16] * len(fmts)
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), chunks)
    distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(min(count, 4))]
    frames, used = [], []
    for first in range(0, count, 4):
        n = min(4, count - first)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        r, u, res = ctx.encode_frames_rgba([distinct[(first + i) % len(distinct)] for i in range(n)], w, h, w * 4, list(fmts),
                                           [1] * len(fmts), chunks, bufs, flags=hap_amd.ENCODE_FRAGMENT_INDEX)
        assert r == 0 and res == [0] * n, (r, res)
        # (keep the frames' bytes only)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
    del distinct
    torch.cuda.empty_cache()
    return frames, used


def measure(ctx, call, reps):
    """(median call ms by the host clock, median block_decode ms per call by HIP events, launches per call)"""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    kernel, launches = [], 0
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        launches, ms = ctx.collect_profile()["block_decode"]
        kernel.append(ms)
    ctx.set_profiling(False)
    return statistics.median(times), (statistics.median(kernel) if launches else None), launches


def one_workload(ctx, name, w, h, count, fmts, reps):
    blocks = (w // 4) * (h // 4)
    frames, used = make_frames(ctx, w, h, count, fmts)
    tc = len(fmts)
    full = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(count)]
    small = {s: [torch.zeros((w >> s) * (h >> s) * 4, dtype=torch.uint8, device="cuda") for _ in range(count)] for s in (1, 2)}
    torch.cuda.synchronize()

    def ok(r):
        assert r[0] == 0 and not any(r[1]), r

    def full_size():
        ok(ctx.decode_frames_rgba(frames, used, tc, full, w, h))

    def long_way(s):
        full_size()
        for p in full:
            box(p, w, h, s)

    def scaled(s):
        ok(ctx.decode_frames_rgba_scaled(frames, used, tc, small[s], w, h, s))

    read = 16 + (8 if tc == 2 else 0)
    legs = (("full", full_size, read + 64), ("long_way_half", lambda: long_way(1), None), ("long_way_quarter", lambda: long_way(2), None),
            ("half", lambda: scaled(1), read + 16), ("quarter", lambda: scaled(2), read + 4))
    res = {"geometry": [w, h], "frames": count, "textures_per_frame": tc, "blocks_per_frame": blocks,
           "frame_bytes_over_texture_bytes": round(sum(used) / (count * blocks * (16 + (8 if tc == 2 else 0))), 3)}
    for _rnd in range(2):
        for leg, call, bpb in legs:
            call_ms, kernel_ms, launches = measure(ctx, call, reps)
            out = {"call_ms": round(call_ms, 3), "block_decode_ms": round(kernel_ms, 4) if kernel_ms is not None else None,
                   "launches": launches}
            if bpb and kernel_ms:
                gbs = count * blocks * bpb / (kernel_ms * 1e-3) / 1e9
                out.update({"bytes_per_block": bpb, "GBps": round(gbs, 0), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)})
            res.setdefault(leg, []).append(out)
    for s, leg in ((1, "half"), (2, "quarter")):
        want = box(full[0], w, h, s).permute(1, 2, 0).contiguous().view(-1)
        res[leg + "_equals_box_of_full_size"] = bool(torch.equal(small[s][0], want))
        best = lambda k, f: min(r[f] for r in res[k] if r[f] is not None)      # noqa: E731
        res[leg + "_call_over_long_way"] = round(best(leg, "call_ms") / best("long_way_" + leg, "call_ms"), 3)
        res[leg + "_kernel_over_full_kernel"] = round(best(leg, "block_decode_ms") / best("full", "block_decode_ms"), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scaled_decode.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"hbm_peak_GBps": HBM_PEAK_GBS, "reps": args.reps}
    for name, w, h, count, fmts in WORKLOADS:
        w, h = w // args.shrink // 4 * 4, h // args.shrink // 4 * 4
        res[name] = one_workload(ctx, name, w, h, count, fmts, args.reps)
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

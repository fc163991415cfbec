"""GPU cost and gain of HAPGPU_ENCODE_REFINE_ENDPOINTS: HapGpuEncodeFramesRGBA with the flag against the same call
without it, which is the code path the encoder had before the flag existed.

    python tools/refine_endpoints_timing.py [--reps N] [--out FILE] [--shrink K] [--unflagged-only]

Workloads, pictures and output buffers in HBM, pictures from hap_amd.synth (four distinct ones, repeated), Snappy,
16 chunks a texture:

  hap_4k_x60, hap_alpha_4k_x60          60 pictures of 3840 x 2160 to Hap (RGB_DXT1) and to Hap Alpha (RGBA_DXT5)
  hap_1080p_x60, hap_alpha_1080p_x60    60 pictures of 1920 x 1080
  ..._table                             the same with the fragment table (ENCODE_FRAGMENT_INDEX)

Per workload, for the call without the flag ("default") and with it ("refined"):

  call_ms            [median, min, max] of N calls after warm-up between HIP events (the call ends with the host waiting)
  block_encode_ms    the block-encode kernels' own time in the call, by profile class, median (for Hap Alpha without the
                     flag 0: those blocks are made inside the fused compress kernel)
  frame_bytes        the 60 frames together
  psnr_db            per channel R, G, B (and A for Hap Alpha), and R, G and B together, from HapGpuMeasureFrames against the source pictures
  sse                per channel, the sums behind them

and refined_over_default for the call, bytes_ratio, psnr_gain_db (R, G and B together).  --unflagged-only leaves the
flagged half out: with HAP_AMD_LIBRARY pointing at a build of another commit it times that commit's encoder with the same
script.  Prints one JSON line.
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

FMT_DXT1, FMT_DXT5 = 0x83F0, 0x83F3
BLOCK_BYTES = {FMT_DXT1: 8, FMT_DXT5: 16}
REFINE = 0x20                      # hap_amd.ENCODE_REFINE_ENDPOINTS (by value: a build of an earlier commit has no such name)
CHUNKS = 16
GEOMETRIES = (("4k", 3840, 2160), ("1080p", 1920, 1080))
FLAVOURS = (("hap", FMT_DXT1), ("hap_alpha", FMT_DXT5))
FRAMES = 60


def timed_ms(call, reps):
    """[median, min, max] ms between HIP events around `call`"""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return [round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)]


def block_encode_ms(ctx, call, reps):
    times = []
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        times.append(ctx.collect_profile()["block_encode"][1])
    ctx.set_profiling(False)
    return round(statistics.median(times), 4)


def one_side(ctx, pictures, bufs, w, h, fmt, flags, reps):
    n = len(pictures)
    last = {}

    def call():
        r, used, res = ctx.encode_frames_rgba(pictures, w, h, w * 4, [fmt], [1], [CHUNKS], bufs, flags=flags)
        assert r == 0 and not any(res), (r, res)
        last["used"] = list(used)

    out = {"call_ms": timed_ms(call, reps), "block_encode_ms": block_encode_ms(ctx, call, reps)}
    used = last["used"]
    out["frame_bytes"] = sum(used)
    r, res, errors = ctx.measure_frames(bufs, used, 1, pictures, w, h)
    assert r == 0 and not any(res), (r, res)
    channels = 4 if fmt == FMT_DXT5 else 3
    sse = [sum(e.sse[c] for e in errors) for c in range(channels)]
    out["sse"] = sse
    out["psnr_db"] = {"RGBA"[c]: (round(hap_amd.psnr(sse[c], n * w * h), 3) if sse[c] else "inf") for c in range(channels)}
    out["psnr_db"]["rgb"] = round(hap_amd.psnr(sum(sse[:3]), 3 * n * w * h), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_endpoints.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    ap.add_argument("--unflagged-only", action="store_true", help="the call without the flag alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "refine_endpoints_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "times": "[median, min, max] ms", "frames": FRAMES, "chunks": CHUNKS,
           "library": os.environ.get("HAP_AMD_LIBRARY", "in-tree")}
    for gname, w, h in GEOMETRIES:
        w, h = w // args.shrink // 4 * 4, h // args.shrink // 4 * 4
        distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(4)]
        pictures = [distinct[i % 4] for i in range(FRAMES)]
        for fname, fmt in FLAVOURS:
            cap = hap_amd.HapMaxEncodedLength([(w // 4) * (h // 4) * BLOCK_BYTES[fmt]], [fmt], [CHUNKS])
            bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(FRAMES)]
            torch.cuda.synchronize()
            for table in (0, hap_amd.ENCODE_FRAGMENT_INDEX):
                name = "%s_%s_x%d%s" % (fname, gname, FRAMES, "_table" if table else "")
                case = {"geometry": [w, h], "format": fmt}
                case["default"] = one_side(ctx, pictures, bufs, w, h, fmt, table, args.reps)
                if not args.unflagged_only:
                    case["refined"] = one_side(ctx, pictures, bufs, w, h, fmt, table | REFINE, args.reps)
                    case["refined_over_default"] = round(case["refined"]["call_ms"][0] / case["default"]["call_ms"][0], 3)
                    case["bytes_ratio"] = round(case["refined"]["frame_bytes"] / case["default"]["frame_bytes"], 4)
                    case["psnr_gain_db"] = round(case["refined"]["psnr_db"]["rgb"] - case["default"]["psnr_db"]["rgb"], 3)
                res[name] = case
                print("%s: done" % name, file=sys.stderr, flush=True)
            del bufs
            torch.cuda.empty_cache()
        del pictures, distinct
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

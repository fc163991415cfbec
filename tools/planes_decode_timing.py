"""GPU timing of the planar decode call (HapGpuDecodeFramesPlanes) against the path a client has without it:
HapGpuDecodeFramesRGBA[Scaled] into device pictures, then torch -- permute(0, 3, 1, 2), conversion to half, multiply and
add -- into a preallocated tensor.

    python tools/planes_decode_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and tensors in HBM, sources made here from hap_amd.synth pictures (16 chunks a texture):

  hap_q_8k_x60           60 Hap Q frames of 7680 x 4320, hap.h sections only       -> three half planes
  hap_q_8k_x60_table     the same with the fragment table (ENCODE_FRAGMENT_INDEX)   -> three half planes
  hap_q_alpha_16k_x4     4 Hap Q Alpha frames of 15360 x 8640                       -> four half planes

each at scale_log2 0 and 2, with the ImageNet constants.  Per workload and scale, medians of N calls after warm-up between
HIP events (every route ends with the host waiting, so the events bracket all of it), in one process:

  planes_ms              the one call
  rgba_then_torch_ms     the three-step path as written (copy_ of the permuted view into the half tensor, mul_, add_) and
                         as a single expression (torch.addcmul of the converted view); the faster is the baseline
  block_decode_ms        the block-decode kernels' own time in the one call, by profile class, and their fraction of HBM
                         peak from the bytes they must move: blocks read plus planes written

The torch path rounds differently (half arithmetic): the two tensors are compared to a tolerance only, as a check that
both routes computed the same thing.  Prints one JSON line.
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

FMT_YCOCG, FMT_RGTC1 = 0x01, 0x8DBB
BLOCK_BYTES = {FMT_YCOCG: 16, FMT_RGTC1: 8}
HBM_PEAK_GBS = 8000.0
# name, width, height, frames, source formats, encode flags of the sources
WORKLOADS = (("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,), ""),
             ("hap_q_8k_x60_table", 7680, 4320, 60, (FMT_YCOCG,), "index"),
             ("hap_q_alpha_16k_x4", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1), ""))
SCALES = (0, 2)
CHUNKS = 16
STD = (0.229, 0.224, 0.225, 1.0)
MEAN = (0.485, 0.456, 0.406, 0.0)


def make_frames(ctx, w, h, count, fmts, flags):
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))
    distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(min(count, 4))]
    frames, used = [], []
    for first in range(0, count, 4):
        n = min(4, count - first)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        r, u, res = ctx.encode_frames_rgba([distinct[(first + i) % len(distinct)] for i in range(n)], w, h, w * 4, list(fmts),
                                           [1] * len(fmts), [CHUNKS] * len(fmts), bufs, flags=flags)
        assert r == 0 and res == [0] * n, (r, res)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
    del distinct
    torch.cuda.empty_cache()
    return frames, used


def median_ms(call, reps):
    """median ms between HIP events around `call`, which leaves nothing running on any stream but torch's"""
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
    return round(statistics.median(times), 3)


def block_decode_ms(ctx, call, reps):
    times = []
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        times.append(ctx.collect_profile()["block_decode"][1])
    ctx.set_profiling(False)
    return statistics.median(times)


def one_case(ctx, frames, used, w, h, src, s, reps):
    count, channels = len(frames), 2 + len(src)
    ow, oh = w >> s, h >> s
    scale = [1.0 / (255.0 * v) for v in STD[:channels]]
    bias = [-m / v for m, v in zip(MEAN, STD)][:channels]
    out = {route: torch.zeros((count, channels, oh, ow), dtype=torch.float16, device="cuda")
           for route in ("planes", "as_written", "single_expression")}
    pics = torch.zeros((count, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pic_list = [pics[i] for i in range(count)]
    scale_t = torch.tensor(scale, dtype=torch.float16, device="cuda").view(1, channels, 1, 1)
    bias_t = torch.tensor(bias, dtype=torch.float16, device="cuda").view(1, channels, 1, 1)
    torch.cuda.synchronize()

    def planes():
        r, res = ctx.decode_frames_planes(frames, used, len(src), out["planes"], w, h, scale_log2=s, scale=scale, bias=bias)
        assert r == 0 and not any(res), (r, res)

    def rgba():
        if s:
            r, res = ctx.decode_frames_rgba_scaled(frames, used, len(src), pic_list, w, h, s)
        else:
            r, res = ctx.decode_frames_rgba(frames, used, len(src), pic_list, w, h)
        assert r == 0 and not any(res), (r, res)
        return pics.permute(0, 3, 1, 2)[:, :channels]

    def as_written():
        o = out["as_written"]
        o.copy_(rgba())
        o.mul_(scale_t)
        o.add_(bias_t)

    def single_expression():
        torch.addcmul(bias_t, rgba().to(torch.float16), scale_t, out=out["single_expression"])

    blocks = (w // 4) * (h // 4)
    moved = count * (blocks * sum(BLOCK_BYTES[f] for f in src) + channels * ow * oh * 2)
    res = {"scale_log2": s, "planes": channels, "element": "float16", "tensor_bytes": count * channels * ow * oh * 2,
           "picture_bytes_the_torch_path_holds": count * ow * oh * 4}
    res["planes_ms"] = median_ms(planes, reps)
    res["rgba_then_torch_ms"] = {"as_written": median_ms(as_written, reps),
                                 "single_expression": median_ms(single_expression, reps)}
    res["rgba_ms"] = median_ms(rgba, reps)
    baseline = min(res["rgba_then_torch_ms"].values())
    res["planes_over_rgba_then_torch"] = round(res["planes_ms"] / baseline, 3)
    kernel = block_decode_ms(ctx, planes, reps)
    res["block_decode_ms"] = round(kernel, 4)
    res["block_decode_ms_of_the_rgba_call"] = round(block_decode_ms(ctx, rgba, reps), 4)
    res["block_decode_bytes"] = moved
    res["block_decode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    torch.cuda.synchronize()
    res["max_difference_from_the_torch_path"] = float((out["planes"] - out["as_written"]).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_decode.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "planes_decode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS}
    for name, w, h, count, src, flag in WORKLOADS:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        frames, used = make_frames(ctx, w, h, count, src, hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0)
        res[name] = {"geometry": [w, h], "frames": count, "source_formats": list(src), "source_flags": flag or "none",
                     "frame_bytes_per_step": sum(used)}
        for s in SCALES:
            res[name]["scale_log2_%d" % s] = one_case(ctx, frames, used, w, h, src, s, args.reps)
            print("%s at scale_log2 %d: done" % (name, s), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        del frames
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

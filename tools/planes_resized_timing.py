"""GPU timing of the planar decode of a resized crop per frame (HapGpuDecodeFramesPlanesResized) against the road a client
has without it.

    python tools/planes_resized_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and tensors in HBM, sources made here from hap_amd.synth pictures (16 chunks a texture), all to three
half planes of 224 x 224 with the ImageNet constants:

  hap_q_8k_x60_table     60 Hap Q frames of 7680 x 4320 with the fragment table
  hap_q_8k_x60           the same, hap.h sections only (the block scan's pieces)
  hap_1080p_x256         256 Hap frames of 1920 x 1080, hap.h sections only

each with a random-resized crop per frame (fixed seed): 8 % to 100 % of the frame's area at an aspect of 3/4 to 4/3, as
a training loader draws them, a side cut to the 16 x 224 texels the call can take; scale_log2 is the smallest at which
every crop of the call is at most 4 x 224 texels of the level a side, and the crops are given in texels of that level.
Per workload, medians of N calls after warm-up between HIP events (every route ends with the host waiting, so the events
bracket all of it), in one process:

  planes_resized_ms          the one call
  region_then_interpolate_ms one HapGpuDecodeFramesPlanesRegion call per frame (each crop has its own size) of the crop
                             rounded outward to the blocks, at the same scale_log2, then torch's slice,
                             torch.nn.functional.interpolate(mode="bilinear", antialias=False) and the copy into the batch
  kernels_ms                 the one call's kernel time by profile class (decode_plan holds the skip kernel)
  skipped_texture_bytes      the rise of HapGpuSkippedTextureBytes per step of the one call, beside the textures' bytes

and the largest difference between the two roads' tensors (they are not the same filter bit for bit: the call's is the
integer definition of include/hap_gpu.h).  Prints one JSON line.
"""
import argparse
import json
import math
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

FMT_DXT1, FMT_YCOCG = 0x83F0, 0x01
BLOCK_BYTES = {FMT_DXT1: 8, FMT_YCOCG: 16}
# name, width, height, frames, source format, encode flags of the sources
WORKLOADS = (("hap_q_8k_x60_table", 7680, 4320, 60, FMT_YCOCG, "index"),
             ("hap_q_8k_x60", 7680, 4320, 60, FMT_YCOCG, ""),
             ("hap_1080p_x256", 1920, 1080, 256, FMT_DXT1, ""))
CHUNKS = 16
OUT = 224
RATIO = 4                   # a crop is at most 4 x the output a side, at scale_log2 0 to 2
SEED = 20240611
STD = (0.229, 0.224, 0.225)
MEAN = (0.485, 0.456, 0.406)
CLASSES = ("decode_plan", "block_scan", "snappy_decode", "block_decode")


def make_frames(ctx, w, h, count, fmt, flags):
    cap = hap_amd.HapMaxEncodedLength([(w // 4) * (h // 4) * BLOCK_BYTES[fmt]], [fmt], [CHUNKS])
    distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(min(count, 4))]
    frames, used = [], []
    for first in range(0, count, 4):
        n = min(4, count - first)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        r, u, res = ctx.encode_frames_rgba([distinct[(first + i) % len(distinct)] for i in range(n)], w, h, w * 4, [fmt], [1],
                                           [CHUNKS], bufs, flags=flags)
        assert r == 0 and res == [0] * n, (r, res)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
    del distinct
    torch.cuda.empty_cache()
    return frames, used


def random_resized_crop(rng, w, h, most):
    """(x, y, cw, ch) in full-size texels, as torchvision's RandomResizedCrop draws it: 8 % to 100 % of the area, the
    logarithm of the aspect uniform between 3/4 and 4/3; the whole frame after ten draws that do not fit"""
    for _ in range(10):
        area = w * h * rng.uniform(0.08, 1.0)
        aspect = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            break
    else:
        cw, ch = w, h
    cw, ch = min(cw, most), min(ch, most)
    return rng.randrange(w - cw + 1), rng.randrange(h - ch + 1), cw, ch


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


def kernels_ms(ctx, call, reps):
    kernel = {c: [] for c in CLASSES}
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        prof = ctx.collect_profile()
        for c in CLASSES:
            kernel[c].append(prof[c][1])
    ctx.set_profiling(False)
    return {c: round(statistics.median(v), 4) for c, v in kernel.items()}


def one_case(ctx, frames, used, w, h, crops, s, out, reps):
    count = len(frames)
    scale = [1.0 / (255.0 * v) for v in STD]
    bias = [-m / v for m, v in zip(MEAN, STD)]
    half = torch.float16
    resized = torch.zeros((count, 3, out, out), dtype=half, device="cuda")
    stacked = torch.zeros((count, 3, out, out), dtype=half, device="cuda")
    # the other road's rectangles: every crop taken back to full-size texels and rounded outward to the blocks
    rects = []
    for x, y, cw, ch in crops:
        x0, y0 = (x << s) & ~3, (y << s) & ~3
        rects.append((x0, y0, ((((x + cw) << s) + 3) & ~3) - x0, ((((y + ch) << s) + 3) & ~3) - y0))
    torch.cuda.synchronize()

    def one_call():
        r, res = ctx.decode_frames_planes_resized(frames, used, 1, resized, w, h, crops, (out, out), scale_log2=s, scale=scale,
                                                  bias=bias)
        assert r == 0 and not any(res), (r, res)

    def region_then_interpolate():
        for f, ((x, y, cw, ch), (x0, y0, rw, rh)) in enumerate(zip(crops, rects)):
            block = torch.empty((1, 3, rh >> s, rw >> s), dtype=half, device="cuda")
            r, res = ctx.decode_frames_planes_region([frames[f]], [used[f]], 1, block, w, h, [(x0, y0)], (rw, rh), scale_log2=s,
                                                     scale=scale, bias=bias)
            assert r == 0 and not any(res), (r, res)
            ox, oy = x - (x0 >> s), y - (y0 >> s)
            stacked[f] = torch.nn.functional.interpolate(block[:, :, oy: oy + ch, ox: ox + cw], size=(out, out), mode="bilinear",
                                                         antialias=False, align_corners=False)[0]

    res = {"scale_log2": s, "planes": 3, "element": "float16", "out": [out, out], "tensor_bytes": count * 3 * out * out * 2}
    res["planes_resized_ms"] = median_ms(one_call, reps)
    res["region_then_interpolate_ms"] = median_ms(region_then_interpolate, reps)
    res["planes_resized_over_region_then_interpolate"] = round(res["planes_resized_ms"] / res["region_then_interpolate_ms"], 4)
    res["kernels_ms"] = kernels_ms(ctx, one_call, reps)
    res["block_decode_share_of_the_call"] = round(res["kernels_ms"]["block_decode"] / res["planes_resized_ms"], 4)
    before = ctx.skipped_texture_bytes()
    one_call()
    res["skipped_texture_bytes"] = ctx.skipped_texture_bytes() - before
    region_then_interpolate()
    torch.cuda.synchronize()
    res["max_difference_from_region_then_interpolate"] = float((resized.float() - stacked.float()).abs().max())
    res["a_byte_in_elements"] = round(max(scale), 6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_resized.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide the geometries' sides and the output's by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "planes_resized_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "seed": SEED}
    out = max(OUT // args.shrink, 1)
    for name, w, h, count, fmt, flag in WORKLOADS:
        w, h = w // args.shrink // 4 * 4, h // args.shrink // 4 * 4
        rng = random.Random(SEED)
        full = [random_resized_crop(rng, w, h, RATIO * 4 * out) for _ in range(count)]
        s = next(k for k in (0, 1, 2) if all(max(c[2], c[3]) >> k <= RATIO * out for c in full) or k == 2)
        crops = [(x >> s, y >> s, max(cw >> s, 1), max(ch >> s, 1)) for x, y, cw, ch in full]
        frames, used = make_frames(ctx, w, h, count, fmt, hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0)
        res[name] = {"geometry": [w, h], "frames": count, "source_format": fmt, "source_flags": flag or "none",
                     "frame_bytes_per_step": sum(used), "texture_bytes_per_step": count * (w // 4) * (h // 4) * BLOCK_BYTES[fmt],
                     "crop_share_of_the_frame_mean": round(sum(c[2] * c[3] for c in full) / (count * w * h), 4),
                     "crops_in_level_texels": crops}
        res[name].update(one_case(ctx, frames, used, w, h, crops, s, out, args.reps))
        print("%s at scale_log2 %d: done" % (name, s), file=sys.stderr, flush=True)
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

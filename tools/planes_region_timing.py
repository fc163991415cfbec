"""GPU timing of the planar decode of a crop per frame (HapGpuDecodeFramesPlanesRegion) against the two roads a client has
without it.

    python tools/planes_region_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and tensors in HBM, sources made here from hap_amd.synth pictures (16 chunks a texture):

  hap_q_8k_x60_table         60 Hap Q frames of 7680 x 4320 with the fragment table    -> three half planes
  hap_q_8k_x60               the same, hap.h sections only (the block scan's pieces)   -> three half planes
  hap_q_alpha_16k_x4_table   4 Hap Q Alpha frames of 15360 x 8640 with the table       -> four half planes

each with a 1024 x 1024 rectangle at a random block-aligned origin per frame (fixed seed), at scale_log2 0 and 1, with the
ImageNet constants.  Per workload and scale, medians of N calls after warm-up between HIP events (every route ends with
the host waiting, so the events bracket all of it), in one process:

  planes_region_ms           the one call
  planes_then_slice_ms       (a) HapGpuDecodeFramesPlanes of the whole frames, then torch's slice and .contiguous() per frame
  region_then_torch_ms       (b) one HapGpuDecodeFramesRGBARegion call per frame (each has its own rectangle), then torch --
                             permute, conversion to half, multiply, add; at scale_log2 1 also a 2 x 2 average pool, which a
                             client has to add because that call has no scale (it rounds differently)
  kernels_ms                 the one call's kernel time by profile class (decode_plan holds the skip kernel)
  skipped_texture_bytes      the rise of HapGpuSkippedTextureBytes per step of the one call, beside the textures' bytes

The one call's tensors are compared bit for bit with the crops of road (a)'s.  Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

FMT_YCOCG, FMT_RGTC1 = 0x01, 0x8DBB
BLOCK_BYTES = {FMT_YCOCG: 16, FMT_RGTC1: 8}
# name, width, height, frames, source formats, encode flags of the sources
WORKLOADS = (("hap_q_8k_x60_table", 7680, 4320, 60, (FMT_YCOCG,), "index"),
             ("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,), ""),
             ("hap_q_alpha_16k_x4_table", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1), "index"))
SCALES = (0, 1)
CHUNKS = 16
CROP = 1024
SEED = 20240611
STD = (0.229, 0.224, 0.225, 1.0)
MEAN = (0.485, 0.456, 0.406, 0.0)
CLASSES = ("decode_plan", "block_scan", "snappy_decode", "block_decode")


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


def one_case(ctx, frames, used, w, h, src, origins, size, s, reps):
    count, channels = len(frames), 2 + len(src)
    cw, ch = size[0] >> s, size[1] >> s
    scale = [1.0 / (255.0 * v) for v in STD[:channels]]
    bias = [-m / v for m, v in zip(MEAN, STD)][:channels]
    half = torch.float16
    crops = torch.zeros((count, channels, ch, cw), dtype=half, device="cuda")
    whole = torch.zeros((count, channels, h >> s, w >> s), dtype=half, device="cuda")
    pics = torch.zeros((count, size[1], size[0], 4), dtype=torch.uint8, device="cuda")
    from_pics = torch.zeros((count, channels, ch, cw), dtype=half, device="cuda")
    scale_t = torch.tensor(scale, dtype=half, device="cuda").view(1, channels, 1, 1)
    bias_t = torch.tensor(bias, dtype=half, device="cuda").view(1, channels, 1, 1)
    torch.cuda.synchronize()

    def region():
        r, res = ctx.decode_frames_planes_region(frames, used, len(src), crops, w, h, origins, size, scale_log2=s,
                                                 scale=scale, bias=bias)
        assert r == 0 and not any(res), (r, res)

    def planes_then_slice():
        r, res = ctx.decode_frames_planes(frames, used, len(src), whole, w, h, scale_log2=s, scale=scale, bias=bias)
        assert r == 0 and not any(res), (r, res)
        return [whole[f, :, y >> s: (y + size[1]) >> s, x >> s: (x + size[0]) >> s].contiguous()
                for f, (x, y) in enumerate(origins)]

    def region_then_torch():
        for f, (x, y) in enumerate(origins):
            r, res = ctx.decode_frames_rgba_region([frames[f]], [used[f]], len(src), [pics[f]], w, h, (x, y) + tuple(size))
            assert r == 0 and not any(res), (r, res)
        planar = pics.permute(0, 3, 1, 2)[:, :channels].to(half)
        if s:
            planar = torch.nn.functional.avg_pool2d(planar, 1 << s)
        from_pics.copy_(planar)
        from_pics.mul_(scale_t)
        from_pics.add_(bias_t)

    res = {"scale_log2": s, "planes": channels, "element": "float16", "crop": list(size),
           "tensor_bytes": count * channels * cw * ch * 2,
           "whole_tensor_bytes_road_a_holds": count * channels * (w >> s) * (h >> s) * 2}
    res["planes_region_ms"] = median_ms(region, reps)
    res["planes_then_slice_ms"] = median_ms(planes_then_slice, reps)
    res["region_then_torch_ms"] = median_ms(region_then_torch, reps)
    res["planes_region_over_planes_then_slice"] = round(res["planes_region_ms"] / res["planes_then_slice_ms"], 4)
    res["planes_region_over_region_then_torch"] = round(res["planes_region_ms"] / res["region_then_torch_ms"], 4)
    res["kernels_ms"] = kernels_ms(ctx, region, reps)
    res["kernels_ms_of_the_whole_frame_call"] = kernels_ms(
        ctx, lambda: ctx.decode_frames_planes(frames, used, len(src), whole, w, h, scale_log2=s, scale=scale, bias=bias), reps)
    before = ctx.skipped_texture_bytes()
    region()
    res["skipped_texture_bytes"] = ctx.skipped_texture_bytes() - before
    want = planes_then_slice()
    torch.cuda.synchronize()
    res["equals_crop_of_whole_frame_tensor"] = all(torch.equal(crops[f].view(torch.int16), want[f].view(torch.int16))
                                                   for f in range(count))
    res["max_difference_from_region_then_torch"] = float((crops - from_pics).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_region.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide the geometries' and the crop's sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "planes_region_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "seed": SEED}
    for name, w, h, count, src, flag in WORKLOADS:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        size = (CROP // args.shrink // 16 * 16,) * 2
        rng = random.Random(SEED)
        origins = [(4 * rng.randrange((w - size[0]) // 4 + 1), 4 * rng.randrange((h - size[1]) // 4 + 1)) for _ in range(count)]
        frames, used = make_frames(ctx, w, h, count, src, hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0)
        texture_bytes = count * (w // 4) * (h // 4) * sum(BLOCK_BYTES[f] for f in src)
        res[name] = {"geometry": [w, h], "frames": count, "source_formats": list(src), "source_flags": flag or "none",
                     "frame_bytes_per_step": sum(used), "texture_bytes_per_step": texture_bytes,
                     "rectangle_share_of_the_frame": round(size[0] * size[1] / (w * h), 5), "origins": origins}
        for s in SCALES:
            res[name]["scale_log2_%d" % s] = one_case(ctx, frames, used, w, h, src, origins, size, s, args.reps)
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

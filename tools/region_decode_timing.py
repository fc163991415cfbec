"""GPU timing of the region decode (HapGpuDecodeFramesRGBARegion) against the full-size call it replaces for clients that
show a tile of a large canvas.

    python tools/region_decode_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and pictures in HBM: 4 Hap Q Alpha frames of 15360 x 8640 per step and 60 Hap Q frames of 7680 x 4320,
each as "table" frames (HAPGPU_ENCODE_FRAGMENT_INDEX: the private fragment table) and as "plain" frames (hap.h sections
only: the decoder's block scan finds their 8 KiB pieces), 16 chunks a texture, made here from hap_amd.synth pictures.
Per workload and frame kind, medians of N calls after warm-up, by the context's own timer (HIP events on its stream
around the whole call):

  full   HapGpuDecodeFramesRGBA
  band   the region call for a one-eighth row band in the middle of the frame: (0, H / 2, W, H / 8 rounded to blocks)
  tile   the region call for a one-eighth tile: a quarter of the width by half the height, off the frame's edges

with, per leg, the kernel time by profile class (decode_plan -- which holds the skip kernel --, block_scan, snappy_decode,
block_decode; taken in separate calls) and the rise of HapGpuSkippedTextureBytes per call.  The pictures of the first
frame are compared with the crop of its full-size picture.  Prints one JSON line.
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
WORKLOADS = (("hap_q_alpha_16k_x4", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1)), ("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,)))
CLASSES = ("decode_plan", "block_scan", "snappy_decode", "block_decode")


def make_frames(ctx, w, h, count, fmts, flags):
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
                                           [1] * len(fmts), chunks, bufs, flags=flags)
        assert r == 0 and res == [0] * n, (r, res)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
    del distinct
    torch.cuda.empty_cache()
    return frames, used


def measure(ctx, call, reps):
    """median call ms by the context's timer, median kernel ms per profile class, skipped bytes per call"""
    for _ in range(2):
        call()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        times.append(ctx.timer_stop())
    before = ctx.skipped_texture_bytes()
    call()
    skipped = ctx.skipped_texture_bytes() - before
    kernel = {c: [] for c in CLASSES}
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        prof = ctx.collect_profile()
        for c in CLASSES:
            kernel[c].append(prof[c][1])
    ctx.set_profiling(False)
    out = {"call_ms": round(statistics.median(times), 3), "skipped_texture_bytes": skipped}
    out.update({c + "_ms": round(statistics.median(v), 4) for c, v in kernel.items()})
    out["kernels_ms"] = round(sum(out[c + "_ms"] for c in CLASSES), 4)
    return out


def one_workload(ctx, w, h, count, fmts, reps):
    tc = len(fmts)
    band = (0, h // 2 // 4 * 4, w, h // 8 // 4 * 4)
    tile = (w // 8 // 4 * 4, h // 4 // 4 * 4, w // 4 // 4 * 4, h // 2 // 4 * 4)
    res = {"geometry": [w, h], "frames": count, "textures_per_frame": tc, "band": band, "tile": tile,
           "texture_bytes_per_step": count * (w // 4) * (h // 4) * (16 + (8 if tc == 2 else 0))}
    full = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(count)]
    pics = {name: [torch.zeros(r[2] * r[3] * 4, dtype=torch.uint8, device="cuda") for _ in range(count)]
            for name, r in (("band", band), ("tile", tile))}
    for kind, flags in (("table", hap_amd.ENCODE_FRAGMENT_INDEX), ("plain", 0)):
        frames, used = make_frames(ctx, w, h, count, fmts, flags)
        torch.cuda.synchronize()

        def ok(r):
            assert r[0] == 0 and not any(r[1]), r

        legs = (("full", lambda: ok(ctx.decode_frames_rgba(frames, used, tc, full, w, h))),
                ("band", lambda: ok(ctx.decode_frames_rgba_region(frames, used, tc, pics["band"], w, h, band))),
                ("tile", lambda: ok(ctx.decode_frames_rgba_region(frames, used, tc, pics["tile"], w, h, tile))))
        out = {"frame_bytes_per_step": sum(used)}
        for leg, call in legs:
            out[leg] = measure(ctx, call, reps)
        for leg, r in (("band", band), ("tile", tile)):
            want = full[0].view(h, w, 4)[r[1]: r[1] + r[3], r[0]: r[0] + r[2]].contiguous().view(-1)
            out[leg + "_equals_crop_of_full_size"] = bool(torch.equal(pics[leg][0], want))
            out[leg + "_call_over_full"] = round(out[leg]["call_ms"] / out["full"]["call_ms"], 3)
            out[leg + "_kernels_over_full"] = round(out[leg]["kernels_ms"] / out["full"]["kernels_ms"], 3)
        res[kind] = out
        del frames
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "region_decode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps}
    for name, w, h, count, fmts in WORKLOADS:
        w, h = w // args.shrink // 4 * 4, h // args.shrink // 4 * 4
        res[name] = one_workload(ctx, w, h, count, fmts, args.reps)
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

"""GPU timing of the measuring call (HapGpuMeasureFrames) against the path a client has without it:
HapGpuDecodeFramesRGBA into device pictures, then torch -- widen, subtract, square or abs, sum per channel -- and a host
read-back of the eight sums per frame.

    python tools/measure_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and pictures in HBM, sources made here from hap_amd.synth pictures (16 chunks a texture), every frame
measured against a copy of its own source picture:

  hap_q_8k_x60           60 Hap Q frames of 7680 x 4320, hap.h sections only
  hap_q_8k_x60_table     the same with the fragment table (ENCODE_FRAGMENT_INDEX)
  hap_q_alpha_16k_x4     4 Hap Q Alpha frames of 15360 x 8640

Per workload, medians of N calls after warm-up between HIP events (every route ends with the host waiting, so the events
bracket all of it), in one process:

  measure_ms             (a) the one call
  rgba_then_torch_ms     (b) decode_frames_rgba, then one of three torch expressions for the eight sums per frame, then
                         .cpu(); the fastest is the baseline and is named
  rgba_ms                (c) decode_frames_rgba alone
  block_decode_ms        the block kernels' own time in (a) and in (c), by profile class, and (a)'s fraction of HBM peak
                         from the bytes it must move: per block the texture's 16 (+ 8) bytes and 64 of the picture

The structs of (a) must equal the sums of (b) for every frame, or the tool fails.  Prints one JSON line.
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
CHUNKS = 16


def make_frames(ctx, w, h, count, fmts, flags):
    """(frames, their sizes, a copy of every frame's source picture)"""
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))
    distinct = [synth.rgba_frame(w, h, i, device="cuda") for i in range(min(count, 4))]
    frames, used, sources = [], [], []
    for first in range(0, count, 4):
        n = min(4, count - first)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        pictures = [distinct[(first + i) % len(distinct)] for i in range(n)]
        r, u, res = ctx.encode_frames_rgba(pictures, w, h, w * 4, list(fmts), [1] * len(fmts), [CHUNKS] * len(fmts), bufs,
                                           flags=flags)
        assert r == 0 and res == [0] * n, (r, res)
        frames += [b[:x].clone() for b, x in zip(bufs, u)]
        used += list(u)
        sources += [p.clone() for p in pictures]
    del distinct
    torch.cuda.empty_cache()
    return frames, used, sources


def timed_ms(call, reps):
    """(median, min, max) ms between HIP events around `call`, which leaves nothing running on any stream but torch's"""
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


def block_decode_ms(ctx, call, reps):
    times = []
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        times.append(ctx.collect_profile()["block_decode"][1])
    ctx.set_profiling(False)
    return statistics.median(times)


# The eight sums per frame from decoded pictures d and reference pictures p, both (N, H, W, 4) uint8 in HBM: (N, 2, 4)
# int64 on the host, [:, 0] the squares and [:, 1] the absolute values.  All exact.
def sums_int32_per_frame(d, p):
    out = torch.empty((d.shape[0], 2, 4), dtype=torch.int64, device=d.device)
    for f in range(d.shape[0]):
        e = d[f].to(torch.int32) - p[f].to(torch.int32)
        out[f, 0] = (e * e).sum(dim=(0, 1))
        out[f, 1] = e.abs().sum(dim=(0, 1))
    return out.cpu()


def sums_float64_per_frame(d, p):
    # (float32 holds every difference and square exactly, and a float64 sum of integers below 2^53 is exact)
    out = torch.empty((d.shape[0], 2, 4), dtype=torch.float64, device=d.device)
    for f in range(d.shape[0]):
        e = d[f].to(torch.float32) - p[f].to(torch.float32)
        out[f, 0] = (e * e).sum(dim=(0, 1), dtype=torch.float64)
        out[f, 1] = e.abs().sum(dim=(0, 1), dtype=torch.float64)
    return out.to(torch.int64).cpu()


def sums_int16_whole_batch(d, p):
    e = d.to(torch.int16) - p.to(torch.int16)
    sad = e.abs().sum(dim=(1, 2), dtype=torch.int64)
    sse = (e.to(torch.int32) ** 2).sum(dim=(1, 2), dtype=torch.int64)
    return torch.stack((sse, sad), dim=1).cpu()


EXPRESSIONS = {"int32_per_frame": sums_int32_per_frame, "float64_sums_per_frame": sums_float64_per_frame,
               "int16_whole_batch": sums_int16_whole_batch}


def one_case(ctx, frames, used, sources, w, h, src, reps):
    count = len(frames)
    refs = torch.stack(sources)
    del sources[:]
    pics = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    ref_list, pic_list = [refs[i] for i in range(count)], [pics[i] for i in range(count)]
    torch.cuda.synchronize()
    last = {}

    def measure():
        r, res, errors = ctx.measure_frames(frames, used, len(src), ref_list, w, h)
        assert r == 0 and not any(res), (r, res)
        last["measure"] = errors

    def rgba():
        r, res = ctx.decode_frames_rgba(frames, used, len(src), pic_list, w, h)
        assert r == 0 and not any(res), (r, res)

    def rgba_then(expression):
        def call():
            rgba()
            last[expression] = EXPRESSIONS[expression](pics, refs)
        return call

    blocks = (w // 4) * (h // 4)
    moved = count * blocks * (sum(BLOCK_BYTES[f] for f in src) + 64)
    res = {"picture_bytes_the_torch_path_holds": count * w * h * 4, "reference_picture_bytes": count * w * h * 4}
    res["measure_ms"] = timed_ms(measure, reps)
    res["rgba_ms"] = timed_ms(rgba, reps)
    res["rgba_then_torch_ms"] = {}
    for expression in EXPRESSIONS:
        res["rgba_then_torch_ms"][expression] = timed_ms(rgba_then(expression), reps)
        torch.cuda.empty_cache()
    fastest = min(res["rgba_then_torch_ms"], key=lambda k: res["rgba_then_torch_ms"][k][0])
    res["fastest_torch_expression"] = fastest
    res["measure_over_rgba"] = round(res["measure_ms"][0] / res["rgba_ms"][0], 3)
    res["measure_over_rgba_then_torch"] = round(res["measure_ms"][0] / res["rgba_then_torch_ms"][fastest][0], 3)
    kernel = block_decode_ms(ctx, measure, reps)
    res["block_decode_ms"] = round(kernel, 4)
    res["block_decode_ms_of_the_rgba_call"] = round(block_decode_ms(ctx, rgba, reps), 4)
    res["block_decode_bytes"] = moved
    res["block_decode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    # the tool's own sanity: the structs of (a) are the sums of (b), for every frame and every expression
    got = [[list(e.sse), list(e.sad)] for e in last["measure"]]
    for expression in EXPRESSIONS:
        assert last[expression].tolist() == got, expression
    assert all(e.texels == w * h for e in last["measure"])
    res["structs_equal_the_torch_sums"] = True
    sse = [sum(e.sse[c] for e in last["measure"]) for c in range(4)]
    res["psnr_db"] = {"rgb": round(hap_amd.psnr(sum(sse[:3]), 3 * count * w * h), 3),
                      "alpha": round(hap_amd.psnr(sse[3], count * w * h), 3) if sse[3] else "inf"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS, "times": "[median, min, max] ms"}
    for name, w, h, count, src, flag in WORKLOADS:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        frames, used, sources = make_frames(ctx, w, h, count, src, hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0)
        res[name] = {"geometry": [w, h], "frames": count, "source_formats": list(src), "source_flags": flag or "none",
                     "frame_bytes_per_step": sum(used)}
        res[name].update(one_case(ctx, frames, used, sources, w, h, src, args.reps))
        print("%s: done" % name, file=sys.stderr, flush=True)
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

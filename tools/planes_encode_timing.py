"""GPU timing of the planar encode call (HapGpuEncodeFramesPlanes) against the path a client has without it: torch --
multiply, add, round, clamp, conversion to bytes, permute into a preallocated RGBA8 batch whose alpha is 255 -- and then
HapGpuEncodeFramesRGBA of those pictures, fused compress kernel included.

    python tools/planes_encode_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, tensors and frames in HBM, tensors made here from hap_amd.synth pictures (16 Snappy chunks a texture):

  hap_q_8k_x60           60 tensors of three half planes, 7680 x 4320   -> Hap Q frames, hap.h sections only
  hap_q_8k_x60_table     the same                                       -> Hap Q frames with the fragment table
  hap_q_alpha_16k_x4     4 tensors of four half planes, 15360 x 8640    -> Hap Q Alpha frames

with scale 255 and bias 0.  Per workload, medians of N calls after warm-up between HIP events (every route ends with the
host waiting, so the events bracket all of it), in one process:

  planes_ms              the one call
  torch_then_rgba_ms     the detour, its torch half as separate statements and as one expression; the faster is the baseline
  torch_ms, rgba_ms      the detour's two halves by themselves (the faster torch form)
  block_encode_ms        the block-encode kernel's own time in the one call, by profile class, and its fraction of HBM
                         peak from the bytes it must move: planes read plus blocks written

The torch path computes in half precision: its pictures are compared with the call's definition to a tolerance only
(the largest byte difference is reported), as a check that both routes computed the same thing; the frames are not
compared.  Prints one JSON line.
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
# name, width, height, tensors, destination formats, encode flags
WORKLOADS = (("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,), ""),
             ("hap_q_8k_x60_table", 7680, 4320, 60, (FMT_YCOCG,), "index"),
             ("hap_q_alpha_16k_x4", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1), ""))
CHUNKS = 16


def make_tensor(w, h, count, channels):
    """(count, channels, h, w) half elements in 0 .. 1 from the synthetic pictures (four distinct ones)"""
    out = torch.empty((count, channels, h, w), dtype=torch.float16, device="cuda")
    for i in range(min(count, 4)):
        pic = synth.rgba_frame(w, h, i, device="cuda")
        out[i].copy_(pic.permute(2, 0, 1)[:channels].to(torch.float32) / 255.0)
    for i in range(4, count):
        out[i].copy_(out[i % 4])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


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


def class_ms(ctx, call, reps, name):
    times = []
    ctx.set_profiling(True)
    for _ in range(reps):
        ctx.collect_profile()
        call()
        times.append(ctx.collect_profile()[name][1])
    ctx.set_profiling(False)
    return statistics.median(times)


def one_case(ctx, tensor, w, h, fmts, flags, reps):
    count, channels = tensor.shape[0], tensor.shape[1]
    fmts = list(fmts)
    n = len(fmts)
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, fmts, [CHUNKS] * n)
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)]
    pics = torch.full((count, h, w, 4), 255, dtype=torch.uint8, device="cuda")          # alpha stays 255 with three planes
    pic_list = [pics[i] for i in range(count)]
    target = pics.permute(0, 3, 1, 2)[:, :channels]
    torch.cuda.synchronize()
    comps, chunks = [1] * n, [CHUNKS] * n
    used = {}

    def planes():
        r, u, res = ctx.encode_frames_planes(tensor, w, h, fmts, comps, chunks, outs, flags=flags)
        assert r == 0 and not any(res), (r, res)
        used["planes"] = u

    def as_written():
        x = tensor * 255.0
        x = x + 0.0
        x = torch.round(x)
        x = torch.clamp(x, 0.0, 255.0)
        target.copy_(x.to(torch.uint8))

    def single_expression():
        target.copy_(tensor.mul(255.0).add_(0.0).round_().clamp_(0.0, 255.0).to(torch.uint8))

    def rgba():
        r, u, res = ctx.encode_frames_rgba(pic_list, w, h, w * 4, fmts, comps, chunks, outs, flags=flags)
        assert r == 0 and not any(res), (r, res)
        used["rgba"] = u

    res = {"planes": channels, "element": "float16", "tensor_bytes": tensor.numel() * 2,
           "picture_bytes_the_detour_holds": pics.numel()}
    res["planes_ms"] = median_ms(planes, reps)
    torch_ms = {"as_written": median_ms(as_written, reps), "single_expression": median_ms(single_expression, reps)}
    convert = as_written if torch_ms["as_written"] <= torch_ms["single_expression"] else single_expression
    torch.cuda.empty_cache()

    def detour():
        convert()
        rgba()

    res["torch_ms"] = torch_ms
    res["rgba_ms"] = median_ms(rgba, reps)
    res["torch_then_rgba_ms"] = median_ms(detour, reps)
    res["planes_over_torch_then_rgba"] = round(res["planes_ms"] / res["torch_then_rgba_ms"], 3)
    res["frame_bytes"] = {k: int(sum(v)) for k, v in used.items()}
    kernel = class_ms(ctx, planes, reps, "block_encode")
    moved = tensor.numel() * 2 + count * sum(sizes)
    res["block_encode_ms"] = round(kernel, 4)
    res["block_encode_bytes"] = moved
    res["block_encode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    res["encode_fused_ms_of_the_rgba_call"] = round(class_ms(ctx, rgba, reps, "encode_fused"), 4)
    res["block_encode_ms_of_the_rgba_call"] = round(class_ms(ctx, rgba, reps, "block_encode"), 4)
    # both routes computed the same thing: the definition's bytes of the first tensor against the torch path's picture
    x = tensor[0].to(torch.float32) * 255.0
    want = torch.where(torch.isnan(x), torch.zeros_like(x), torch.round(x).clamp(0.0, 255.0)).to(torch.uint8)
    res["max_byte_difference_from_the_torch_path"] = int((want.to(torch.int16) - target[0].to(torch.int16)).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_encode.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "planes_encode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS}
    for name, w, h, count, fmts, flag in WORKLOADS:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        tensor = make_tensor(w, h, count, 2 + len(fmts))
        res[name] = {"geometry": [w, h], "tensors": count, "formats": list(fmts), "flags": flag or "none"}
        res[name].update(one_case(ctx, tensor, w, h, fmts, hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0, args.reps))
        print("%s: done" % name, file=sys.stderr, flush=True)
        del tensor
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

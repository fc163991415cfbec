"""GPU timing of the video decode call (HapGpuDecodeFramesNV12) against the path a client has without it:
HapGpuDecodeFramesRGBA[Scaled] into RGBA8 pictures, and then torch -- the same integer RGB -> YCbCr conversion, exact,
every pair from the sums of its 2 x 2 texels, into preallocated planes.

    python tools/nv12_decode_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames, pictures and planes in HBM, frames made here from hap_amd.synth pictures (four distinct ones; 16
Snappy chunks a texture; BT.709, limited range):

  hap_q_8k_x60, hap_q_8k_x60_table             60 Hap Q frames, 7680 x 4320, plain / with the fragment table, s = 0
  hap_q_8k_x60_half, hap_q_8k_x60_table_half   the same at s = 1 (3840 x 2160 pictures)
  hap_4k_x60                                   60 Hap frames, 3840 x 2160
  hap_q_alpha_16k_x4                           4 Hap Q Alpha frames, 15360 x 8640, textureCount 2

Per workload, medians of N calls after warm-up between HIP events (every route ends with the host waiting, so the events
bracket all of it), in one process:

  nv12_ms                the one call
  rgba_ms                (a) HapGpuDecodeFramesRGBA[Scaled] alone
  rgba_then_torch_ms     (b) that call and then torch; its torch half in three exact forms, the fastest being the baseline
  torch_ms               the torch half by itself, per form
  block_decode_ms        the block-decode kernel's own time in the one call, by profile class, and its fraction of HBM
                         peak from the bytes it must move: the source blocks read, 24 written a destination block

The torch forms compute the definition's integers: their planes must equal the call's exactly (checked on every
picture).  Prints one JSON line.
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
HBM_PEAK_GBS = 8000.0
CHUNKS = 16
# BT.709 limited: yr, yg, yb, cbr, cbg, ch, crg, crb, lo (include/hap_gpu.h: HapGpuDecompressNV12)
YR, YG, YB, CBR, CBG, CH, CRG, CRB, LO = 11966, 40254, 4064, 6596, 22188, 28784, 26145, 2639, 16
BIAS = (128 << 18) + (1 << 17)
# name, width, height, frames, texture formats, fragment table, scale
WORKLOADS = (
    ("hap_q_8k_x60", 7680, 4320, 60, (FMT_YCOCG,), False, 0),
    ("hap_q_8k_x60_table", 7680, 4320, 60, (FMT_YCOCG,), True, 0),
    ("hap_q_8k_x60_half", 7680, 4320, 60, (FMT_YCOCG,), False, 1),
    ("hap_q_8k_x60_table_half", 7680, 4320, 60, (FMT_YCOCG,), True, 1),
    ("hap_4k_x60", 3840, 2160, 60, (FMT_DXT1,), False, 0),
    ("hap_q_alpha_16k_x4", 15360, 8640, 4, (FMT_YCOCG, FMT_RGTC1), False, 0),
)


def make_frames(ctx, w, h, count, fmts, table):
    """`count` frames on the device, four distinct ones among them"""
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))
    distinct = min(count, 4)
    pics = [synth.rgba_frame(w, h, i, device="cuda") for i in range(distinct)]
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(distinct)]
    torch.cuda.synchronize()
    r, used, res = ctx.encode_frames_rgba(pics, w, h, w * 4, list(fmts), [1] * len(fmts), [CHUNKS] * len(fmts), outs,
                                          flags=hap_amd.ENCODE_FRAGMENT_INDEX if table else 0)
    assert r == 0 and not any(res), (r, res)
    frames = [outs[i][: used[i]].clone() for i in range(distinct)]
    del pics, outs
    torch.cuda.empty_cache()
    return [frames[i % distinct] for i in range(count)], [int(used[i % distinct]) for i in range(count)]


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


def converters(pics, luma, chroma):
    """The exact integer conversion of `pics` (count, H, W, 4) into luma (count, H, W) and chroma (count, H / 2, W),
    three ways"""
    count, h, w, _four = pics.shape
    pairs = chroma.view(count, h // 2, w // 2, 2)

    def samples(p, y_out, pair_out, sums):
        rgb = p[..., :3].to(torch.int32)
        y_out.copy_(((YR * rgb[..., 0] + YG * rgb[..., 1] + YB * rgb[..., 2] + 32768) >> 16) + LO)
        s = sums(rgb)
        rs, gs, bs = s[..., 0], s[..., 1], s[..., 2]
        pair_out[..., 0].copy_(((CH * bs - CBR * rs - CBG * gs + BIAS) >> 18).clamp_(0, 255))
        pair_out[..., 1].copy_(((CH * rs - CRG * gs - CRB * bs + BIAS) >> 18).clamp_(0, 255))

    def reshaped(rgb):
        lead = rgb.shape[:-3]
        return rgb.view(*lead, h // 2, 2, w // 2, 2, 3).sum(dim=(-4, -2))

    def strided(rgb):
        return rgb[..., 0::2, 0::2, :] + rgb[..., 0::2, 1::2, :] + rgb[..., 1::2, 0::2, :] + rgb[..., 1::2, 1::2, :]

    def reshape_sum():
        samples(pics, luma, pairs, reshaped)

    def strided_adds():
        samples(pics, luma, pairs, strided)

    def frame_by_frame():
        for f in range(count):
            samples(pics[f], luma[f], pairs[f], strided)

    return {"reshape_sum": reshape_sum, "strided_adds": strided_adds, "frame_by_frame": frame_by_frame}


def one_case(ctx, w, h, count, fmts, table, s, reps):
    frames, lens = make_frames(ctx, w, h, count, fmts, table)
    ow, oh = w >> s, h >> s
    luma = torch.zeros((count, oh, ow), dtype=torch.uint8, device="cuda")
    chroma = torch.zeros((count, oh // 2, ow), dtype=torch.uint8, device="cuda")
    luma2, chroma2 = torch.zeros_like(luma), torch.zeros_like(chroma)
    pics = torch.zeros((count, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pic_list = [pics[i] for i in range(count)]
    # (addresses, as a C client has them: the wrapper then slices no tensor per frame and call)
    luma_at, chroma_at = [luma[i].data_ptr() for i in range(count)], [chroma[i].data_ptr() for i in range(count)]
    torch.cuda.synchronize()

    def nv12():
        r, res = ctx.decode_frames_nv12(frames, lens, len(fmts), luma_at, chroma_at, w, h, scale_log2=s,
                                        matrix=hap_amd.YCBCR_BT709, range=hap_amd.YCBCR_LIMITED, luma_row_bytes=ow,
                                        chroma_row_bytes=ow)
        assert r == 0 and not any(res), (r, res)

    def rgba():
        if s == 0:
            r, res = ctx.decode_frames_rgba(frames, lens, len(fmts), pic_list, w, h)
        else:
            r, res = ctx.decode_frames_rgba_scaled(frames, lens, len(fmts), pic_list, w, h, s)
        assert r == 0 and not any(res), (r, res)

    forms = converters(pics, luma2, chroma2)
    res = {"frame_bytes": int(sum(lens)), "plane_bytes": luma.numel() + chroma.numel(),
           "picture_bytes_the_detour_holds": pics.numel()}
    res["nv12_ms"] = median_ms(nv12, reps)
    res["rgba_ms"] = median_ms(rgba, reps)
    torch_ms, equal = {}, True
    for name, form in forms.items():
        luma2.zero_()
        chroma2.zero_()
        torch_ms[name] = median_ms(form, reps)
        # the form computed the definition: the call's planes, exactly
        equal = equal and torch.equal(luma, luma2) and torch.equal(chroma, chroma2)
        torch.cuda.empty_cache()
    convert = forms[min(torch_ms, key=torch_ms.get)]

    def detour():
        rgba()
        convert()

    res["torch_ms"] = torch_ms
    res["planes_equal"] = bool(equal)
    res["rgba_then_torch_ms"] = median_ms(detour, reps)
    res["nv12_over_rgba_then_torch"] = round(res["nv12_ms"] / res["rgba_then_torch_ms"], 3)
    res["nv12_over_rgba"] = round(res["nv12_ms"] / res["rgba_ms"], 3)
    kernel = class_ms(ctx, nv12, reps, "block_decode")
    moved = count * ((w // 4) * (h // 4) * BLOCK_BYTES[fmts[0]] + (ow // 4) * (oh // 4) * 24)
    res["block_decode_ms"] = round(kernel, 4)
    res["block_decode_bytes"] = moved
    res["block_decode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    res["block_decode_ms_of_the_rgba_call"] = round(class_ms(ctx, rgba, reps, "block_decode"), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nv12_decode.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide every geometry's sides by this")
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nv12_decode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS, "matrix": "BT.709", "range": "limited"}
    for name, w, h, count, fmts, table, s in WORKLOADS:
        if args.only and name not in args.only.split(","):
            continue
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        res[name] = {"geometry": [w, h], "frames": count, "formats": list(fmts), "table": table, "scale_log2": s}
        res[name].update(one_case(ctx, w, h, count, fmts, table, s, args.reps))
        print("%s: done" % name, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

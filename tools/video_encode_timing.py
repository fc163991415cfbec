"""GPU timing of the video encode call (HapGpuEncodeFramesNV12) against the path a client has without it: torch -- the
same integer YCbCr -> RGB conversion, exact, chroma replicated 2 x 2, into a preallocated RGBA8 batch whose alpha is 255
-- and then HapGpuEncodeFramesRGBA of those pictures, fused compress kernel included.

    python tools/video_encode_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, planes and frames in HBM, NV12 pictures made here from hap_amd.synth pictures (BT.709, limited range; 16 Snappy
chunks a texture):

  hap_q_8k_x60, hap_q_8k_x60_table     60 NV12 pictures, 7680 x 4320 -> Hap Q frames, plain / with the fragment table
  hap_8k_x60, hap_8k_x60_table         the same                      -> Hap frames
  hap_q_4k_x60 ... hap_4k_x60_table    60 NV12 pictures, 3840 x 2160, the same four ways

Per workload, medians of N calls after warm-up between HIP events (every route ends with the host waiting, so the events
bracket all of it), in one process:

  nv12_ms                the one call
  torch_then_rgba_ms     the detour; its torch half in three exact forms, the fastest being the baseline
  torch_ms, rgba_ms      the detour's two halves by themselves
  block_encode_ms        the block-encode kernel's own time in the one call, by profile class, and its fraction of HBM
                         peak from the bytes it must move: 24 read and 8 (Hap) or 16 (Hap Q) written a block; beside it
                         the planar kernel's recorded time for 60 8K tensors (profiles/planes_encode.json)

The torch forms compute the definition's integers: their pictures must equal the call's definition exactly (checked on
the first picture), and the frames of both routes must be the same bytes (checked on the first frame).  Prints one JSON
line.
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

FMT_DXT1, FMT_YCOCG = 0x83F0, 0x01
BLOCK_BYTES = {FMT_DXT1: 8, FMT_YCOCG: 16}
HBM_PEAK_GBS = 8000.0
CHUNKS = 16
# BT.709 limited: cy, crv, cbu, cgu, cgv, luma offset (include/hap_gpu.h: HapGpuCompressNV12)
CY, CRV, CBU, CGU, CGV, OFFSET = 76309, 117489, 138438, 13975, 34925, 16
GEOMETRIES = (("8k", 7680, 4320), ("4k", 3840, 2160))
FLAVOURS = (("hap_q", FMT_YCOCG), ("hap", FMT_DXT1))
COUNT = 60


def make_nv12(w, h, count):
    """(count, h, w) Y and (count, h / 2, w) CbCr bytes from the synthetic pictures (four distinct ones): BT.709, limited
    range, chroma the mean of its 2 x 2 samples -- a video's planes, however they were made"""
    luma = torch.empty((count, h, w), dtype=torch.uint8, device="cuda")
    chroma = torch.empty((count, h // 2, w), dtype=torch.uint8, device="cuda")
    for i in range(min(count, 4)):
        rgb = synth.rgba_frame(w, h, i, device="cuda")[..., :3].to(torch.float32)
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        y = 0.2126 * r + 0.7152 * g + 0.0722 * b
        luma[i].copy_((16.0 + y * (219.0 / 255.0)).round().clamp(0, 255).to(torch.uint8))
        cb = ((b - y) / 1.8556 * (224.0 / 255.0) + 128.0).reshape(h // 2, 2, w // 2, 2).mean(dim=(1, 3))
        cr = ((r - y) / 1.5748 * (224.0 / 255.0) + 128.0).reshape(h // 2, 2, w // 2, 2).mean(dim=(1, 3))
        pairs = chroma[i].view(h // 2, w // 2, 2)
        pairs[..., 0].copy_(cb.round().clamp(0, 255).to(torch.uint8))
        pairs[..., 1].copy_(cr.round().clamp(0, 255).to(torch.uint8))
        del rgb, r, g, b, y, cb, cr
    for i in range(4, count):
        luma[i].copy_(luma[i % 4])
        chroma[i].copy_(chroma[i % 4])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return luma, chroma


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


def converters(luma, chroma, pics):
    """The exact integer conversion into `pics` (count, h, w, 4; alpha stays 255), three ways"""
    count, h, w = luma.shape
    pairs = chroma.view(count, h // 2, w // 2, 2)
    quads = pics.view(count, h // 2, 2, w // 2, 2, 4)

    def terms(uv):
        u, v = uv[..., 0].to(torch.int32) - 128, uv[..., 1].to(torch.int32) - 128
        return CRV * v + 32768, 32768 - CGU * u - CGV * v, CBU * u + 32768

    def upsampled():
        l = (luma.to(torch.int32) - OFFSET) * CY
        for c, t in enumerate(terms(pairs)):
            t = t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            pics[..., c].copy_(((l + t) >> 16).clamp_(0, 255))

    def broadcast():
        l = ((luma.to(torch.int32) - OFFSET) * CY).view(count, h // 2, 2, w // 2, 2)
        for c, t in enumerate(terms(pairs)):
            quads[..., c].copy_(((l + t[:, :, None, :, None]) >> 16).clamp_(0, 255))

    def frame_by_frame():
        for f in range(count):
            l = ((luma[f].to(torch.int32) - OFFSET) * CY).view(h // 2, 2, w // 2, 2)
            for c, t in enumerate(terms(pairs[f])):
                quads[f, ..., c].copy_(((l + t[:, None, :, None]) >> 16).clamp_(0, 255))

    return {"upsampled": upsampled, "broadcast": broadcast, "frame_by_frame": frame_by_frame}


def one_case(ctx, luma, chroma, pics, w, h, fmt, flags, reps, torch_ms):
    count = luma.shape[0]
    size = (w // 4) * (h // 4) * BLOCK_BYTES[fmt]
    cap = hap_amd.HapMaxEncodedLength([size], [fmt], [CHUNKS])
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)]
    outs2 = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)]
    pic_list = [pics[i] for i in range(count)]
    forms = converters(luma, chroma, pics)
    torch.cuda.synchronize()
    used = {}

    def nv12():
        r, u, res = ctx.encode_frames_nv12(luma, chroma, w, h, [fmt], [1], [CHUNKS], outs, matrix=hap_amd.YCBCR_BT709,
                                           range=hap_amd.YCBCR_LIMITED, flags=flags)
        assert r == 0 and not any(res), (r, res)
        used["nv12"] = u

    def rgba():
        r, u, res = ctx.encode_frames_rgba(pic_list, w, h, w * 4, [fmt], [1], [CHUNKS], outs2, flags=flags)
        assert r == 0 and not any(res), (r, res)
        used["rgba"] = u

    res = {"plane_bytes": luma.numel() + chroma.numel(), "picture_bytes_the_detour_holds": pics.numel()}
    res["nv12_ms"] = median_ms(nv12, reps)
    if not torch_ms:
        # (the conversion does not depend on the destination: timed once per geometry)
        for name, form in forms.items():
            torch_ms[name] = median_ms(form, reps)
            torch.cuda.empty_cache()
    convert = forms[min(torch_ms, key=torch_ms.get)]

    def detour():
        convert()
        rgba()

    res["torch_ms"] = dict(torch_ms)
    res["rgba_ms"] = median_ms(rgba, reps)
    res["torch_then_rgba_ms"] = median_ms(detour, reps)
    res["nv12_over_torch_then_rgba"] = round(res["nv12_ms"] / res["torch_then_rgba_ms"], 3)
    res["nv12_over_rgba"] = round(res["nv12_ms"] / res["rgba_ms"], 3)
    res["frame_bytes"] = {k: int(sum(v)) for k, v in used.items()}
    kernel = class_ms(ctx, nv12, reps, "block_encode")
    moved = luma.numel() + chroma.numel() + count * size
    res["block_encode_ms"] = round(kernel, 4)
    res["block_encode_bytes"] = moved
    res["block_encode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    res["encode_fused_ms_of_the_rgba_call"] = round(class_ms(ctx, rgba, reps, "encode_fused"), 4)
    res["block_encode_ms_of_the_rgba_call"] = round(class_ms(ctx, rgba, reps, "block_encode"), 4)
    # both routes computed the same thing: the same frame bytes
    res["frames_equal"] = bool(used["nv12"] == used["rgba"] and
                               torch.equal(outs[0][: used["nv12"][0]], outs2[0][: used["rgba"][0]]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_encode.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    ap.add_argument("--count", type=int, default=COUNT, help="pictures a workload")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "video_encode_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS, "matrix": "BT.709", "range": "limited"}
    recorded = os.path.join(ROOT, "profiles", "planes_encode.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            res["planar_block_encode_ms_recorded_hap_q_8k_x60"] = json.load(f).get("hap_q_8k_x60", {}).get("block_encode_ms")
    for geometry, w, h in GEOMETRIES:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        luma, chroma = make_nv12(w, h, args.count)
        pics = torch.full((args.count, h, w, 4), 255, dtype=torch.uint8, device="cuda")
        torch_ms = {}
        for flavour, fmt in FLAVOURS:
            for flag in ("", "index"):
                name = "%s_%s_x%d%s" % (flavour, geometry, args.count, "_table" if flag else "")
                res[name] = {"geometry": [w, h], "pictures": args.count, "format": fmt, "flags": flag or "none"}
                res[name].update(one_case(ctx, luma, chroma, pics, w, h, fmt,
                                          hap_amd.ENCODE_FRAGMENT_INDEX if flag else 0, args.reps, torch_ms))
                print("%s: done" % name, file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        del luma, chroma, pics
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

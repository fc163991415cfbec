"""GPU timing of the compositing call (HapGpuCompositeFrames) against the path a client has without it:
HapGpuDecodeFramesRGBA once per layer into device pictures, then torch -- the blend of the definition, exact, over those
pictures -- into the output pictures.

    python tools/composite_timing.py [--reps N] [--out FILE] [--shrink K]

Workloads, frames and pictures in HBM, sources made here from hap_amd.synth pictures with a sloped alpha channel
(16 chunks a texture); layers are listed bottom to top, opacities change from output frame to output frame:

  q_alpha_over_q_8k_x60          60 output frames of 7680 x 4320: Hap Q Alpha over Hap Q, hap.h sections only
  q_alpha_over_q_8k_x60_table    the same with the fragment table (ENCODE_FRAGMENT_INDEX)
  three_layers_8k_x20            20 output frames of 7680 x 4320: Hap Q, Hap Alpha, Hap Q Alpha
  q_alpha_over_q_alpha_16k_x4    4 output frames of 15360 x 8640: Hap Q Alpha over Hap Q Alpha

Per workload, medians of N calls after warm-up between HIP events (every route ends with the host waiting, so the events
bracket all of it), in one process:

  composite_ms           (a) the one call
  rgba_then_torch_ms     (b) decode_frames_rgba per layer, then one of the torch expressions for the blend; the fastest is
                         the baseline and is named
  rgba_ms                (c) decode_frames_rgba per layer alone
  block_decode_ms        the block kernels' own time in (a) and in (c), by profile class, and (a)'s fraction of HBM peak
                         from the bytes it must move: per block every layer's 16 (+ 8) bytes read and 64 written

The pictures of (a) must equal those of (b) for every output frame and every expression, or the tool fails.  A report,
not a pass criterion.  Prints one JSON line.
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

FMT_DXT5, FMT_YCOCG, FMT_RGTC1 = 0x83F3, 0x01, 0x8DBB
BLOCK_BYTES = {FMT_DXT5: 16, FMT_YCOCG: 16, FMT_RGTC1: 8}
HBM_PEAK_GBS = 8000.0
HAP_Q, HAP_ALPHA, HAP_Q_ALPHA = (FMT_YCOCG,), (FMT_DXT5,), (FMT_YCOCG, FMT_RGTC1)
# name, width, height, output frames, layers (bottom to top, each its frames' texture formats), encode flags of the sources
WORKLOADS = (("q_alpha_over_q_8k_x60", 7680, 4320, 60, (HAP_Q, HAP_Q_ALPHA), ""),
             ("q_alpha_over_q_8k_x60_table", 7680, 4320, 60, (HAP_Q, HAP_Q_ALPHA), "index"),
             ("three_layers_8k_x20", 7680, 4320, 20, (HAP_Q, HAP_ALPHA, HAP_Q_ALPHA), ""),
             ("q_alpha_over_q_alpha_16k_x4", 15360, 8640, 4, (HAP_Q_ALPHA, HAP_Q_ALPHA), ""))
CHUNKS = 16
BACKGROUND = (17, 34, 51, 128)


def source_pictures(w, h, layer):
    """four distinct pictures for a layer, alpha sloped across the picture so that every blend weight occurs"""
    y = torch.arange(h, dtype=torch.int64, device="cuda").view(-1, 1)
    x = torch.arange(w, dtype=torch.int64, device="cuda").view(1, -1)
    out = []
    for i in range(4):
        p = synth.rgba_frame(w, h, 4 * layer + i, device="cuda").clone()
        p[:, :, 3] = ((x * (3 + layer) + y * (5 + i)) >> 3).to(torch.uint8)
        out.append(p)
    return out


def make_frames(ctx, w, h, count, fmts, flags, layer):
    """(frames, their sizes) of one layer: one frame per output frame"""
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))
    distinct = source_pictures(w, h, layer)
    frames, used = [], []
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
    del distinct
    torch.cuda.empty_cache()
    return frames, used


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


# The blend of one output frame from its layers' decoded pictures ([H, W, 4] uint8 in HBM, bottom to top), their
# opacities and the background, into out ([H, W, 4] uint8).  All exact to the definition; the tool checks that they are.
def rdiv255(x):
    t = x + 128
    return (t + (t >> 8)) >> 8


def blend_int32_by_channel_group(layers, opacities, background, out):
    canvas = torch.tensor(background, dtype=torch.int32, device=out.device).expand(out.shape).clone()
    for picture, o in zip(layers, opacities):
        s = picture.to(torch.int32)
        a = rdiv255(s[:, :, 3:4] * o)
        inv = 255 - a
        colour = rdiv255(s[:, :, :3] * a + canvas[:, :, :3] * inv)
        alpha = a + rdiv255(canvas[:, :, 3:4] * inv)
        canvas = torch.cat((colour, alpha), dim=2)
    out.copy_(canvas)


def blend_int32_four_channels(layers, opacities, background, out):
    # (the canvas's alpha as a fourth colour whose source is 255: rdiv255(255 a + y) = a + rdiv255(y))
    canvas = torch.tensor(background, dtype=torch.int32, device=out.device).expand(out.shape).clone()
    for picture, o in zip(layers, opacities):
        s = picture.to(torch.int32)
        a = rdiv255(s[:, :, 3:4] * o)
        s[:, :, 3] = 255
        canvas = rdiv255(s * a + canvas * (255 - a))
    out.copy_(canvas)


def blend_float32_four_channels(layers, opacities, background, out):
    # (every product and sum is an integer below 2^24, and floor((2 x + 255) / 510) is rdiv255(x): the quotient is an
    # integer or at least 1 / 510 away from one)
    def nearest(x):
        return torch.floor((2.0 * x + 255.0) / 510.0)
    canvas = torch.tensor(background, dtype=torch.float32, device=out.device).expand(out.shape).clone()
    for picture, o in zip(layers, opacities):
        s = picture.to(torch.float32)
        a = nearest(s[:, :, 3:4] * float(o))
        s[:, :, 3] = 255.0
        canvas = nearest(s * a + canvas * (255.0 - a))
    out.copy_(canvas)


EXPRESSIONS = {"int32_by_channel_group": blend_int32_by_channel_group, "int32_four_channels": blend_int32_four_channels,
               "float32_four_channels": blend_float32_four_channels}


def one_case(ctx, layer_frames, layer_used, layer_formats, w, h, count, reps):
    layers = len(layer_formats)
    counts = [len(f) for f in layer_formats]
    opacities = [[255 if l == 0 else (37 + 211 * f // max(1, count - 1) + 50 * l) % 256 for l in range(layers)]
                 for f in range(count)]
    frames = [[layer_frames[l][f] for l in range(layers)] for f in range(count)]
    sizes = [[layer_used[l][f] for l in range(layers)] for f in range(count)]
    out = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    check = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    decoded = [torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(layers)]
    out_list, check_list = [out[i] for i in range(count)], [check[i] for i in range(count)]
    torch.cuda.synchronize()

    def composite():
        r, res = ctx.composite_frames(frames, sizes, counts, out_list, w, h, opacities=opacities, background=BACKGROUND)
        assert r == 0 and not any(res), (r, res)

    def rgba():
        for l in range(layers):
            r, res = ctx.decode_frames_rgba(layer_frames[l], layer_used[l], counts[l], [decoded[l][i] for i in range(count)],
                                            w, h)
            assert r == 0 and not any(res), (r, res)

    def rgba_then(expression):
        def call():
            rgba()
            for f in range(count):
                EXPRESSIONS[expression]([decoded[l][f] for l in range(layers)], opacities[f], BACKGROUND, check_list[f])
            torch.cuda.synchronize()
        return call

    blocks = (w // 4) * (h // 4)
    read = sum(sum(BLOCK_BYTES[f] for f in fmts) for fmts in layer_formats)
    moved = count * blocks * (read + 64)
    res = {"layers": layers, "texture_counts": counts,
           "picture_bytes_the_torch_path_holds": layers * count * w * h * 4, "output_picture_bytes": count * w * h * 4}
    res["composite_ms"] = timed_ms(composite, reps)
    res["rgba_ms"] = timed_ms(rgba, reps)
    res["rgba_then_torch_ms"] = {}
    for expression in EXPRESSIONS:
        res["rgba_then_torch_ms"][expression] = timed_ms(rgba_then(expression), reps)
        # the tool's own sanity: the pictures of (a) are those of (b), for every output frame and every expression
        assert torch.equal(out, check), expression
        check.zero_()
        torch.cuda.empty_cache()
    res["pictures_equal_the_torch_blend"] = True
    fastest = min(res["rgba_then_torch_ms"], key=lambda k: res["rgba_then_torch_ms"][k][0])
    res["fastest_torch_expression"] = fastest
    res["composite_over_rgba"] = round(res["composite_ms"][0] / res["rgba_ms"][0], 3)
    res["composite_over_rgba_then_torch"] = round(res["composite_ms"][0] / res["rgba_then_torch_ms"][fastest][0], 3)
    kernel = block_decode_ms(ctx, composite, reps)
    res["block_decode_ms"] = round(kernel, 4)
    res["block_decode_ms_of_the_rgba_calls"] = round(block_decode_ms(ctx, rgba, reps), 4)
    res["block_decode_bytes"] = moved
    res["block_decode_of_hbm_peak"] = round(moved / (kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kernel > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide both geometries' sides by this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "composite_timing.py needs a GPU"
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "hbm_peak_GBps": HBM_PEAK_GBS, "times": "[median, min, max] ms", "background": list(BACKGROUND)}
    for name, w, h, count, layer_formats, flag in WORKLOADS:
        w, h = w // args.shrink // 16 * 16, h // args.shrink // 16 * 16
        flags = hap_amd.ENCODE_FRAGMENT_INDEX if flag == "index" else 0
        made = [make_frames(ctx, w, h, count, fmts, flags, l) for l, fmts in enumerate(layer_formats)]
        res[name] = {"geometry": [w, h], "output_frames": count, "layer_formats": [list(f) for f in layer_formats],
                     "source_flags": flag or "none", "frame_bytes_per_step": sum(sum(u) for _f, u in made)}
        res[name].update(one_case(ctx, [f for f, _u in made], [u for _f, u in made], layer_formats, w, h, count, args.reps))
        print("%s: done" % name, file=sys.stderr, flush=True)
        del made
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

"""GPU timing of compositing straight to frames (HapGpuCompositeFramesEncoded) against the two-call route it replaces:
HapGpuCompositeFramesPlaced into RGBA8 pictures in device memory, then HapGpuEncodeFramesRGBA of those pictures.

    python tools/composite_encode_timing.py [--reps N] [--out FILE] [--shrink K] [--frames N] [--only WORKLOAD]

Workloads, frames and pictures in HBM, sources made here from hap_amd.synth pictures with a sloped alpha channel, Snappy,
16 chunks a texture, each with and without HAPGPU_ENCODE_FRAGMENT_INDEX:

  over              60 output frames of 7680 x 4320: Hap Q Alpha over Hap Q at an opacity that changes from frame to
                    frame, to Hap Q
  stack             20 output frames of 7680 x 4320: Hap Alpha over Hap Q Alpha over Hap Q, to Hap Q Alpha
  mosaic            60 output frames of 3840 x 2160: sixteen 1920 x 1080 Hap clips in a 4 x 4 grid, a centred 960 x 540
                    window of each, to Hap

Per workload and flag, [median, min, max] ms of N calls after warm-up between HIP events (both routes end with the host
waiting, so the events bracket all of it), in one process, the two routes interleaved.  The frames of the one call must
equal the two-call route's byte for byte, or the tool fails.  The ratios are a report, not a pass criterion: the two-call
route ends in the fused encode kernel, this one runs the block encoder as a pass of its own in front of the compressor,
and what it certainly saves is the pictures' 64 written and 64 read bytes per block, and their memory.

Prints one JSON line, and writes it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import hap_amd  # noqa: E402
from composite_placed_timing import BLOCK_BYTES, CHUNKS, HAP, HAP_Q, HAP_Q_ALPHA, FMT_DXT5, make_frames, ratio  # noqa: E402
from composite_timing import timed_ms  # noqa: E402

HAP_ALPHA = (FMT_DXT5,)
SNAPPY = 1
CANVAS = (7680, 4320)
FLAGS = (("plain", 0), ("fragment_index", hap_amd.ENCODE_FRAGMENT_INDEX))


def both_routes(ctx, name, layers, sizes, placements, opacities, canvas, count, dst, reps):
    """layers: per layer (its formats, (w, h)); one frame of each per output frame.  The timings of both routes, per flag"""
    w, h = canvas
    made = [make_frames(ctx, lw, lh, count, fmts, l) for l, (fmts, (lw, lh)) in enumerate(layers)]
    n = len(layers)
    frames = [[made[l][0][f] for l in range(n)] for f in range(count)]
    lens = [[made[l][1][f] for l in range(n)] for f in range(count)]
    counts = [len(fmts) for fmts, _s in layers]
    out_sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in dst]
    cap = hap_amd.HapMaxEncodedLength(out_sizes, list(dst), [CHUNKS] * len(dst))
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)]
    check = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(count)]
    pictures = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    comps, chunks = [SNAPPY] * len(dst), [CHUNKS] * len(dst)
    used = {}
    res = {"canvas": [w, h], "output_frames": count, "layer_formats": [list(f) for f, _s in layers],
           "layer_sizes": [list(s) for _f, s in layers], "destination": list(dst),
           "picture_bytes_of_the_two_call_route": int(pictures.numel())}
    for flag_name, flags in FLAGS:
        def one_call():
            r, u, results, layer_results = ctx.composite_frames_encoded(frames, lens, counts, sizes, w, h, list(dst), comps, chunks,
                                                                        outs, placements=placements, opacities=opacities,
                                                                        encode_flags=flags)
            assert r == 0 and not any(results) and not any(layer_results), (r, results, layer_results)
            used["one"] = u

        def two_calls():
            r, results = ctx.composite_frames_placed(frames, lens, counts, sizes, list(pictures), w, h, placements=placements,
                                                     opacities=opacities)
            assert r == 0 and not any(results), (r, results)
            r, u, results = ctx.encode_frames_rgba(list(pictures), w, h, w * 4, list(dst), comps, chunks, check, flags=flags)
            assert r == 0 and not any(results), (r, results)
            used["two"] = u

        # (interleaved: one, two, one, two -- two medians each, so that drift shows)
        t = {"one_call_ms": timed_ms(one_call, reps), "two_calls_ms": timed_ms(two_calls, reps),
             "one_call_again_ms": timed_ms(one_call, reps), "two_calls_again_ms": timed_ms(two_calls, reps)}
        assert used["one"] == used["two"], "%s: the frames' sizes differ from the two-call route's" % name
        for f in range(count):
            assert torch.equal(outs[f][: used["one"][f]], check[f][: used["two"][f]]), \
                "%s: output frame %d differs from the two-call route's" % (name, f)
        t["frames_equal"] = True
        t["frame_bytes"] = int(sum(used["one"]))
        t["one_call_over_two_calls"] = ratio(t["one_call_ms"], t["two_calls_ms"])
        t["one_call_again_over_two_calls_again"] = ratio(t["one_call_again_ms"], t["two_calls_again_ms"])
        for which, call in (("one_call", one_call), ("two_calls", two_calls)):
            ctx.set_profiling(True)
            ctx.collect_profile()
            call()
            prof = ctx.collect_profile()
            ctx.set_profiling(False)
            t["kernel_ms_of_" + which] = {k: round(v[1], 4) for k, v in prof.items() if v[0]}
        res[flag_name] = t
    return res


def over(ctx, w, h, count, reps):
    layers = [(HAP_Q, (w, h)), (HAP_Q_ALPHA, (w, h))]
    opacities = [[255, (37 + 211 * f // max(1, count - 1)) % 256] for f in range(count)]
    return both_routes(ctx, "over", layers, [(w, h)] * 2, None, opacities, (w, h), count, HAP_Q, reps)


def stack(ctx, w, h, count, reps):
    layers = [(HAP_Q, (w, h)), (HAP_Q_ALPHA, (w, h)), (HAP_ALPHA, (w, h))]
    opacities = [[255, 200, (90 + 7 * f) % 256] for f in range(count)]
    return both_routes(ctx, "stack", layers, [(w, h)] * 3, None, opacities, (w, h), count, HAP_Q_ALPHA, reps)


def mosaic(ctx, w, h, tw, th, count, reps):
    """a centred (w / 4) x (h / 4) window of each of sixteen tw x th clips"""
    ww, wh = w // 4, h // 4
    sx, sy = (tw - ww) // 2 // 4 * 4, (th - wh) // 2 // 4 * 4
    layers = [(HAP, (tw, th))] * 16
    placements = [[(sx, sy, ww, wh, ww * (l % 4), wh * (l // 4)) for l in range(16)]] * count
    return both_routes(ctx, "mosaic", layers, [(tw, th)] * 16, placements, None, (w, h), count, HAP, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=60, help="output frames of `over` and `mosaic`; `stack` has a third of them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_encode.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide every geometry's sides by this")
    ap.add_argument("--only", choices=("over", "stack", "mosaic"), action="append", help="these workloads alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "composite_encode_timing.py needs a GPU"
    w, h = (v // args.shrink // 16 * 16 for v in CANVAS)
    if args.shrink == 1:
        assert (w, h) == (7680, 4320)
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "times": "[median, min, max] ms", "compressor": "snappy", "chunks": CHUNKS}
    for name in args.only or ["over", "stack", "mosaic"]:
        if name == "over":
            res[name] = over(ctx, w, h, args.frames, args.reps)
        elif name == "stack":
            res[name] = stack(ctx, w, h, max(1, args.frames // 3), args.reps)
        else:
            res[name] = mosaic(ctx, w // 2, h // 2 // 16 * 16, w // 4, h // 4 // 4 * 4, args.frames, args.reps)
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

"""GPU timing of the placed compositing call (HapGpuCompositeFramesPlaced) against what a client has without it, and of the
existing call (HapGpuCompositeFrames) against itself in the parent commit's build.

    python tools/composite_placed_timing.py [--reps N] [--out FILE] [--shrink K] [--frames N]
                                            [--parent-root DIR --parent-out FILE] [--only WORKLOAD]

Workloads, frames and pictures in HBM, sources made here from hap_amd.synth pictures with a sloped alpha channel
(16 chunks a texture), 60 output frames of 7680 x 4320 each:

  full_size         (A) Hap Q Alpha over Hap Q, both of the canvas's size, placements None: the placed call against
                    composite_frames on the same inputs -- what the clip test costs where it decides nothing
  inset             (B) a Hap Q background with a 1920 x 1080 Hap Q Alpha inset at opacity 200: against decode_frames_rgba
                    of the background into the canvases and of the inset into pictures of its own, then the fastest exact
                    torch blend of the sub-rectangle
  mosaic            (C) sixteen 1920 x 1080 Hap layers in a 4 x 4 grid: against sixteen decode_frames_rgba calls that
                    write their tiles straight into the canvases through rowBytes

Per workload, [median, min, max] ms of N calls after warm-up between HIP events (every route ends with the host
waiting, so the events bracket all of it), in one process.  The pictures of the placed call must equal the other
route's for every output frame, or the tool fails.  The ratios are a report, not a pass criterion.

With --parent-root (a checkout of the parent commit with its library built, for instance under hap_amd/variants/, where
tools/build_variants.sh's builds go: the package is the parent's too, since this one binds calls the parent's library
does not have), workload (A)'s composite_frames is timed in child processes, this build's and the parent's,
alternating, and the tool fails unless each median lies within the other's smallest-to-largest range: the existing call
is what it was.  --only parent does nothing else.

Prints one JSON line per file written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child process of --parent-root imports the package of that checkout)
sys.path.insert(0, os.environ.get("HAP_AMD_TIMING_PACKAGE_ROOT") or ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import hap_amd  # noqa: E402
from composite_timing import rdiv255, source_pictures, timed_ms  # noqa: E402

FMT_DXT1, FMT_DXT5, FMT_YCOCG, FMT_RGTC1 = 0x83F0, 0x83F3, 0x01, 0x8DBB
BLOCK_BYTES = {FMT_DXT1: 8, FMT_DXT5: 16, FMT_YCOCG: 16, FMT_RGTC1: 8}
HAP, HAP_Q, HAP_Q_ALPHA = (FMT_DXT1,), (FMT_YCOCG,), (FMT_YCOCG, FMT_RGTC1)
CHUNKS = 16
CANVAS = (7680, 4320)
TILE = (1920, 1080)
INSET_AT = (5600, 3100)
INSET_OPACITY = 200


def make_frames(ctx, w, h, count, fmts, layer):
    """(frames, their sizes) of one layer: one frame per output frame, four distinct pictures in turn"""
    sizes = [(w // 4) * (h // 4) * BLOCK_BYTES[f] for f in fmts]
    cap = hap_amd.HapMaxEncodedLength(sizes, list(fmts), [CHUNKS] * len(fmts))
    distinct = source_pictures(w, h, layer)
    made = []
    for i in range(min(4, count)):
        buf = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r, u, res = ctx.encode_frames_rgba([distinct[i]], w, h, w * 4, list(fmts), [1] * len(fmts), [CHUNKS] * len(fmts), [buf])
        assert r == 0 and res == [0], (r, res)
        made.append(buf[: u[0]].clone())
    del distinct
    torch.cuda.empty_cache()
    # (a frame of its own per output frame, as a player has them)
    frames = [made[i % len(made)].clone() if i >= len(made) else made[i] for i in range(count)]
    return frames, [int(f.numel()) for f in frames]


def ratio(a, b):
    return round(a[0] / b[0], 3)


def spreads_overlap(a, b):
    """each median within the other's smallest-to-largest range"""
    return b[1] <= a[0] <= b[2] and a[1] <= b[0] <= a[2]


def full_size(ctx, w, h, count, reps):
    layers = (HAP_Q, HAP_Q_ALPHA)
    made = [make_frames(ctx, w, h, count, fmts, l) for l, fmts in enumerate(layers)]
    frames = [[made[l][0][f] for l in range(2)] for f in range(count)]
    sizes = [[made[l][1][f] for l in range(2)] for f in range(count)]
    opacities = [[255, (37 + 211 * f // max(1, count - 1)) % 256] for f in range(count)]
    out = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    check = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def existing():
        r, res = ctx.composite_frames(frames, sizes, [1, 2], list(check), w, h, opacities=opacities)
        assert r == 0 and not any(res), (r, res)

    def placed():
        r, res = ctx.composite_frames_placed(frames, sizes, [1, 2], [(w, h)] * 2, list(out), w, h, opacities=opacities)
        assert r == 0 and not any(res), (r, res)

    res = {"geometry": [w, h], "output_frames": count, "layer_formats": [list(f) for f in layers]}
    # (interleaved: placed, existing, placed, existing -- two medians each, so that drift shows)
    res["placed_ms"] = timed_ms(placed, reps)
    res["composite_frames_ms"] = timed_ms(existing, reps)
    res["placed_again_ms"] = timed_ms(placed, reps)
    res["composite_frames_again_ms"] = timed_ms(existing, reps)
    assert torch.equal(out, check), "full_size: the placed call's pictures differ from composite_frames'"
    res["pictures_equal"] = True
    res["placed_over_composite_frames"] = ratio(res["placed_ms"], res["composite_frames_ms"])
    res["spreads_overlap"] = spreads_overlap(res["placed_ms"], res["composite_frames_ms"])
    for name, call in (("placed", placed), ("composite_frames", existing)):
        times = []
        ctx.set_profiling(True)
        for _ in range(reps):
            ctx.collect_profile()
            call()
            times.append(ctx.collect_profile()["block_decode"][1])
        ctx.set_profiling(False)
        res["block_decode_ms_of_" + name] = [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]
    return res


def blend_inset_int32(canvas_part, inset, opacity):
    s = inset.to(torch.int32)
    a = rdiv255(s[..., 3:4] * opacity)
    s[..., 3] = 255
    canvas_part.copy_(rdiv255(s * a + canvas_part.to(torch.int32) * (255 - a)))


def blend_inset_float32(canvas_part, inset, opacity):
    # (floor((2 x + 255) / 510) is rdiv255(x): composite_timing.py)
    def nearest(x):
        return torch.floor((2.0 * x + 255.0) / 510.0)
    s = inset.to(torch.float32)
    a = nearest(s[..., 3:4] * float(opacity))
    s[..., 3] = 255.0
    canvas_part.copy_(nearest(s * a + canvas_part.to(torch.float32) * (255.0 - a)))


def blend_inset_int32_in_place(canvas_part, inset, opacity):
    # (the same in fewer passes: the canvas's int32 copy is scaled and accumulated into in place)
    s = inset.to(torch.int32)
    a = rdiv255(s[..., 3:4] * opacity)
    s[..., 3] = 255
    d = canvas_part.to(torch.int32)
    d.mul_(255 - a).addcmul_(s, a)
    canvas_part.copy_(rdiv255(d))


INSET_EXPRESSIONS = {"int32": blend_inset_int32, "float32": blend_inset_float32, "int32_in_place": blend_inset_int32_in_place}


def inset(ctx, w, h, tw, th, at, count, reps):
    x, y = at
    background, frames_in = make_frames(ctx, w, h, count, HAP_Q, 0), make_frames(ctx, tw, th, count, HAP_Q_ALPHA, 1)
    frames = [[background[0][f], frames_in[0][f]] for f in range(count)]
    sizes = [[background[1][f], frames_in[1][f]] for f in range(count)]
    placements = [[(0, 0, w, h, 0, 0), (0, 0, tw, th, x, y)]] * count
    opacities = [[255, INSET_OPACITY]] * count
    out = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    check = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    small = torch.zeros((count, th, tw, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def placed():
        r, res = ctx.composite_frames_placed(frames, sizes, [1, 2], [(w, h), (tw, th)], list(out), w, h, placements=placements,
                                             opacities=opacities)
        assert r == 0 and not any(res), (r, res)

    def decodes():
        r, res = ctx.decode_frames_rgba(background[0], background[1], 1, list(check), w, h)
        assert r == 0 and not any(res), (r, res)
        r, res = ctx.decode_frames_rgba(frames_in[0], frames_in[1], 2, list(small), tw, th)
        assert r == 0 and not any(res), (r, res)

    def decodes_then(expression):
        def call():
            decodes()
            INSET_EXPRESSIONS[expression](check[:, y: y + th, x: x + tw], small, INSET_OPACITY)
            torch.cuda.synchronize()
        return call

    res = {"geometry": [w, h], "inset": [tw, th], "inset_at": [x, y], "opacity": INSET_OPACITY, "output_frames": count}
    res["placed_ms"] = timed_ms(placed, reps)
    res["decodes_ms"] = timed_ms(decodes, reps)
    res["decodes_then_torch_ms"] = {}
    for expression in INSET_EXPRESSIONS:
        res["decodes_then_torch_ms"][expression] = timed_ms(decodes_then(expression), reps)
        assert torch.equal(out, check), "inset: the placed call's pictures differ from torch's (%s)" % expression
        check.zero_()
        torch.cuda.empty_cache()
    res["pictures_equal_the_torch_blend"] = True
    fastest = min(res["decodes_then_torch_ms"], key=lambda k: res["decodes_then_torch_ms"][k][0])
    res["fastest_torch_expression"] = fastest
    res["placed_over_decodes_then_torch"] = ratio(res["placed_ms"], res["decodes_then_torch_ms"][fastest])
    res["placed_over_decodes"] = ratio(res["placed_ms"], res["decodes_ms"])
    return res


def mosaic(ctx, w, h, tw, th, count, reps):
    nx, ny = w // tw, h // th
    tiles = nx * ny
    made = [make_frames(ctx, tw, th, count, HAP, l) for l in range(tiles)]
    frames = [[made[l][0][f] for l in range(tiles)] for f in range(count)]
    sizes = [[made[l][1][f] for l in range(tiles)] for f in range(count)]
    placements = [[(0, 0, tw, th, tw * (l % nx), th * (l // nx)) for l in range(tiles)]] * count
    out = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    check = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def placed():
        r, res = ctx.composite_frames_placed(frames, sizes, [1] * tiles, [(tw, th)] * tiles, list(out), w, h, placements=placements)
        assert r == 0 and not any(res), (r, res)

    def decodes():
        for l in range(tiles):
            tx, ty = tw * (l % nx), th * (l // nx)
            r, res = ctx.decode_frames_rgba(made[l][0], made[l][1], 1, [check[f, ty:, tx:] for f in range(count)], tw, th,
                                            row_bytes=w * 4)
            assert r == 0 and not any(res), (r, res)

    res = {"geometry": [w, h], "tile": [tw, th], "tiles": tiles, "output_frames": count, "layer_formats": [list(HAP)]}
    res["placed_ms"] = timed_ms(placed, reps)
    res["decodes_into_tiles_ms"] = timed_ms(decodes, reps)
    # (what of the canvas no tile covers -- nothing, with these sizes -- is the background in one and zero in the other)
    assert nx * tw == w and ny * th == h
    assert torch.equal(out, check), "mosaic: the placed call's pictures differ from the decoders'"
    res["pictures_equal"] = True
    res["placed_over_decodes_into_tiles"] = ratio(res["placed_ms"], res["decodes_into_tiles_ms"])
    return res


def existing_call_alone(w, h, count, reps):
    """(child process: the library is whatever HAP_AMD_LIBRARY says) composite_frames on workload (A): one JSON line"""
    ctx = hap_amd.Context(0)
    layers = (HAP_Q, HAP_Q_ALPHA)
    made = [make_frames(ctx, w, h, count, fmts, l) for l, fmts in enumerate(layers)]
    frames = [[made[l][0][f] for l in range(2)] for f in range(count)]
    sizes = [[made[l][1][f] for l in range(2)] for f in range(count)]
    opacities = [[255, (37 + 211 * f // max(1, count - 1)) % 256] for f in range(count)]
    out = torch.zeros((count, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def existing():
        r, res = ctx.composite_frames(frames, sizes, [1, 2], list(out), w, h, opacities=opacities)
        assert r == 0 and not any(res), (r, res)

    times = timed_ms(existing, reps)
    digest = int(out.view(-1)[:: 4099].to(torch.int64).sum().item())
    ctx.close()
    print(json.dumps({"composite_frames_ms": times, "package": os.path.dirname(os.path.abspath(hap_amd.__file__)), "digest": digest}))


def against_parent(args, w, h):
    """workload (A)'s composite_frames in fresh child processes: this build, the parent's, this build, the parent's"""
    runs = {"this_build": [], "parent_build": []}
    for turn in range(4):
        which = "parent_build" if turn % 2 else "this_build"
        env = dict(os.environ)
        env.pop("HAP_AMD_LIBRARY", None)
        env.pop("HAP_AMD_TIMING_PACKAGE_ROOT", None)
        if which == "parent_build":
            env["HAP_AMD_TIMING_PACKAGE_ROOT"] = os.path.abspath(args.parent_root)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-call-alone", "--reps", str(args.reps),
                               "--shrink", str(args.shrink), "--frames", str(args.frames)], env=env, capture_output=True,
                              text=True, timeout=900)
        assert done.returncode == 0, done.stderr[-2000:]
        runs[which].append(json.loads(done.stdout.strip().splitlines()[-1]))
    res = {"workload": "full_size: composite_frames, Hap Q Alpha over Hap Q", "geometry": [w, h], "output_frames": args.frames,
           "reps": args.reps, "times": "[median, min, max] ms", "order": "this, parent, this, parent: a fresh process each"}
    for which, made in runs.items():
        res[which] = [m["composite_frames_ms"] for m in made]
        # (the two runs of a build as one: the median of their medians, the smallest and the largest of all their calls)
        res[which + "_ms"] = [round(statistics.median(m["composite_frames_ms"][0] for m in made), 3),
                              min(m["composite_frames_ms"][1] for m in made), max(m["composite_frames_ms"][2] for m in made)]
    res["same_pictures"] = len({m["digest"] for made in runs.values() for m in made}) == 1
    res["this_over_parent"] = ratio(res["this_build_ms"], res["parent_build_ms"])
    res["medians_within_each_others_range"] = spreads_overlap(res["this_build_ms"], res["parent_build_ms"])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.parent_out)), exist_ok=True)
    with open(args.parent_out, "w") as f:
        f.write(line + "\n")
    assert res["same_pictures"], "composite_frames' pictures differ between this build and the parent's"
    assert res["medians_within_each_others_range"], "composite_frames is not what it was: %r against the parent's %r" % (
        res["this_build_ms"], res["parent_build_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_placed.json"), help="where the JSON goes")
    ap.add_argument("--shrink", type=int, default=1, help="rehearsal: divide every geometry's sides by this")
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built: times composite_frames in both")
    ap.add_argument("--parent-out", default=os.path.join(ROOT, "profiles", "composite_placed_parent.json"))
    ap.add_argument("--only", choices=("full_size", "inset", "mosaic", "parent"), action="append",
                    help="these workloads alone (parent: the comparison of --parent-root alone)")
    ap.add_argument("--existing-call-alone", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "composite_placed_timing.py needs a GPU"
    w, h = (v // args.shrink // 16 * 16 for v in CANVAS)
    tw, th = w // 4, h // 4 // 4 * 4
    if args.shrink == 1:
        assert (tw, th) == TILE
    if args.existing_call_alone:
        existing_call_alone(w, h, args.frames, args.reps)
        return
    at = (INSET_AT[0] // args.shrink // 4 * 4, INSET_AT[1] // args.shrink // 4 * 4)
    if args.only == ["parent"]:
        against_parent(args, w, h)
        return
    ctx = hap_amd.Context(0)
    res = {"reps": args.reps, "times": "[median, min, max] ms"}
    wanted = [name for name in args.only or ["full_size", "inset", "mosaic"] if name != "parent"]
    for name in wanted:
        if name == "full_size":
            res[name] = full_size(ctx, w, h, args.frames, args.reps)
        elif name == "inset":
            res[name] = inset(ctx, w, h, tw, th, at, args.frames, args.reps)
        else:
            res[name] = mosaic(ctx, w, 4 * th, tw, th, args.frames, args.reps)
        print("%s: done" % name, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if args.parent_root:
        against_parent(args, w, h)


if __name__ == "__main__":
    main()

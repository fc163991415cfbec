"""GPU measurement of the A8 <-> RGTC1 kernels (hap_amd/csrc/alpha_plane.hip) at 8K (7680 x 4320) and 16K (15360 x 8640).

    python tools/bench_alpha.py [--reps N] [--batch F] [--out FILE]

Per geometry, with the context's event timer (HIP events of the block_encode / block_decode profile classes):

  encode  HapGpuCompressAlpha on one A8 picture in HBM, and in the same run the yardstick: HapGpuCompressRGBA(...,
          A_RGTC1) on the RGBA8 picture that carries the plane (the same block maths on four times the input bytes);
          then F pictures -> Hap Alpha-Only frames in one HapGpuEncodeFramesAlpha call (kernel time of its block-encode
          launch, and the call)
  decode  HapGpuDecompressAlpha into a picture in HBM, and in the same run the DXT1 -> RGBA8 decoder at the same
          geometry; then F frames -> pictures in one HapGpuDecodeFramesAlpha call

and prints time, bytes moved and the fraction of HBM peak as one JSON line.  Bytes per block: 16 + 8 (A8), 64 + 8
(RGBA8 -> RGTC1, DXT1 -> RGBA8).  The kernels are alternated over two rounds: the spread between rounds is the noise.

The road is the library's choice (the wide one for these aligned pictures).  A measurement build of the library
(tools/build_variants.sh, loaded with HAP_AMD_LIBRARY) takes the one-block-per-lane road with HAP_AMD_NO_WIDE_PLANES=1:
run the tool once with each in the same sitting and compare "road".  The encoder's texture is compared with the RGBA
road's, and a block row of the decoder's picture with the oracle.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hap_amd  # noqa: E402
from hap_amd import synth  # noqa: E402

FMT_DXT1, FMT_RGTC1 = 0x83F0, 0x8DBB
HBM_PEAK_GBS = 8000.0
GEOMETRIES = {"8k": (7680, 4320), "16k": (15360, 8640)}


def rate(blocks, bytes_per_block, kernel_us):
    gbs = blocks * bytes_per_block / (kernel_us * 1e-6) / 1e9
    return {"kernel_us": round(kernel_us, 2), "bytes": blocks * bytes_per_block, "GBps": round(gbs, 0),
            "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)}


def timed(ctx, cls, call, reps, blocks, bytes_per_block):
    for _ in range(3):
        call()
    ctx.set_profiling(True)
    ctx.collect_profile()
    ctx.timer_start()
    for _ in range(reps):
        call()
    call_ms = ctx.timer_stop()
    n, ms = ctx.collect_profile()[cls]
    ctx.set_profiling(False)
    # (a call whose launches are replayed from a recorded graph opens no timing scope: then only the call is timed)
    out = rate(blocks, bytes_per_block, ms / n * 1e3) if n else {"kernel_us": None, "bytes": blocks * bytes_per_block}
    out["launches"] = n
    out["call_us"] = round(call_ms / reps * 1e3, 2)
    return out


def one_geometry(ctx, w, h, reps, batch):
    blocks = (w // 4) * (h // 4)
    res = {"geometry": [w, h], "blocks": blocks}
    rgba = synth.rgba_frame(w, h, 0, device="cuda")
    plane = rgba[..., 3].contiguous()
    tex_a = torch.zeros(blocks * 8, dtype=torch.uint8, device="cuda")
    tex_r = torch.zeros(blocks * 8, dtype=torch.uint8, device="cuda")
    dxt1 = torch.zeros(blocks * 8, dtype=torch.uint8, device="cuda")
    back = torch.zeros(w * h, dtype=torch.uint8, device="cuda")
    pic = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.compress_rgba(rgba, w, h, w * 4, FMT_DXT1, dxt1)[0] == 0

    def ok(r):
        assert r[0] == 0, r

    runs = (("encode_a8", "block_encode", lambda: ok(ctx.compress_alpha(plane, w, h, w, tex_a)), 24),
            ("encode_rgba8_rgtc1", "block_encode", lambda: ok(ctx.compress_rgba(rgba, w, h, w * 4, FMT_RGTC1, tex_r)), 72),
            ("decode_a8", "block_decode", lambda: ok(ctx.decompress_alpha(tex_a, w, h, out=back)), 24),
            ("decode_dxt1_rgba8", "block_decode", lambda: ok(ctx.decompress_rgba(dxt1, FMT_DXT1, w, h, rgba=pic)), 72))
    for _rnd in range(2):
        for name, cls, call, bpb in runs:
            res.setdefault(name, []).append(timed(ctx, cls, call, reps, blocks, bpb))
    ctx.synchronize()
    res["encode_equals_rgba_road"] = bool(torch.equal(tex_a, tex_r))
    import _data as D
    want = D.oracle_bc_decode(tex_a[: (w // 4) * 8].cpu().numpy().tobytes(), FMT_RGTC1, w, 4)
    res["decode_row_equals_oracle"] = bool(np.array_equal(back[: 4 * w].cpu().numpy().reshape(4, w), want))
    best = {k: min(r["kernel_us"] for r in res[k]) for k, _c, _f, _b in runs}
    res["encode_a8_over_rgba8"] = round(best["encode_a8"] / best["encode_rgba8_rgtc1"], 3)
    res["decode_of_peak_a8_and_dxt1"] = [max(r["of_hbm_peak"] for r in res["decode_a8"]),
                                         max(r["of_hbm_peak"] for r in res["decode_dxt1_rgba8"])]
    del rgba, pic, tex_r, dxt1

    # F pictures -> frames -> pictures, one call each way
    planes = [plane] + [synth.rgba_frame(w, h, i, device="cuda")[..., 3].contiguous() for i in range(1, min(batch, 4))]
    planes = [planes[i % len(planes)] for i in range(batch)]
    cap = hap_amd.HapMaxEncodedLength([blocks * 8], [FMT_RGTC1], [16])
    frames = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    backs = [torch.zeros(w * h, dtype=torch.uint8, device="cuda") for _ in range(batch)]
    torch.cuda.synchronize()
    used = [0] * batch

    def enc():
        r, u, rr = ctx.encode_frames_alpha(planes, w, h, w, 1, 16, frames, flags=hap_amd.ENCODE_FRAGMENT_INDEX)
        assert r == 0 and rr == [0] * batch, (r, rr)
        used[:] = u

    def dec():
        r, rr = ctx.decode_frames_alpha(frames, used, backs, w, h)
        assert r == 0 and rr == [0] * batch, (r, rr)

    for name, cls, call in (("encode_frames", "block_encode", enc), ("decode_frames", "block_decode", dec)):
        out = timed(ctx, cls, call, 5, blocks * batch, 24)
        out["pictures"] = batch
        out["kernel_us_per_picture"] = round(out["kernel_us"] / batch, 2) if out["kernel_us"] else None
        res[name] = out
    res["frames_ratio"] = round(sum(used) / (batch * blocks * 8), 3)
    ctx.synchronize()
    res["frames_round_trip_equals_single"] = bool(torch.equal(backs[0], back))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_alpha.py needs a GPU"
    narrow = bool(os.environ.get("HAP_AMD_LIBRARY")) and "HAP_AMD_NO_WIDE_PLANES" in os.environ
    ctx = hap_amd.Context(0)
    res = {"road": "narrow (measurement build, one block per lane)" if narrow else "wide (four blocks per lane)",
           "hbm_peak_GBps": HBM_PEAK_GBS, "reps": args.reps}
    for name, (w, h) in GEOMETRIES.items():
        res[name] = one_geometry(ctx, w, h, args.reps, args.batch)
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

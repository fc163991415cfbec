#!/usr/bin/env python3
"""Dev tool (CPU only): the table of an alternating A/B series of bench.py lines, by the project's rule.

    python tools/ab_summary.py profiles/r11_ab_bench_full_parent.jsonl profiles/r11_ab_bench_full_branch.jsonl [key ...]

Each file holds one JSON result line per run.  For every key (dotted path into the line; a default list when none is
given, keys a line does not have are left out) it prints both arms' runs, median and range, the difference of the
medians in units of the PARENT's spread (max - min of its runs) and whether the branch's worst run beats the parent's
best.  A figure counts as changed at three spreads with the worst beating the best; higher is better for `value`, lower
for everything else."""
import json
import statistics
import sys

DEFAULT_KEYS = ["kernels.encode_fused.ms_avg", "value", "ms_per_step", "encode_only.ms", "decode_only.ms", "c5.encode_only.ms",
                "c5.kernels.block_encode.ms_avg", "c5.value", "c3.value", "c3.encode_only.ms", "c2.encode_only.ms",
                "bc7_opaque.encode_ms", "bc7_opaque.decode_ms", "separate_passes.kernels_ms.block_encode"]
HIGHER_IS_BETTER = ("value",)


def dig(line, key):
    for part in key.split("."):
        if not isinstance(line, dict) or part not in line:
            return None
        line = line[part]
    return line if isinstance(line, (int, float)) else None


def main():
    parent = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
    branch = [json.loads(l) for l in open(sys.argv[2]) if l.strip()]
    keys = sys.argv[3:] or DEFAULT_KEYS
    print("parent %d runs, branch %d runs" % (len(parent), len(branch)))
    for key in keys:
        a, b = [dig(l, key) for l in parent], [dig(l, key) for l in branch]
        if None in a or None in b or not a or not b:
            continue
        ma, mb = statistics.median(a), statistics.median(b)
        spread = max(a) - min(a)
        up = key.split(".")[-1] in HIGHER_IS_BETTER
        gain = (mb - ma) if up else (ma - mb)
        beats = (min(b) > max(a)) if up else (max(b) < min(a))
        fmt = lambda v: " ".join("%.4g" % x for x in v)
        print("%-42s parent %s median %.4g (%.4g-%.4g) | branch %s median %.4g (%.4g-%.4g) | diff %+.4g (%+.2f%%) = %.1f spreads "
              "(spread %.4g); branch worst beats parent best: %s" % (key, fmt(a), ma, min(a), max(a), fmt(b), mb, min(b), max(b),
                                                                   mb - ma, 100.0 * (mb - ma) / ma, gain / spread if spread else float("inf"),
                                                                   spread, beats))
    for name, get in (("bit_exact", lambda l: l.get("bit_exact")), ("snappy_ratio", lambda l: (l.get("config") or {}).get("snappy_ratio"))):
        print("%s: %s %s" % (name, [get(l) for l in parent], [get(l) for l in branch]))


if __name__ == "__main__":
    main()

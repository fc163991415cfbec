#!/usr/bin/env python3
"""Dev tool (CPU only): static instruction counts of a HIP kernel by source line.

    python tools/isa_by_line.py hap_amd/csrc/snappy_decode_fields.hip [--func decode_fields_unit<4] [-D...]
        [--ranges 234:256=measure,288:355=walk,...]

Compiles the file for gfx950 with -gline-tables-only, attributes every instruction of the kernel to the `.loc`
in front of it and prints VALU / SALU / LDS / VMEM counts per source line (or per named line range).  The counts
are static (loops once, every inlined layout separately when --func is not given); trip counts are the
reader's business.  hipcc cross-compiles: no GPU needed.

    python tools/isa_by_line.py --fused-budget [--weights tools/isa_weights_w5.json] [--csrc OTHER/hap_amd/csrc]
    python tools/isa_by_line.py --resources snappy_compress_blocks.hip [--csrc ...]

The cycle budget of the fused encode kernel (snappy_compress_blocks_kernel<4, YCoCg>, -DSCB_ONLY_FUSED_YCOCG): the same
attribution, per PHASE (found by anchor text in the sources, so the table follows the code when lines move), each VALU
instruction weighted by its measured issue cost (tools/micro/valu_rates2.hip at the kernel's five waves per SIMD;
weights file: opcode -> cycles, "default" for what was not measured; a matrix instruction has a column of its own and
counts in `cycles` with what it costs beside VALU, tools/micro/mfma_beside_valu.hip), times the phase's trip count for an 8K Hap Q
fragment.  Code inlined from the helpers at the top of the file or from a system header (`min`, `max`, popcount, the
DPP moves) counts under the line of the kernel's body that called it, found from the assembler's inlined-at comments, so
a phase's row is everything it issues.  Also prints the kernel's register and scratch figures from the code object's
metadata.
"""
import collections
import re
import subprocess
import sys
import tempfile


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


# Phases of the fused encode kernel: (name, file, anchor text, n-th occurrence, trips per 8K Hap Q fragment).  A phase
# runs from its anchor's line to the next anchor of the same file.  An anchor with None for its occurrence is one that
# older trees (--csrc) do not have: first occurrence where present, skipped where not.  Trips: 8 steps of 64 blocks; the choose loop 1.2
# passes, the element list 9.2 turns and the tag walk 7.4 passes (LABNOTES, 8K stream: 470 elements per fragment).
CORE, SCB = "bc_encode_core.hpp", "snappy_compress_blocks.hip"
FUSED_PHASES = [
    ("helpers: mad24 / quant", CORE, "namespace hapbc {", 0, 8.0),
    ("luma ramp", CORE, "__device__ __forceinline__ uint2 alpha_block", 0, 8.0),
    ("end points", CORE, "struct projection {", 0, 8.0),
    ("colour index", CORE, "// The clamp the definition states, t to 0 .. top", None, 8.0),
    ("colour index (RGB)", CORE, "template <bool FLIPPED = false>", 0, 8.0),
    ("end points", CORE, "__device__ __forceinline__ unsigned pack3", 0, 8.0),
    ("colour box+covariance (RGB)", CORE, "__device__ __forceinline__ uint2 colour_block", 0, 8.0),
    ("colour box+covariance", CORE, "__device__ __forceinline__ uint2 ycocg_colour_block", 0, 8.0),
    ("end points", CORE, "const int mo = lo_o + hi_o", None, 8.0),              # (the scalar form, before R11)
    ("colour index", CORE, "const int K = mad24(d_o", None, 8.0),
    ("end points", CORE, "const pk_i16 mid = lo + hi;", None, 8.0),             # (the pair form)
    ("end points", CORE, "const pk_i16 mid = lo_b + hi_b;", None, 8.0),         # (the pair form on biased pairs, R13)
    ("colour index", CORE, "const int K = dot_back + sixth", None, 8.0),
    ("YCoCg transform", CORE, "// ---- the YCoCg transform as one 4x4x4 signed-byte matrix product", None, 8.0),
    ("YCoCg transform", CORE, "2 (Co - 128) | 4 (Cg - 128) << 16 of four pixels", None, 8.0),
    ("YCoCg transform", CORE, "template <int FMT", 0, 8.0),
    ("loop+address overhead", SCB, "#include <hip/hip_runtime.h>", 0, 1.0),
    ("choose", SCB, "__device__ __forceinline__ int scan_add", 0, 1.0),
    ("nibble transpose", SCB, "// value of lane ^ 4 / ^ 2 / ^ 1", 0, 8.0),
    ("match compare", SCB, "// 1 where the field differs", 0, 8.0),
    ("table probe", SCB, "// value of an index field", 0, 8.0),
    ("loop+address overhead", SCB, "// FUSED >= 0: the texture does not exist yet", 0, 1.0),
    ("loop+address overhead (step)", SCB, "// ---- 1. match ----", 0, 8.0),
    ("match compare", SCB, "unsigned differ = 0;", 0, 8.0),
    ("table probe", SCB, "// table candidates of the index fields", 0, 8.0),
    ("nibble transpose", SCB, "// nibbles of 8 lanes", 0, 8.0),
    ("choose", SCB, "// (the table has served", 0, 1.0),
    ("choose (loop)", SCB, "while (__builtin_amdgcn_ballot_w64(front != 0u)", 0, 1.2),
    ("choose", SCB, "const unsigned cov = A[0] | A[1]", 0, 1.0),
    ("choose (element list)", SCB, "while (__builtin_amdgcn_ballot_w64(left != 0u)", 0, 9.2),
    ("look-back", SCB, "// ---- placed streams", 0, 1.0),
    ("literal walk", SCB, "// ---- 3a. emit the literal bytes", 0, 1.0),
    ("literal walk (step)", SCB, "const unsigned hh = 8u * s + (lane >> 3);", 0, 8.0),
    ("tag walk (set-up)", SCB, "// ---- 3b. emit the elements' tags", 0, 1.0),
    ("tag walk", SCB, "for (unsigned e0 = 0; e0 < elements; e0 += 64u)", 0, 7.4),
    ("group table", SCB, "if (want_sizes) {", 0, 1.0),
]


def phase_spans(csrc):
    """{file: [(first line, last line, name, trips)]} from the anchors."""
    spans = {}
    for fname in (CORE, SCB):
        lines = open(csrc + "/" + fname).read().splitlines()
        marks = []
        for name, f, anchor, nth, trips in FUSED_PHASES:
            if f != fname:
                continue
            hits = [i + 1 for i, l in enumerate(lines) if anchor in l]
            if nth is None:
                if not hits:
                    continue
                nth = 0
            if len(hits) <= nth:
                raise SystemExit("isa_by_line: anchor %r not found in %s" % (anchor, fname))
            marks.append((hits[nth], name, trips))
        marks.sort()
        spans[fname] = [(lo, (marks[i + 1][0] - 1) if i + 1 < len(marks) else len(lines), name, trips)
                        for i, (lo, name, trips) in enumerate(marks)]
    return spans


def attribute(fname, line, loc, body_first, prev):
    """The (file, line) an instruction counts under.  The assembler's comment lists where the code was inlined from,
    innermost first.  Lines of bc_encode_core.hpp count where they stand (its helpers are a phase of their own), and so
    does what they inlined from a system header (`min` / `max` / `abs`): under the innermost line of that file.  The
    small helpers at the top of snappy_compress_blocks.hip, and system headers called from it, count under the line
    of the kernel's body that called them -- the outermost one.  Line 0 (compiler-made code) stays with the phase
    of the instruction in front of it."""
    chain = [(f.split("/")[-1], int(l)) for f, l in re.findall(r"([\w./+-]+):(\d+):\d+", loc.split(";", 1)[1])] if ";" in loc else []
    chain = chain or [(fname, line)]
    for f, l in chain:
        if f == CORE:
            return (f, l)
    for f, l in reversed(chain):
        if f == SCB and l >= body_first:
            return (f, l)
    if chain[0] == (SCB, 0) and prev is not None:
        return prev
    return chain[0]


def base_op(op):
    for suf in ("_e32", "_e64", "_sdwa", "_dpp"):
        if op.endswith(suf):
            return op[: -len(suf)] + ("_dpp" if suf == "_dpp" else "")
    return op


def fused_budget(args):
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "hap_amd", "csrc")
    wfile = os.path.join(here, "isa_weights_w5.json")
    for i, a in enumerate(args):
        if a == "--csrc":                   # another checkout's hap_amd/csrc (the parent's table with the same tool)
            csrc = args[i + 1]
    defs = [a for a in args if a.startswith("-D")]
    if not any(a.startswith("-DSCB_ONLY_FUSED") for a in defs):
        defs.append("-DSCB_ONLY_FUSED_YCOCG")
    for i, a in enumerate(args):
        if a == "--weights":
            wfile = args[i + 1]
    weights = json.load(open(wfile))
    default_w = weights["default"]
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-gline-tables-only",
               "-DHAP_MEASUREMENT_BUILD", "-I" + csrc, "-S", "--cuda-device-only", "-o", tmp.name, os.path.join(csrc, SCB)] + defs
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        text = open(tmp.name).read().splitlines()
    spans = phase_spans(csrc)
    body_first = min(lo for lo, hi, nm, tr in spans[SCB] if nm == "loop+address overhead" and lo > 100)
    files, cur = {}, None
    acc = collections.OrderedDict()
    unweighted = collections.Counter()
    meta = []
    for line in text:
        s = line.strip()
        m = re.match(r"\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", s)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)\s+(\d+)", s)
        if m:
            cur = attribute(files.get(int(m.group(1)), "?"), int(m.group(2)), s, body_first, cur)
            continue
        if re.match(r"\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):", s):
            meta.append(s)
        if not s or s.startswith((".", ";", "//")) or s.endswith(":") or cur is None:
            continue
        op = s.split()[0]
        kind = classify(op)
        name, trips = "other: " + cur[0], 1.0
        for lo, hi, nm, tr in spans.get(cur[0], ()):
            if lo <= cur[1] <= hi:
                name, trips = nm, tr
                break
        row = acc.setdefault(name, {"trips": trips, "valu": 0, "mfma": 0, "cycles": 0.0, "salu": 0, "lds": 0, "vmem": 0, "nop": 0})
        if op.startswith("v_mfma"):         # the matrix pipe: priced in cycles (what it costs beside VALU), not a VALU
            row["mfma"] += 1
            row["cycles"] += weights.get(base_op(op), default_w)
        elif kind == "valu":
            w = weights.get(op, weights.get(base_op(op)))      # (an SDWA form weighed on its own goes by its own name)
            if w is None:
                w = default_w
                unweighted[base_op(op)] += 1
            row["valu"] += 1
            row["cycles"] += w
        elif kind == "wait":
            row["nop"] += 1 if op == "s_nop" else 0
        elif kind in row:
            row[kind] += 1
    print("weights: %s (%d opcodes measured, default %.2f)" % (os.path.basename(wfile), len(weights) - 1, default_w))
    print("%-30s %6s %7s %6s %9s | %9s %9s %11s | %5s %5s %5s %5s" % ("phase", "trips", "valu", "mfma", "cycles", "valu/frag",
                                                                      "mfma/frag", "cycles/frag", "salu", "lds", "vmem", "s_nop"))
    print("(valu, cycles: per trip -- phases with 8 trips are the eight unrolled steps, listed as one step's share)")
    tv = tm = tc = 0.0
    for name, r in sorted(acc.items(), key=lambda kv: -frag(kv[1], "cycles")):
        per = 8.0 if r["trips"] == 8.0 else 1.0
        print("%-30s %6.1f %7.1f %6.1f %9.1f | %9.0f %9.0f %11.0f | %5d %5d %5d %5d" % (
            name, r["trips"], r["valu"] / per, r["mfma"] / per, r["cycles"] / per, frag(r, "valu"), frag(r, "mfma"),
            frag(r, "cycles"), r["salu"], r["lds"], r["vmem"], r["nop"]))
        tv += frag(r, "valu"); tm += frag(r, "mfma"); tc += frag(r, "cycles")
    print("%-30s %6s %7s %6s %9s | %9.0f %9.0f %11.0f |" % ("per fragment", "", "", "", "", tv, tm, tc))
    for m in meta:
        print("  " + m)
    if unweighted:
        print("opcodes at the default weight: " + ", ".join("%s x%d" % kv for kv in unweighted.most_common()))


def frag(r, key):
    """A phase's share of one fragment: the eight steps are unrolled (their static count IS the fragment's), loops run
    `trips` times."""
    return r[key] * (1.0 if r["trips"] == 8.0 else r["trips"])


def resources(args):
    """--resources FILE.hip [-D...]: registers, scratch and static VALU count of every kernel of a translation unit."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "hap_amd", "csrc")
    for i, a in enumerate(args):
        if a == "--csrc":
            csrc = args[i + 1]
    src = args[args.index("--resources") + 1]
    defs = [a for a in args if a.startswith("-D")]
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + csrc, "-S",
               "--cuda-device-only", "-o", tmp.name, os.path.join(csrc, src)] + defs
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        text = open(tmp.name).read()
    valu = {}
    for m in re.finditer(r"^(_Z\w+):.*?s_endpgm", text, re.S | re.M):
        valu[m.group(1)] = len(re.findall(r"^\s+v_", m.group(0), re.M))
    try:
        demangle = subprocess.run(["c++filt"], input="\n".join(valu), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        demangle = list(valu)
    names = dict(zip(valu, demangle))
    print("%-6s %-6s %-8s %-6s %s" % ("vgpr", "sgpr", "scratch", "valu", "kernel (" + src + ")"))
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        body = m.group(2)
        get = lambda k: re.search(r"\." + k + r":\s+(\d+)", body).group(1)
        nm = names.get(m.group(1), m.group(1)).replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print("%-6s %-6s %-8s %-6d %s" % (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"),
                                        valu.get(m.group(1), 0), nm))


def main():
    args = sys.argv[1:]
    if "--fused-budget" in args:
        return fused_budget(args)
    if "--resources" in args:
        return resources(args)
    src = args[0]
    defs = [a for a in args[1:] if a.startswith("-D")]
    ranges = []
    func = None
    for i, a in enumerate(args):
        if a == "--ranges":
            for item in args[i + 1].split(","):
                span, name = item.split("=")
                lo, hi = span.split(":")
                ranges.append((int(lo), int(hi), name))
        if a == "--func":
            func = args[i + 1]
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-gline-tables-only",
               "-DHAP_MEASUREMENT_BUILD", "-Ihap_amd/csrc", "-S", "--cuda-device-only", "-o", tmp.name, src] + defs
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        text = open(tmp.name).read().splitlines()
    files = {}
    per = collections.defaultdict(collections.Counter)
    cur = None
    inlined_at = None
    for line in text:
        s = line.strip()
        m = re.match(r"\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", s)
        if m:
            files[int(m.group(1))] = m.group(3) or m.group(2)
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (int(m.group(1)), int(m.group(2)))
            continue
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        if cur is None:
            continue
        per[cur][classify(op)] += 1
    main_file = None
    for k, v in files.items():
        if v.endswith(src.split("/")[-1]):
            main_file = k
    tot = collections.Counter()
    rows = []
    if ranges:
        acc = collections.defaultdict(collections.Counter)
        for (fid, ln), c in per.items():
            name = "other:" + files.get(fid, "?").split("/")[-1]
            if fid == main_file:
                name = "unranged"
                for lo, hi, nm in ranges:
                    if lo <= ln <= hi:
                        name = nm
                        break
            acc[name] += c
        rows = sorted(acc.items(), key=lambda kv: -kv[1]["valu"])
    else:
        rows = sorted((("%s:%d" % (files.get(fid, "?").split("/")[-1], ln), c) for (fid, ln), c in per.items()),
                      key=lambda kv: -kv[1]["valu"])[:60]
    print("%-28s %6s %6s %6s %6s %6s" % ("where", "valu", "salu", "lds", "vmem", "wait"))
    for name, c in rows:
        tot += c
        print("%-28s %6d %6d %6d %6d %6d" % (name, c["valu"], c["salu"], c["lds"], c["vmem"], c["wait"]))
    print("%-28s %6d %6d %6d %6d %6d" % ("total (listed)", tot["valu"], tot["salu"], tot["lds"], tot["vmem"], tot["wait"]))


if __name__ == "__main__":
    main()

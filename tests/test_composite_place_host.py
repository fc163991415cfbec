"""hap_place.h -- what a placement must be, what of it a canvas shows, and the scratch layout of layers of sizes of their
own -- walked by tests/c/place_layout.c under AddressSanitizer + UBSan: a plain executable with its own main, nothing
preloaded.  The clip is compared, block by block, with the definition over every block-aligned placement of the walk's
layers and canvases; every refusal is asked for at its edge; the layout keeps hap_slice.h's limits."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_placement_arithmetic_is_clean_and_is_the_definition(tmp_path):
    exe = str(tmp_path / "place_layout")
    cmd = ["gcc", "-std=c99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "hap_amd", "csrc"), os.path.join(ROOT, "tests", "c", "place_layout.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), (done.returncode, done.stdout, done.stderr[-3000:])
    walked = re.match(r"(\d+) placements and (\d+) canvas blocks walked, (\d+) layouts: ok", done.stdout.strip())
    # (every pair of axes of the walk: millions of placements, none skipped)
    assert walked and int(walked.group(1)) > 1000000 and int(walked.group(2)) > int(walked.group(1)) and int(walked.group(3)) > 100


def test_the_header_is_plain_c_without_a_runtime():
    text = open(os.path.join(ROOT, "hap_amd", "csrc", "hap_place.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes == ["hap_slice.h"], includes
    for word in ("hap_place_valid", "hap_place_layer_valid", "hap_place_clip_of", "hap_place_layout_of", "long long"):
        assert word in text, word

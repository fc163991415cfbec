#!/usr/bin/env python3
"""Regenerates tests/golden/bptc_pillow.json: SHA-256 digests of Pillow's BC7 decode of the block sets of
tests/_bptc.py (one per mode, the reserved blocks, and the shuffled mix of all of them), and of the block bytes
themselves.  Needs Pillow (12 decodes BC7 through its "bcn" decoder); the JSON it writes is committed, so that the
reference decoder stays pinned to third-party code on machines without Pillow (tests/test_bptc_reference.py).

Pillow decodes reserved blocks to (0, 0, 0, 255); its pictures are recorded as they are, and the test sets those
texels of the reference's pictures to the same value before it compares digests.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _bptc as B  # noqa: E402

OUT = os.path.join(HERE, "bptc_pillow.json")


def main():
    import PIL
    sets = B.block_sets()
    doc = {"generator": "tests/_bptc.py block_sets()", "pillow": PIL.__version__, "sets": {}}
    for name in sorted(sets):
        data = sets[name]
        w, h = B.geometry(len(data) // 16)
        pic = B.pillow_bc7_decode(data, w, h)
        doc["sets"][name] = {
            "width": w, "height": h,
            "blocks_sha256": hashlib.sha256(data).hexdigest(),
            "pillow_sha256": hashlib.sha256(pic.tobytes()).hexdigest(),
        }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()

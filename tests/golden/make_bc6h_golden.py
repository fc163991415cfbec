#!/usr/bin/env python3
"""Regenerates tests/golden/bc6h_pillow.json: SHA-256 digests of the block sets of tests/_bc6h.py (one per mode and
signedness, the reserved blocks, and the shuffled mix of each signedness), and of Pillow's BC6H decode of each set
under the signedness it was made for.  Needs Pillow (12 decodes BC6H through its "bcn" decoder, to 8-bit RGB); the
JSON it writes is committed, so that the reference decoder stays pinned to third-party code on machines without Pillow
(tests/test_bc6h_reference.py).

Pillow departs from the specification in two known ways (_bc6h.pillow_mask): the texels concerned are set to 0 in its
pictures before hashing, and the test does the same to the reference's projection.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _bc6h as B  # noqa: E402

OUT = os.path.join(HERE, "bc6h_pillow.json")


def main():
    import PIL
    sets = B.block_sets()
    doc = {"generator": "tests/_bc6h.py block_sets()", "pillow": PIL.__version__, "sets": {}}
    for name in sorted(sets):
        data = sets[name]
        signed = B.set_is_signed(name)
        w, h = B.geometry(len(data) // 16)
        pic = B.pillow_bc6h_decode(data, w, h, signed).copy()
        pic[B.pillow_mask(data, w, h, signed)] = 0
        doc["sets"][name] = {
            "width": w, "height": h, "signed": signed,
            "blocks_sha256": hashlib.sha256(data).hexdigest(),
            "pillow_sha256": hashlib.sha256(pic.tobytes()).hexdigest(),
        }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()

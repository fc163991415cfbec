#!/usr/bin/env python3
"""Regenerates tests/golden/reference_answers.json: runs tests/test_oracle_pinning.py with every question to the
reference answered by the live library (oracle/_ref/libhap_ref.so + libsnappy 1.1.8, built by `make -C oracle ref`
where the reference sources are at hand) and records the digests of its answers.  The JSON it writes is committed;
the tests read it wherever the live library is not built, and check it against the library wherever it is.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import _libs as L  # noqa: E402


def main():
    assert L.ref_api() is not None, "reference not built (make -C oracle ref)"
    L.RecordedReference.recording = True
    rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(TESTS, "test_oracle_pinning.py")])
    if rc != 0:
        sys.exit("the oracle disagrees with the live reference: nothing written")
    rec = L.recorded_reference()
    rec.save()
    print("%d answers -> %s" % (len(rec.table), L.ANSWERS))


if __name__ == "__main__":
    main()

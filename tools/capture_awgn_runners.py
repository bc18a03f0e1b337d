#!/usr/bin/env python3
"""Record tests/golden/G20_awgn_runners.npz: every array (and, for the verbose calls, the printed text) that the cases of
tests/test_awgn_runners_bits_gpu.py return, computed on an MI355X by the package in use.  Each case runs twice and the two results must agree bit
for bit.  Run it with the code whose output is to be pinned -- never to make a failing test pass.

    python tools/capture_awgn_runners.py [out.npz]        (default: the fixture itself)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import test_awgn_runners_bits_gpu as t


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.FIXTURE + ".npz")
    rec = {}
    for name, fn in t.CASES.items():
        got, again = fn(), fn()
        assert set(got) == set(again) and all(t.same_bits(got[k], again[k]) for k in got), (name, "two calls of the same code disagree")
        rec.update({"%s//%s" % (name, k): np.asarray(v) for k, v in got.items()})
        print(name, {k: (str(np.asarray(v).dtype), np.asarray(v).shape) for k, v in got.items()}, flush=True)
        if "stdout" in got:
            print(str(got["stdout"]), end="", flush=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes,", len(t.CASES), "cases")


if __name__ == "__main__":
    main()

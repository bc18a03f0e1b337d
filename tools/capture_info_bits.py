#!/usr/bin/env python3
"""Record tests/golden/G19_info_bits.npz: AIR, GMI, BER and the four counts of every launch of tests/test_info_bits_gpu.py, computed on an MI355X by
the library in use (VAEQ_LIB=... selects a build), plus a sha256 of each launch's inputs.  Run it with the library whose bits are to be pinned --
never to make a failing test pass.

    python tools/capture_info_bits.py [out.npz]        (default: the fixture itself)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import test_info_bits_gpu as t


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.FIXTURE + ".npz")
    rec = {}
    for kernel, mode, name in t.CASES:
        xs = t.build_inputs(kernel, name)
        got, again = t.run_launch(kernel, mode, xs), t.run_launch(kernel, mode, xs)
        assert all(t.same_bits(got[k], again[k]) for k in t.KEYS), (kernel, mode, name, "two launches of the same build disagree")
        empty = (got["kept"] == 0).reshape(3, -1).all(axis=1)
        if name == t.K0:                                       # one run without a measurement; the other two give what they give when launched alone
            assert empty.sum() == 1, (kernel, mode, got["kept"].tolist())
            for i in np.flatnonzero(~empty):
                alone = t.run_launch(kernel, mode, [xs[i]])
                assert all(t.same_bits(got[k][i:i + 1], alone[k]) and np.isfinite(alone[k]).all() for k in t.KEYS), (kernel, mode, i)
        for k in t.KEYS[:3]:
            assert np.isnan(got[k].reshape(3, -1)[empty]).all() and np.isfinite(got[k].reshape(3, -1)[~empty]).all(), (kernel, mode, name, k)
        rec["%s/%s/sha256" % (kernel, name)] = np.array(t.digest(kernel, xs))
        rec.update({"%s/%s/%s/%s" % (kernel, mode, name, k): v for k, v in got.items()})
        print(kernel, mode, name, "GMI", got["GMI"].ravel().tolist(), "kept", got["kept"].ravel().tolist(), "hyp", got["hyp"].ravel().tolist())
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes,", len(t.CASES), "launches")


if __name__ == "__main__":
    main()

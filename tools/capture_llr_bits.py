#!/usr/bin/env python3
"""Record tests/golden/G22_llr_bits.npz: one sha256 per row of LLR planes of every launch of tests/test_llr_bits_gpu.py and the seven arrays of
every vaeq_awgn_track_info launch, computed on an MI355X by the library in use (VAEQ_LIB=... selects a build), plus a sha256 of each launch's
inputs.  The hypotheses of the DP, AWGN and CMA launches are the recorded ones of tests/golden/G19_info_bits.npz, those of the track launches the
ones recorded here.  Run it with the library whose bits are to be pinned -- never to make a failing test pass.

    python tools/capture_llr_bits.py [out.npz]        (default: the fixture itself)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import test_llr_bits_gpu as t


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.FIXTURE + ".npz")
    figures, rec = t.load_golden(t.G.FIXTURE), {}
    for kernel, mode, name in t.CASES:
        xs = t.build_inputs(kernel, name)
        case = "%s/%s/%s" % (kernel, mode, name)
        rec["%s/%s/sha256" % (kernel, name)] = np.array(t.digest(kernel, xs))
        if kernel == "track":
            got, again = t.run_track_info(xs), t.run_track_info(xs)
            assert all(t.G.same_bits(got[k], again[k]) for k in t.KEYS), (case, "two launches of the same build disagree")
            empty = got["kept"] == 0
            for k in t.KEYS[:3]:
                assert np.isnan(got[k][empty]).all() and np.isfinite(got[k][~empty]).all(), (case, k)
            if name in t.K0_TRACK:
                assert empty.tolist() == [False, True, False], (case, got["kept"].tolist())
            rec.update({"%s/%s" % (case, k): v for k, v in got.items()})
        kept, hyp = t.recorded_figures(kernel, mode, name, rec, figures)
        llr, again = t.run_llr(kernel, mode, xs, hyp), t.run_llr(kernel, mode, xs, hyp)
        rows = t.row_digests(llr)
        assert (rows == t.row_digests(again)).all(), (case, "two launches of the same build disagree")
        assert ((rows == t.zero_digest(llr)) == (kept == 0)).all() and np.isfinite(llr).all(), (case, kept.tolist())
        if name == t.G.K0 or name in t.K0_TRACK:               # one run without an LLR; the other two give what they give when launched alone
            empty = (kept == 0).reshape(3, -1).all(axis=1)
            assert empty.sum() == 1, (case, kept.tolist())
            for i in np.flatnonzero(~empty):
                assert (t.row_digests(t.run_llr(kernel, mode, [xs[i]], hyp[i:i + 1])) == rows[i:i + 1]).all(), (case, i)
        rec[case + "/llr"] = rows
        print(case, "kept", kept.ravel().tolist(), "hyp", hyp.ravel().tolist(), "llr", [r[:8] for r in rows.ravel()])
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes,", len(t.CASES), "launches")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/G23_dp_wave_b100_short_phases.npz: every output of the launch forms of tests/test_dp_wave_short_phases_gpu.py, computed on an
MI355X by the library in use (VAEQ_LIB=... selects a build).  Run it with the library whose bits are to be pinned -- never to make a failing test pass.

    python tools/capture_dp_wave_short_phases.py <commit of the library in use> [out.npz]        (default: the fixture itself)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import test_dp_wave_short_phases_gpu as t


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", t.FIXTURE + ".npz")
    rec = {"parent_commit": np.array(commit)}
    for name in sorted(t.CASES):
        rx = t.make_rx(name)
        got, kernel = t.run_case(name, rx)
        again, _ = t.run_case(name, rx)
        assert kernel == t.CASES[name]["kernel"], (name, kernel)
        assert all(np.array_equal(t.bits(got[k]), t.bits(again[k])) for k in got), name + ": two launches of the same build disagree"
        assert all(np.isfinite(v).all() for v in got.values()), name
        rec[name + "/rx_sha256"] = np.array(t.rx_digest(rx))
        rec.update({name + "/" + k: v for k, v in got.items()})
        zeros = {k: (int(np.sum(t.bits(v) == 0x80000000)), int(np.sum(t.bits(v) == 0))) for k, v in got.items() if v.dtype == np.float32}
        print(name, kernel, {k: v.shape for k, v in got.items()}, "loss", got["loss"][:, -1, -1], "(-0, +0) per array", zeros)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

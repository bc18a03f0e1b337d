#!/usr/bin/env python3
"""Time the two baseline LLR kernels (GPU): vaeq_cma_epilogue_llr against vaeq_cma_epilogue_info on the same inputs and against a device copy
that moves the same number of bytes, vaeq_awgn_track_llr (planar and interleaved) likewise against vaeq_awgn_track_info -- alternating the three
calls of a group (A B C A B C ...) with device events after a warm-up, median / min / max per call.

    python tools/probe_baseline_llr.py [--runs 8192] [--symbols 10000] [--track-symbols 15000] [--small-runs 15] [--rounds 10] [--what cma,track]

A call's bytes are what it must move once: the samples and TX reference it reads plus the 2 b planes it writes, per (polarisation) symbol
(64-QAM: 8 B of y + 4 B of fp16 TX in, 24 B out; the CMA kernel reads y and TX a second time for the radius walk, which is not counted).  The
copy reads half of that and writes half of that.  --small-runs adds the CMA group at that many runs (the default DP sweep), where the grid
decides (the two pure grids of profiles/baseline_llr/probe.txt were builds with CMA_LLR_SPLIT_MAX_R of vaeq_cma_llr.hip set to 0 resp. INT_MAX,
run under VAEQ_LIB, which the lib field names).
The frames are synthetic (64-QAM levels plus noise).  One JSON line per group.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vae_equalizer_amd import engine  # noqa: E402


def time_group(kern, rounds):
    for f in kern.values():                                                    # warm up every shape
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in kern}
    for _ in range(rounds):
        for k, f in kern.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in times.items()}


def report(tag, shape, nbytes, res):
    llr, copy = res["llr"]["median"], res["copy"]["median"]
    print(json.dumps(dict(group=tag, **shape, unit="ms per call (host wrapper + kernel, device events)", **res, bytes_per_call=nbytes,
                          llr_GBps_at_median=round(nbytes / llr / 1e6, 1), copy_GBps_at_median=round(nbytes / copy / 1e6, 1),
                          llr_over_copy=round(llr / copy, 3), llr_over_info=round(llr / res["info"]["median"], 3))), flush=True)


def copier(nbytes, dev):
    a = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


def cma_group(R, N, amp, rounds, dev, g):
    n, b = amp.numel(), 3
    P = torch.full((R, n), 1.0 / n, device=dev)
    var = torch.full((R, 2), 0.0025, device=dev)
    nu = torch.zeros(R, device=dev)
    lev = torch.randint(0, n, (R, 2, 2, N), device=dev, generator=g)
    data = amp[lev].to(torch.float16)
    y = 0.8 * (amp[lev] + 0.05 * torch.randn(R, 2, 2, N, device=dev, generator=g))
    del lev
    sc = torch.tensor([[3, -2]], dtype=torch.int32, device=dev).expand(R, 2).contiguous()     # a stage-c roll, so that the walk wraps
    y = torch.stack([torch.roll(y[:, 0], 3, -1), torch.roll(y[:, 1], -2, -1)], 1).contiguous()   # ya[m] = y[m + shift_c]: TX-aligned after it
    z1, z2 = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, 2, dtype=torch.int32, device=dev)
    al = dict(shift_c=sc, r_c=z1, shift_q=z2, r_q=z1)
    fig = engine.cma_epilogue_info(y, data, amp, P, nu, var, **al)
    hyp = fig["hyp"]
    nb = R * 2 * N * (8 + 4 + 2 * b * 4)
    res = time_group({"llr": lambda: engine.cma_epilogue_llr(y, data, amp, nu, var, hyp=hyp, **al),
                      "info": lambda: engine.cma_epilogue_info(y, data, amp, P, nu, var, **al),
                      "copy": copier(nb, dev)}, rounds)
    report("cma", dict(runs=R, symbols=N, n_lev=n, rounds=rounds, sym_err=int(fig["sym_err"].sum()), lib=os.path.basename(os.environ.get("VAEQ_LIB", "") or "libvaeq_hip.so")), nb, res)


def track_group(R, N, amp, rounds, dev, g, interleaved):
    n, b = amp.numel(), 3
    P = torch.full((R, n), 1.0 / n, device=dev)
    lev = torch.randint(0, n, (R, 2, N), device=dev, generator=g)
    data = amp[lev].to(torch.float16)
    z = 1.3 * (amp[lev] + 0.05 * torch.randn(R, 2, N, device=dev, generator=g))
    del lev
    if interleaved:
        z = torch.complex(z[:, 0], z[:, 1]).contiguous()
    var = torch.full((R,), 0.005, device=dev)
    shift = torch.zeros(R, dtype=torch.int32, device=dev)
    fig = engine.awgn_track_info(z, data, amp, P, var, shift, 11)
    hyp = fig["hyp"]
    nb = R * N * (8 + 4 + 2 * b * 4)
    res = time_group({"llr": lambda: engine.awgn_track_llr(z, data, amp, var, shift, hyp, 11),
                      "info": lambda: engine.awgn_track_info(z, data, amp, P, var, shift, 11),
                      "copy": copier(nb, dev)}, rounds)
    report("track_interleaved" if interleaved else "track_planar", dict(runs=R, symbols=N, n_lev=n, rounds=rounds, sym_err=int(fig["sym_err"].sum())),
           nb, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--track-symbols", type=int, default=15000)
    ap.add_argument("--small-runs", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--what", default="cma,track")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    amp = torch.tensor(np.arange(-7, 8, 2) / np.sqrt(42.0), dtype=torch.float32, device=dev)
    if "cma" in a.what:
        cma_group(a.runs, a.symbols, amp, a.rounds, dev, g)
        torch.cuda.empty_cache()
        if a.small_runs:
            cma_group(a.small_runs, a.symbols, amp, max(a.rounds, 50), dev, g)
    if "track" in a.what:
        for il in (False, True):
            track_group(a.runs, a.track_symbols, amp, a.rounds, dev, g, il)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

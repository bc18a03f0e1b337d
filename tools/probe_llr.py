#!/usr/bin/env python3
"""Time the two LLR kernels (GPU): vaeq_dp_epilogue_llr in q- and y-mode against vaeq_dp_epilogue_info on the same inputs and against a device
copy that moves the same number of bytes, vaeq_awgn_llr likewise against vaeq_awgn_info -- alternating the three calls of a group
(A B C A B C ...) with device events after a warm-up, median / min / max per call.

    python tools/probe_llr.py [--runs 8192] [--symbols 10000] [--awgn-symbols 15000] [--rounds 10] [--what dp,awgn]

A call's bytes are what it must move: the posteriors or samples it reads plus the 2 b planes it writes, per (polarisation) symbol
(y-mode at 64-QAM: 8 B in, 24 B out).  The copy reads half of that and writes half of that.  The frames are synthetic (64-QAM levels plus noise).
One JSON line per group.
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
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
                          llr_over_copy=round(llr / copy, 3))), flush=True)


def copier(nbytes, dev):
    a = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--awgn-symbols", type=int, default=15000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--what", default="dp,awgn")
    a = ap.parse_args()
    R, n, b, B = a.runs, 8, 3, 100
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    amp = torch.tensor(np.arange(-7, 8, 2) / np.sqrt(42.0), dtype=torch.float32, device=dev)
    P = torch.full((R, n), 1.0 / n, device=dev)
    if "dp" in a.what:
        N = a.symbols
        var = torch.full((R, 2), 0.0025, device=dev)
        nu = torch.zeros(R, device=dev)
        lev = torch.randint(0, n, (R, 2, 2, N), device=dev, generator=g)
        data = amp[lev].to(torch.float16)
        y = amp[lev] + 0.05 * torch.randn(R, 2, 2, N, device=dev, generator=g)
        del lev
        shift = torch.zeros(R, 2, dtype=torch.int32, device=dev)
        r = torch.zeros(R, dtype=torch.int32, device=dev)
        hyp = torch.zeros(R, 2, dtype=torch.int32, device=dev)
        shape = dict(runs=R, symbols=N, n_lev=n, batch_len=B, rounds=a.rounds)
        nb = R * 2 * N * (8 + 2 * b * 4)
        report("dp_y", shape, nb, time_group({
            "llr": lambda: engine.dp_epilogue_llr(y=y, amp_levels=amp, nu_sc=nu, var=var, shift=shift, r=r, hyp=hyp, batch_len=B),
            "info": lambda: engine.dp_epilogue_info(y=y, data=data, amp_levels=amp, P=P, nu_sc=nu, var=var, shift=shift, r=r, batch_len=B),
            "copy": copier(nb, dev)}, a.rounds))
        q = engine.soft_demap(y, amp, var, nu)
        nb = R * 2 * N * (2 * n * 4 + 2 * b * 4)
        report("dp_q", shape, nb, time_group({
            "llr": lambda: engine.dp_epilogue_llr(q=q, amp_levels=amp, shift=shift, r=r, hyp=hyp, batch_len=B),
            "info": lambda: engine.dp_epilogue_info(q=q, data=data, amp_levels=amp, P=P, shift=shift, r=r, batch_len=B),
            "copy": copier(nb, dev)}, a.rounds))
        del q, y, data
        torch.cuda.empty_cache()
    if "awgn" in a.what:
        N = a.awgn_symbols
        lev = torch.randint(0, n, (R, 2, N), device=dev, generator=g)
        data = amp[lev].to(torch.float16)
        y = 1.3 * (amp[lev] + 0.05 * torch.randn(R, 2, N, device=dev, generator=g))
        del lev
        am = torch.full((R,), float(amp.abs().mean()), device=dev)
        var = torch.full((R,), 0.005, device=dev)
        shift = torch.zeros(R, dtype=torch.int32, device=dev)
        hyp = torch.zeros(R, dtype=torch.int32, device=dev)
        shape = dict(runs=R, symbols=N, n_lev=n, rounds=a.rounds)
        nb = R * N * (8 + 2 * b * 4)
        report("awgn_y", shape, nb, time_group({
            "llr": lambda: engine.awgn_llr(y=y, amp_levels=amp, amp_mean=am, var=var, shift=shift, hyp=hyp),
            "info": lambda: engine.awgn_info(y=y, data=data, amp_levels=amp, P=P, amp_mean=am, var=var, shift=shift),
            "copy": copier(nb, dev)}, a.rounds))


if __name__ == "__main__":
    main()

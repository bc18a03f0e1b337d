#!/usr/bin/env python3
"""Time vaeq_cma_epilogue_info against vaeq_cma_epilogue, the launch it is added to, on the same frames (GPU): the two kernels are alternated
(A B A B ...) after a warm-up, timed with device events, and reported as median / min / max per kernel.

    python tools/probe_cma_info.py [--runs 8192] [--symbols 10000] [--rounds 10] [--out profiles/cma_info/probe.txt]

The frames are synthetic (64-QAM levels plus noise at a scale the mean-radius normalisation has to undo); the info launch runs on the alignment the
epilogue returns for them.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vae_equalizer_amd import engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cma_info", "probe.txt"))
    a = ap.parse_args()
    R, N, n = a.runs, a.symbols, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    amp = torch.tensor(np.arange(-7, 8, 2) / np.sqrt(42.0), dtype=torch.float32, device=dev)
    P = torch.full((R, n), 1.0 / n, device=dev)
    var = torch.full((R, 2), 0.0025, device=dev)
    nu = torch.zeros(R, device=dev)
    lev = torch.randint(0, n, (R, 2, 2, N), device=dev, generator=g)
    data = amp[lev].to(torch.float16)
    y = (amp[lev] + 0.05 * torch.randn(R, 2, 2, N, device=dev, generator=g)) * 0.8
    del lev
    ep = engine.cma_epilogue(y, data, amp, nu, var)
    align = {k: ep[k] for k in ("shift_c", "r_c", "shift_q", "r_q")}
    kern = {"cma_epilogue_info": lambda: engine.cma_epilogue_info(y, data, amp, P, nu, var, **align),
            "cma_epilogue": lambda: engine.cma_epilogue(y, data, amp, nu, var)}
    for k in kern:                                                             # warm up both shapes
        out = kern[k]()
        if k == "cma_epilogue_info":
            fig = out
    torch.cuda.synchronize()
    times = {k: [] for k in kern}
    for _ in range(a.rounds):
        for k in kern:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kern[k]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"runs": R, "symbols": N, "n_lev": n, "rounds": a.rounds, "unit": "ms per call (host wrapper + kernel, device events)"}
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    res["ratio_of_medians"] = round(res["cma_epilogue_info"]["median"] / res["cma_epilogue"]["median"], 3)
    res["bytes_read_per_call"] = R * N * 2 * (16 + 8)                          # y and tx, each read in both walks
    res["GBps_at_median"] = round(res["bytes_read_per_call"] / res["cma_epilogue_info"]["median"] / 1e6, 1)
    res["GMI_mean"] = round(float(fig["GMI"].mean()), 4)
    res["SER_q_mean"] = round(float(ep["SER"][:, 2:4].mean()), 6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

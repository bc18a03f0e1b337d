#!/usr/bin/env python3
"""Time vaeq_dp_epilogue_info against the epilogue kernel that reads the same data (GPU):
    q-mode against vaeq_dp_epilogue on the same q, y-mode against vaeq_dp_epilogue_compact on the same y,
alternating the two kernels of a pair (A B A B ...) with device events, and report median / min / max per kernel.

    python tools/probe_epilogue_info.py [--runs 8192] [--symbols 10000] [--rounds 10] [--mode both|q|y] [--info-only]

--info-only launches nothing but the new kernel (a few times): the form to put under `rocprofv3 --pmc FETCH_SIZE`, in a run of its own.
The frames are synthetic (64-QAM levels plus noise, demapped by vaeq_soft_demap), built in slices so that no torch temporary is a second q.
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from vae_equalizer_amd import engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--mode", default="both")
    ap.add_argument("--info-only", action="store_true")
    a = ap.parse_args()
    R, N, n, B = a.runs, a.symbols, 8, 100
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    amp = torch.tensor(np.arange(-7, 8, 2) / np.sqrt(42.0), dtype=torch.float32, device=dev)
    P = torch.full((R, n), 1.0 / n, device=dev)
    var = torch.full((R, 2), 0.0025, device=dev)
    nu = torch.zeros(R, device=dev)
    lev = torch.randint(0, n, (R, 2, 2, N), device=dev, generator=g)
    data = amp[lev].to(torch.float16)
    y = amp[lev] + 0.05 * torch.randn(R, 2, 2, N, device=dev, generator=g)
    del lev
    need_q = a.mode in ("both", "q")
    q = eq = dec = None
    if need_q:
        q = engine.soft_demap(y, amp, var, nu)
    if a.mode in ("both", "y") and not a.info_only:
        eq = torch.empty(R, 2, N, device=dev)
        dec = torch.empty(R, 2, 2, N, dtype=torch.int8, device=dev)
        for s in range(0, R, 256):
            qs = q[s:s + 256] if need_q else engine.soft_demap(y[s:s + 256], amp, var[s:s + 256], nu[s:s + 256])
            qs = qs.reshape(-1, 2, 2, n, N)
            eq[s:s + 256] = torch.einsum("i,rpin->rpn", amp, qs[:, :, 0])
            dec[s:s + 256] = qs.argmax(3).to(torch.int8)
    shift = torch.zeros(R, 2, dtype=torch.int32, device=dev)
    r = torch.zeros(R, dtype=torch.int32, device=dev)
    kern = {}
    if need_q:
        kern["info_q"] = lambda: engine.dp_epilogue_info(q=q, data=data, amp_levels=amp, P=P, shift=shift, r=r, batch_len=B)
        kern["dp_epilogue"] = lambda: engine.dp_epilogue(q, y, data, amp, nu, var, batch_len=B)
    if a.mode in ("both", "y"):
        kern["info_y"] = lambda: engine.dp_epilogue_info(y=y, data=data, amp_levels=amp, P=P, nu_sc=nu, var=var, shift=shift, r=r, batch_len=B)
        kern["dp_epilogue_compact"] = lambda: engine.dp_epilogue_compact(eq, dec, y, data, amp, nu, var, batch_len=B)
    if a.info_only:
        for k in ("info_q", "info_y"):
            if k in kern:
                for _ in range(3):
                    out = kern[k]()
        torch.cuda.synchronize()
        print(json.dumps({"info_only": True, "runs": R, "symbols": N, "GMI_mean": float(out["GMI"].mean())}))
        return
    times = {k: [] for k in kern}
    for pair in (("info_q", "dp_epilogue"), ("info_y", "dp_epilogue_compact")):
        if pair[0] not in kern:
            continue
        for k in pair:                                                         # warm up both shapes
            kern[k]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in pair:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                kern[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
    res = {"runs": R, "symbols": N, "n_lev": n, "batch_len": B, "rounds": a.rounds, "unit": "ms per call (host wrapper + kernel, device events)"}
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    if need_q:
        res["q_mode_bytes_per_call"] = R * N * (2 * 2 * n * 4 + 8)
        res["info_q_GBps_at_median"] = round(res["q_mode_bytes_per_call"] / res["info_q"]["median"] / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

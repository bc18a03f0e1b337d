#!/usr/bin/env python3
"""Time vaeq_awgn_info against the validation launch it is an opt-in addition to (GPU):
    y-mode against vaeq_awgn_validate_gen on the same clean frame (8192 runs x 15 000 symbols of 64-QAM),
    q-mode against vaeq_nn_validate on the same noisy frame (2048 runs; the q it reads is vaeq_nn_forward's),
alternating the two kernels of a pair (A B A B ...) after a warm-up, with device events, and print one JSON line per mode with
median / min / max per kernel.

    python tools/probe_awgn_info.py [--runs 8192] [--nn-runs 2048] [--symbols 15000] [--rounds 10] [--mode both|y|q] [--info-only]

--info-only launches nothing but the new kernel (a few times): the form to put under `rocprofv3 --pmc FETCH_SIZE`, in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vae_equalizer_amd import channel as ch, engine  # noqa: E402
from vae_equalizer_amd.func_VAELE_MQAM_shaping import awgn_tables  # noqa: E402
from vae_equalizer_amd.func_VAENN_MQAM import vaenn_tables  # noqa: E402


def alternate(pair, rounds):
    """pair: {name: callable}; -> {name: dict(median, min, max)} in ms per call (host wrapper + kernel, device events)."""
    for f in pair.values():                                                    # warm up both shapes
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in pair}
    for _ in range(rounds):
        for k, f in pair.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in times.items()}


def y_mode(R, N, rounds, info_only, dev):
    sps, M, snr = 2, 25, 24.0
    t = awgn_tables("64-QAM", 0.0270955, snr, "h1", sps)
    eng = engine.AWGNEngine(R, M, t["amps"], t["P"], t["amp_mean"], t["var"], dev, sps)
    frame = ch.generate_awgn_clean_batch_hip(R, N, t["amps"], np.tile(t["P"], (R, 1)), np.full(R, snr, np.float32), t["h_channel"], sps, dev, 1, 0)
    ser, shift, y = eng.validate_clean(frame, 21)
    res = {"mode": "y", "runs": R, "symbols": N, "n_lev": 8, "rounds": rounds, "unit": "ms per call (host wrapper + kernel, device events)"}
    if info_only:
        for _ in range(3):
            out = eng.info(y, frame.data, shift)
        torch.cuda.synchronize()
        res.update(info_only=True, GMI_mean=float(out["GMI"].mean()))
        return res
    res.update(alternate({"awgn_info_y": lambda: eng.info(y, frame.data, shift), "awgn_validate_gen": lambda: eng.validate_clean(frame, 21)}, rounds))
    out = eng.info(y, frame.data, shift)
    res["window_bytes_per_call"] = R * N * 12                                  # 8 B of y + 4 B of TX per symbol; the m_c pass reads y once more
    res["awgn_info_y_GBps_at_median"] = round(res["window_bytes_per_call"] / res["awgn_info_y"]["median"] / 1e6, 1)
    res["ratio_info_to_validate"] = round(res["awgn_info_y"]["median"] / res["awgn_validate_gen"]["median"], 3)
    res["GMI_mean"], res["SER_mean"] = float(out["GMI"].mean()), float(ser.mean())
    return res


def q_mode(R, N, rounds, info_only, dev):
    sps, M, k1, k2, snr = 2, 25, 25, 3, 24.0
    t = vaenn_tables("64-QAM", "h1", sps)
    n = len(t["amps"])
    eng = engine.NNEngine(R, M, k1, k2, t["amps"], dev, sps)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    eng.init_parameters(g)
    sigma = np.full(R, np.sqrt(0.5) / 10 ** (snr / 20), np.float32)
    x, data = ch.generate_awgn_batch_hip(R, N, t["amps"], np.full(n, 1.0 / n), np.full(R, snr, np.float32), t["h_channel"], sps, dev, 1, 0,
                                         sigma_fixed=sigma)
    ser, shift = eng.validate(x, data, 21)
    q = eng.forward(x)
    P = torch.full((R, n), 1.0 / n, device=dev)
    info = lambda: engine.awgn_info(q=q, data=data, amp_levels=eng.amp, P=P, shift=shift)
    res = {"mode": "q", "runs": R, "symbols": N, "n_lev": n, "rounds": rounds, "unit": "ms per call (host wrapper + kernel, device events)"}
    if info_only:
        for _ in range(3):
            out = info()
        torch.cuda.synchronize()
        res.update(info_only=True, GMI_mean=float(out["GMI"].mean()))
        return res
    res.update(alternate({"awgn_info_q": info, "nn_validate": lambda: eng.validate(x, data, 21)}, rounds))
    res["window_bytes_per_call"] = R * N * (2 * n * 4 + 4)
    res["awgn_info_q_GBps_at_median"] = round(res["window_bytes_per_call"] / res["awgn_info_q"]["median"] / 1e6, 1)
    res["ratio_info_to_validate"] = round(res["awgn_info_q"]["median"] / res["nn_validate"]["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--nn-runs", type=int, default=2048)
    ap.add_argument("--symbols", type=int, default=15000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--mode", default="both")
    ap.add_argument("--info-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.mode in ("both", "y"):
        print(json.dumps(y_mode(a.runs, a.symbols, a.rounds, a.info_only, dev)), flush=True)
        torch.cuda.empty_cache()
    if a.mode in ("both", "q"):
        print(json.dumps(q_mode(a.nn_runs, a.symbols, a.rounds, a.info_only, dev)), flush=True)


if __name__ == "__main__":
    main()

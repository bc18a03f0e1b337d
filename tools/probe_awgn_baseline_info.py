#!/usr/bin/env python3
"""Time vaeq_awgn_track_info (and vaeq_awgn_dfe_soft) against the launches they are an opt-in addition to, on the same frames (GPU):
    cma: vaeq_awgn_track_info on the CPE output against vaeq_awgn_cma_validate (8192 runs x 15 000 symbols of 64-QAM at 2 sps),
    dfe: track info on the LMMSE output + vaeq_awgn_dfe_soft + track info on its z against vaeq_awgn_lmmse_eval + vaeq_awgn_dfe
         (the script's 8 SNRs x 5 frames of 128 000 symbols),
alternating the two sides of a pair (A B A B ...) after a warm-up, with device events, and print one JSON line per pair with
median / min / max per side.

    python tools/probe_awgn_baseline_info.py [--runs 8192] [--symbols 15000] [--dfe-symbols 128000] [--rounds 10] [--mode both|cma|dfe] [--info-only]

--info-only launches nothing but the new kernels (a few times): the form to put under `rocprofv3 --pmc FETCH_SIZE`, in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vae_equalizer_amd import DFE_MQAM_shaping as D, channel as ch, engine  # noqa: E402
from vae_equalizer_amd.func_VAELE_MQAM_shaping import awgn_tables  # noqa: E402


def alternate(pair, rounds):
    """pair: {name: callable}; -> {name: dict(median, min, max)} in ms per call (host wrapper + kernels, device events)."""
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


def cma(R, N, rounds, info_only, dev):
    sps, M, snr = 2, 25, 22.0
    t = awgn_tables("64-QAM", 0.0270955, snr, "h1", sps)
    P = np.tile(t["P"], (R, 1))
    rx, data = ch.generate_awgn_batch_hip(R, N, t["amps"], P, np.full(R, snr, np.float32), t["h_channel"], sps, dev, 1, 0)
    h = torch.zeros(R, 2, M, device=dev)
    h[:, 0, M // 2] = 1.0                                                      # the script's initial taps: the kernels' time does not depend on them
    ser, shift, y = engine.awgn_cma_validate(rx, h, data, t["amps"], sps, 21, want_cpe=True)
    info = lambda: engine.awgn_track_info(y, data, t["amps"], P, t["var"], shift, 11)  # noqa: E731
    res = {"pair": "cma", "runs": R, "symbols": N, "n_lev": 8, "rounds": rounds, "unit": "ms per call (host wrapper + kernels, device events)"}
    if info_only:
        for _ in range(3):
            out = info()
        torch.cuda.synchronize()
        res.update(info_only=True, GMI_mean=float(out["GMI"].nanmean()))
        return res
    res.update(alternate({"track_info": info, "awgn_cma_validate": lambda: engine.awgn_cma_validate(rx, h, data, t["amps"], sps, 21, want_cpe=True)},
                         rounds))
    out = info()
    res["window_bytes_per_call"] = R * N * 2 * 12                              # 8 B of z + 4 B of TX per symbol, read by the pre-pass and by the window pass
    res["track_info_GBps_at_median"] = round(res["window_bytes_per_call"] / res["track_info"]["median"] / 1e6, 1)
    res["ratio_info_to_validate"] = round(res["track_info"]["median"] / res["awgn_cma_validate"]["median"], 3)
    res["GMI_mean"], res["SER_mean"] = float(out["GMI"].nanmean()), float(ser.nanmean())
    return res


def dfe(N, rounds, info_only, dev):
    SNRs, E = [int(s) for s in D.SNR_vec], D.num_epochs
    R = len(SNRs) * E
    amps = D.amp_levels.numpy()
    filt = [D._filters(D.h_channel, s) for s in SNRs]
    lm, ff, fb = (torch.stack([filt[r // E][k] for r in range(R)]) for k in range(3))
    P = ch.pcs_probabilities(amps, D.nu)
    rx, data = ch.generate_dfe_batch_hip(R, N, amps, P, np.repeat(np.asarray(SNRs, np.float32), E), D.h_channel, dev, 1, 0)
    var = [10 ** (-SNRs[r // E] / 10) for r in range(R)]
    e = D.N_cut + 11

    def validators():
        ser_m, sh_m, dec_m, out_m = engine.awgn_lmmse_eval(rx, lm, data, amps, D.N_SHIFT_LMMSE, D.N_cut, want_out=True)
        return ser_m, sh_m, out_m, engine.awgn_dfe(rx, ff, fb, dec_m, amps, data, D.N_SHIFT_DFE, D.N_cut, want_ff=True)
    ser_m, sh_m, out_m, r = validators()

    def info():
        a = engine.awgn_track_info(out_m, data, amps, P, var, sh_m, e)
        return a, engine.awgn_track_info(engine.awgn_dfe_soft(r["ff"], fb, r["dec"], amps), data, amps, P, var, r["shift"], e)
    res = {"pair": "dfe", "runs": R, "symbols": N, "n_lev": len(amps), "rounds": rounds, "unit": "ms per call (host wrappers + kernels, device events)"}
    if info_only:
        for _ in range(3):
            a, b = info()
        torch.cuda.synchronize()
        res.update(info_only=True, GMI_mmse_mean=float(a["GMI"].mean()), GMI_dfe_mean=float(b["GMI"].mean()))
        return res
    res.update(alternate({"baseline_info": info, "lmmse_eval+dfe": validators}, rounds))
    a, b = info()
    res["ratio_info_to_validate"] = round(res["baseline_info"]["median"] / res["lmmse_eval+dfe"]["median"], 3)
    res.update(GMI_mmse_mean=float(a["GMI"].mean()), GMI_dfe_mean=float(b["GMI"].mean()), SER_mmse_mean=float(ser_m.mean()),
               SER_dfe_mean=float(r["ser"].mean()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=15000)
    ap.add_argument("--dfe-symbols", type=int, default=128000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--mode", default="both")
    ap.add_argument("--info-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.mode in ("both", "cma"):
        print(json.dumps(cma(a.runs, a.symbols, a.rounds, a.info_only, dev)), flush=True)
        torch.cuda.empty_cache()
    if a.mode in ("both", "dfe"):
        print(json.dumps(dfe(a.dfe_symbols, a.rounds, a.info_only, dev)), flush=True)


if __name__ == "__main__":
    main()

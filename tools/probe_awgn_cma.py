#!/usr/bin/env python3
"""Timing of the AWGN constant-modulus baseline (func_CMA_MQAM_shaping / Eval_run_shaping_cma) on the device: per R in {3, 120, 8192} the
training kernel per 4000-symbol epoch (and per symbol of one wave's chain), the fused validation kernel per 15 000-symbol evaluation, the
device generator's share of an evaluated epoch pair; then the wall time of Eval_run_shaping_cma.main() at the script's own defaults.

Usage: python tools/probe_awgn_cma.py [--skip-main] [--out DIR]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vae_equalizer_amd import channel as ch
from vae_equalizer_amd.engine import awgn_cma, awgn_cma_validate
from vae_equalizer_amd.func_CMA_MQAM_shaping import awgn_tables

DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-main", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t = awgn_tables("64-QAM", 0.0, 22, "h1", 2)
    gen = lambda R, N, f: ch.generate_awgn_batch_hip(R, N, t["amps"], t["P"], 22.0, t["h_channel"], 2, DEV, 5, f)
    amp = torch.tensor(t["amps"], dtype=torch.float32, device=DEV)
    M, Nt, Nv = 25, 4000, 15000
    print(f"device: {torch.cuda.get_device_name(0)}  M = {M}, train_len = {Nt}, N_valid = {Nv}, 64-QAM, h1, 22 dB", flush=True)
    for R in (3, 120, 8192):
        h = torch.zeros(R, 2, M, device=DEV)
        h[:, 0, M // 2] = 1.0
        rx, _ = gen(R, Nt, 0)
        rxv, datav = gen(R, Nv, 1)
        reps = 20 if R < 8192 else 5
        t_train = timed(lambda: awgn_cma(rx, h, 0.5e-4, 2, True), reps)
        t_val = timed(lambda: awgn_cma_validate(rxv, h, datav, amp, 2, 21), reps)
        t_gt = timed(lambda: gen(R, Nt, 2), reps)
        t_gv = timed(lambda: gen(R, Nv, 3), reps)
        pair = t_train + t_val + t_gt + t_gv                                   # one evaluated epoch + one plain epoch (epe = 2)
        pair += t_train + t_gt
        print(f"R={R:5d}: train {t_train:8.3f} ms per {Nt}-symbol epoch ({t_train * 1e3 / Nt:.3f} us per symbol of a run's chain)"
              f" | validate {t_val:8.3f} ms per {Nv}-symbol evaluation | generator train {t_gt:7.3f} ms, valid {t_gv:7.3f} ms"
              f" | generator share of an epe=2 epoch pair {100 * (2 * t_gt + t_gv) / pair:5.1f} %", flush=True)
        del rx, rxv, datav
        torch.cuda.empty_cache()
    if not a.skip_main:
        from vae_equalizer_amd import Eval_run_shaping_cma as ev
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            ev.savePATH = a.out.rstrip("/") + "/"
        t0 = time.time()
        name, d = ev.main()
        wall = time.time() - t0
        S = d["SER"]
        print(f"Eval_run_shaping_cma.main() at its defaults ({ev.iter} runs x {ev.num_epochs} epochs, train_len {ev.train_len}, "
              f"N_valid {ev.N_valid}): {wall:.1f} s wall -> {os.path.basename(name)}; SER of the last 5 evaluations per run: "
              f"{[[round(float(x), 4) for x in S[0, 0, 0, 0, 0, 0, i, -5:]] for i in range(ev.iter)]}", flush=True)


if __name__ == "__main__":
    main()

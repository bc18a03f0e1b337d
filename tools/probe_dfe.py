#!/usr/bin/env python3
"""Times the default sweep of DFE_MQAM_shaping.py (8 SNRs x 5 epochs x 128 000 symbols, 64-QAM, h_1) on one GPU: the whole main()-level
batch, then each stage on its own (generator, LMMSE evaluation, feed-forward FIR, speculative pass, repair pass, DFE evaluation), the
host-chosen chunking C / W and the repaired symbols per frame at each SNR.  Stage times come from separate launches of the same work
(vaeq_awgn_dfe with ser = NULL, C = 1 for the serial cost).

Usage:  python tools/probe_dfe.py [--reps 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from vae_equalizer_amd import DFE_MQAM_shaping as d
    from vae_equalizer_amd import channel as ch
    from vae_equalizer_amd.engine import awgn_dfe, awgn_lmmse_eval, dfe_chunks
    dev = torch.device("cuda:0")
    S, E, N = len(d.SNR_vec), d.num_epochs, d.N_valid
    R = S * E
    amps = d.amp_levels.numpy()
    P = ch.pcs_probabilities(amps, d.nu)
    snr = np.repeat(d.SNR_vec.astype(np.float32), E)
    t_all = timed(lambda: d.run_dfe_batch(d.SNR_vec, E, N, d.mod, d.h_channel_orig, d.nu, seed=1, generator="hip", device=dev), a.reps)
    filt = [d._filters(d.h_channel, int(s)) for s in d.SNR_vec]
    lm, ff, fb = (torch.stack([filt[r // E][k] for r in range(R)]) for k in range(3))
    t_filt = timed(lambda: [d._filters(d.h_channel, int(s)) for s in d.SNR_vec], a.reps)
    rx, data = ch.generate_dfe_batch_hip(R, N, amps, P, snr, d.h_channel, dev, 1, 0)
    t_gen = timed(lambda: ch.generate_dfe_batch_hip(R, N, amps, P, snr, d.h_channel, dev, 1, 0), a.reps)
    t_lm = timed(lambda: awgn_lmmse_eval(rx, lm, data, amps), a.reps)
    _, _, init, _ = awgn_lmmse_eval(rx, lm, data, amps)
    C, W = dfe_chunks(R, N, len(fb[0]))
    one = torch.tensor([1.0 + 0j])
    ffo = awgn_dfe(rx, ff, fb, init, amps, C=1, want_ff=True)["ff"]
    x = torch.stack([ffo.real, ffo.imag], 1).contiguous()
    t_ff_only = timed(lambda: awgn_dfe(rx, ff, fb, init, amps, C=C, W=W), a.reps)           # FIR + spec + repair
    t_id = timed(lambda: awgn_dfe(x, one, fb, init, amps, C=C, W=W), a.reps)               # 1-tap FIR + spec + repair
    t_eval = timed(lambda: awgn_dfe(rx, ff, fb, init, amps, data, C=C, W=W), a.reps) - t_ff_only
    t_serial = timed(lambda: awgn_dfe(x, one, fb, init, amps, C=1), 1)
    r = awgn_dfe(rx, ff, fb, init, amps, data, C=C, W=W)
    rep = r["repairs"].cpu().numpy().reshape(S, E)
    print(f"default sweep: R = {R} frames x N = {N}, 64-QAM h1, C = {C} chunks, W = {W}")
    print(f"main()-level batch (hip generator, filters, LMMSE, DFE, SERs to host): {t_all * 1e3:.2f} ms "
          f"(reference's DFE loop alone at 66 us/symbol on one CPU thread: {R * N * 66e-6:.0f} s)")
    print(f"  host filter design (8 SNRs): {t_filt * 1e3:.2f} ms")
    print(f"  generator (vaeq_gen_awgn, sps 1): {t_gen * 1e3:.3f} ms")
    print(f"  LMMSE eval (FIR + decisions + shift + SER): {t_lm * 1e3:.3f} ms")
    print(f"  feed-forward FIR: {(t_ff_only - t_id) * 1e3:.3f} ms (11 taps minus 1 tap)")
    print(f"  speculative + repair (C = {C}, W = {W}): {t_id * 1e3:.3f} ms")
    print(f"  serial recursion (C = 1): {t_serial * 1e3:.3f} ms")
    print(f"  DFE evaluation (shift + SER): {t_eval * 1e3:.3f} ms")
    for s in range(S):
        print(f"  SNR {int(d.SNR_vec[s])} dB: repaired symbols per frame {rep[s].tolist()}  SER_dfe {r['ser'].cpu().numpy().reshape(S, E)[s].round(4).tolist()}")


if __name__ == "__main__":
    main()

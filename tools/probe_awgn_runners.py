#!/usr/bin/env python3
"""Wall time of one call of each AWGN batch runner (run_awgn_batch, run_awgn_cma_batch, run_vaenn_batch) at the sweep scripts' shapes: R = 20
runs, 40 epochs, epe = 2, generator "hip" with a fixed seed; one warm-up call, then one timed call between two torch.cuda.synchronize().  The
calls are short enough that the host's work per epoch is a visible share of them, which is what this probe is for.

    python tools/probe_awgn_runners.py LABEL [PACKAGE_ROOT]

PACKAGE_ROOT: a directory holding another tree's ``vae_equalizer_amd`` (default: this tree).  Only the public runner functions are used, so the
same file times any two trees: run them alternately, a process each, and compare one tree's median with the other's range.  Prints one line:
LABEL and the three times in milliseconds.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT)
import torch

from vae_equalizer_amd.func_CMA_MQAM_shaping import run_awgn_cma_batch
from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
from vae_equalizer_amd.func_VAENN_MQAM import run_vaenn_batch

R, EPOCHS, EPE, N_VALID = 20, 40, 2, 15000


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    le = [dict(SNR=24, nu=0, lr_optim=5e-3, seed=None) for _ in range(R)]
    cma = [dict(SNR=22, nu=0, lr_optim=0.5e-4, seed=None) for _ in range(R)]
    nn = [dict(SNR=24, lr_optim=4e-3, seed=None) for _ in range(R)]
    ms = (timed(lambda: run_awgn_batch(le, "64-QAM", 2, 25, 350, N_VALID, 1200, EPOCHS, EPE, "h1", generator="hip", seed=1)),
          timed(lambda: run_awgn_cma_batch(cma, "64-QAM", 2, 25, N_VALID, 4000, EPOCHS, EPE, "h1", generator="hip", seed=1)),
          timed(lambda: run_vaenn_batch(nn, "64-QAM", 2, 25, 25, 3, 300, N_VALID, 4000, EPOCHS, EPE, "h1", generator="hip", seed=1)))
    print("%s run_awgn_batch %.2f ms  run_awgn_cma_batch %.2f ms  run_vaenn_batch %.2f ms" % ((sys.argv[1],) + ms))


if __name__ == "__main__":
    main()

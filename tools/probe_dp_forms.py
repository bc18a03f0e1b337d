#!/usr/bin/env python3
"""Time per launch of the other two baked B = 100 forms of the DP wave kernel (8192 runs [argv 1], 5 timed launches): compact = 100 steps with eq / dec
instead of q; flex = 99 VAEflex windows, stride 10, keep_off 45, keep_len 10.  VAEQ_LIB=... python tools/probe_dp_forms.py [R]   (GPU box only)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from vae_equalizer_amd import _native as nat
from vae_equalizer_amd.engine import DPEngine
R = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
amp = (np.arange(-7, 8, 2) / np.sqrt(42.0)).astype(np.float32)
g = torch.Generator(device="cuda:0").manual_seed(0)
for form, steps, kw in (("compact", 100, dict(want_q=False, want_compact=True)), ("flex", 99, dict(stride=10, keep_off=45, keep_len=10))):
    S = ((steps - 1) * kw.get("stride", 100) + 100) * 2
    rx = 0.4 * torch.randn(R, 1, 2, 2, S, device="cuda:0", generator=g)
    eng = DPEngine(R, 25, amp, np.full(8, 1 / 8, np.float32), [0.0025, 0.0025], 0.0, "cuda:0", 2)
    for _ in range(2):
        out = eng.train(rx, 100, steps, 2.5e-3, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        out = eng.train(rx, 100, steps, 2.5e-3, **kw)
    e1.record()
    torch.cuda.synchronize()
    print(f"form {form:8s} {e0.elapsed_time(e1) / 5:9.3f} ms per launch of {steps} steps  {nat.last_kernel()}", flush=True)
    del out, eng, rx

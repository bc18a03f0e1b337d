"""The store path of the baked B = 100 DP wave kernel: its two forms (one 8-byte store per lane and row where keep_off and keep_len are even,
two 4-byte stores otherwise) and the out-of-range mask that drops the symbols outside the kept window, over MORE than one window -- the running
row offset of the q rows and the column of a step both have to advance (tests/test_dp_wave_bits_gpu.py pins the bits, this file the addresses).

Shape: B = 100, M = 25, 64-QAM, 3 runs, 3 steps from the Dirac start, rx = 0.4 * torch.randn with a fixed seed.
  full  keep_off 0, keep_len 100              paired stores         vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>
  flex  stride 10, keep_off 45, keep_len 10   scalar stores (odd offset), 45 of the 50 symbol-pair lanes masked
  even  stride 10, keep_off 44, keep_len 12   paired stores with most lanes masked

1. The default dispatch against the generic kernel (threads = 256, as test_wave_kernel_equals_generic_kernel selects it) on the same inputs.
   The two kernels sum in different orders, so that test compares with tolerances instead of equality; this file uses ITS tolerances:
   loss 2e-6 and y 1e-5 relative, q 2e-4 and W, h 2e-5 absolute.
2. Through the C ABI (vaeq_dp_train) with caller-allocated q and y buffers that carry a guard row in front of and behind the rows the call owns,
   pre-filled with a sentinel: every guard element is still the sentinel afterwards, every element inside is finite and has the bits the engine's
   own call produced.  A wrong running row offset or a lost out-of-range mask lands in a guard row or leaves the sentinel inside.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R, B, M, SPS, STEPS, NLEV = 3, 100, 25, 2, 3, 8
SENTINEL = -7777.0
CASES = {
    "full": dict(stride=100, keep_off=0, keep_len=100, kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
    "flex": dict(stride=10, keep_off=45, keep_len=10, kernel="vaeq::dp_wave_kernel<25, 8, 100, false, 1, 1, 0>"),
    "even": dict(stride=10, keep_off=44, keep_len=12, kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
}
AMP = (np.arange(-7, 8, 2) / np.sqrt(42.0)).astype(np.float32)
LR = 2.5e-3


def _np(t):
    return t.detach().cpu().numpy()


def _engine(threads):
    from vae_equalizer_amd.engine import DPEngine
    return DPEngine(R, M, AMP, np.full(NLEV, 1 / NLEV, np.float32), [0.0025, 0.0025], 0.0, DEV, SPS, threads)


def _window(c):
    return dict(stride=c["stride"], keep_off=c["keep_off"], keep_len=c["keep_len"])


@pytest.fixture(scope="module")
def runs():
    """Per case: rx, and the outputs and final taps of the default dispatch and of the generic kernel (computed once, shared, left unchanged)."""
    from vae_equalizer_amd import _native as nat
    out = {}
    for i, (name, c) in enumerate(sorted(CASES.items())):
        S = ((STEPS - 1) * c["stride"] + B) * SPS
        rx = (0.4 * torch.randn(R, 2, 2, S, generator=torch.Generator().manual_seed(505 + i))).to(DEV)
        res = {"rx": rx}
        for key, threads in (("wave", 0), ("generic", 256)):
            eng = _engine(threads)
            r = eng.train(rx, B, STEPS, LR, **_window(c))
            torch.cuda.synchronize()
            res[key] = dict(q=r["q"], y=r["y"], loss=r["loss"], W=eng.W.clone(), h=eng.h.clone(), kernel=nat.last_kernel())
        out[name] = res
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_store_forms_equal_generic_kernel(name, runs):
    a, b = runs[name]["wave"], runs[name]["generic"]
    No = STEPS * CASES[name]["keep_len"]
    assert a["kernel"] == CASES[name]["kernel"] and "dp_wave_kernel" not in b["kernel"]
    assert tuple(a["q"].shape) == (R, 1, 2, 2 * NLEV, No) and tuple(a["y"].shape) == (R, 1, 2, 2, No)
    for k in ("q", "y", "loss", "W", "h"):
        assert a[k].shape == b[k].shape and bool(torch.isfinite(a[k]).all()), k
    assert relerr(_np(a["loss"]), _np(b["loss"])) < 2e-6
    assert relerr(_np(a["y"]), _np(b["y"])) < 1e-5
    assert np.max(np.abs(_np(a["q"]) - _np(b["q"]))) < 2e-4
    assert np.max(np.abs(_np(a["W"]) - _np(b["W"]))) < 2e-5 and np.max(np.abs(_np(a["h"]) - _np(b["h"]))) < 2e-5


@pytest.mark.parametrize("name", sorted(CASES))
def test_stores_stay_inside_their_rows(name, runs):
    from vae_equalizer_amd import _native as nat
    c, rx, want = CASES[name], runs[name]["rx"], runs[name]["wave"]
    No = STEPS * c["keep_len"]
    eng = _engine(0)
    # [guard row | the rows of the call | guard row], one row = No floats (a multiple of 8 bytes: the kernel's alignment demand holds for the inner view)
    qbuf = torch.full(((R * 4 * NLEV + 2) * No,), SENTINEL, dtype=torch.float32, device=DEV)
    ybuf = torch.full(((R * 4 + 2) * No,), SENTINEL, dtype=torch.float32, device=DEV)
    q, y = qbuf[No:-No], ybuf[No:-No]
    loss = torch.empty(R, 1, STEPS, dtype=torch.float32, device=DEV)
    lr = torch.full((R,), LR, dtype=torch.float32, device=DEV)
    a = nat.DPArgs(R=R, n_frames=1, steps=STEPS, B=B, sps=SPS, M=M, n_lev=NLEV, stride_sym=c["stride"], keep_off=c["keep_off"],
                   keep_len=c["keep_len"], S=rx.shape[-1], rx=nat.ptr(rx), W=nat.ptr(eng.W), h=nat.ptr(eng.h), adam_mW=nat.ptr(eng.mW),
                   adam_vW=nat.ptr(eng.vW), adam_mh=nat.ptr(eng.mh), adam_vh=nat.ptr(eng.vh), step=nat.ptr(eng.step, torch.int32),
                   amp=nat.ptr(eng.amp), P=nat.ptr(eng.P), var=nat.ptr(eng.var), nu_sc=nat.ptr(eng.nu_sc), lr_W=nat.ptr(lr), lr_h=nat.ptr(lr),
                   q_out=nat.ptr(q), y_out=nat.ptr(y), loss=nat.ptr(loss), var_est=None, eq_out=None, dec_out=None, dbg_gW=None, dbg_gh=None,
                   threads=0, no_update=0)
    with torch.cuda.device(DEV):
        nat.check(nat.lib().vaeq_dp_train(C.byref(a), nat.current_stream(torch.device(DEV))), "vaeq_dp_train")
    torch.cuda.synchronize()
    assert nat.last_kernel() == c["kernel"]
    for buf, inner, ref in ((qbuf, q, want["q"]), (ybuf, y, want["y"])):
        assert bool((buf[:No] == SENTINEL).all()) and bool((buf[-No:] == SENTINEL).all()), "a store left the rows of the call"
        assert bool(torch.isfinite(inner).all()) and not bool((inner == SENTINEL).any()), "a kept column was not written"
        assert torch.equal(inner, ref.reshape(-1))
    assert torch.equal(loss, want["loss"]) and torch.equal(eng.W, want["W"]) and torch.equal(eng.h, want["h"])

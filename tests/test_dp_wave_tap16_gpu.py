"""The 16-byte tap reads of the FIR and dL/dU tap loops in the baked B = 100, M = 25 single-wave DP kernel (lds4 and cmac16, csrc/vaeq_wave.h;
pair_fir_carry and pair_du, csrc/vaeq_dp_wave_kernel.h): two taps that are neighbours in LDS arrive as one read.  (The D loop reads its taps 8 bytes at a
time; the one-hot h cases name its taps all the same.)

What can go wrong there: the halves of a read or the two taps of a pair are exchanged, or a pair is taken from the wrong row or offset.  Random taps
catch that only in bulk; these cases name the tap:
  * one-hot W: W is zero except one complex entry W[o, p, k] (re != im != 0) -> y[o] is that tap times the window of polarisation p shifted by k and
    y[1 - o] is exactly zero (numpy, from rx).  k covers both members of both pairs of a stage, the last full stage and the left-over tap;
  * one-hot h: h is zero except h[chi, nu, j], W at the Dirac start -> loss, var_est, dL/dw and dL/dh tap by tap against the C oracle in float32:
    D (through e) and dL/dU (through dL/dy) each see the single tap.
Tolerances: the ones tests/test_dp_kernel_gpu.py and tests/test_dp_wave_cell_carry_gpu.py use (y 2e-6, dL/dh 2e-5, dL/dw 1e-4 of the largest reference
magnitude; loss and var_est 1e-5 relative).
"""
import numpy as np
import pytest
import torch

import oracle
from test_dp_wave_tapgrad_map_gpu import B, DEV, M, SPS, _case, _dev, _engine

pytestmark = pytest.mark.gpu

R = 3
K_W = (0, 1, 2, 3, 23, 24)          # FIR taps: stage 0 (both members of both 16-byte pairs), the last full stage's last tap, the left-over tap
J_H = (0, 1, 2, 3, 22, 23, 24)      # channel taps: the same, and the last tap of the last full dL/dU stage (22, 23: D's last pair)
RE = np.array([0.75, -0.5, 0.625], np.float32)      # per run; re != im != 0
IM = np.array([-0.375, 0.875, 0.25], np.float32)
# One seed per constellation for all 28 one-hot h cases: the first of 400 + n, 410 + n, ... at which the fp32 oracle's own loss, var_est, dL/dh and
# dL/dw are within half the tolerances below of its float64 evaluation for every (chi, nu, j) and all three runs, and its largest |dL/dw| is not
# below 1 -- judged by the oracle alone (onehot_h_seed_ok).
# The noise variances of the case builder are made for 64-QAM.  With W exactly at the Dirac start y sits on the constellation plus the case's
# inter-symbol interference, and with two or four levels the distance to the next level is then 30 .. 80 variances: q is one-hot to the last bit,
# dL/dy is a product of tails exp(-30 .. -80) and the largest |dL/dw| of a run is 1e-27 .. 1e-37 (with random taps it is about 100).  Such a
# gradient is the rounding of whichever stable form of the tail a demapper uses, not a function of the taps, and a tolerance in units of its
# largest magnitude says nothing.  So the variances scale with the squared level spacing, (amp[1] - amp[0])^2 against 64-QAM's: the demapper works at
# the same spacing-to-noise ratio for every n.
SEED_H = {2: 402, 4: 404, 8: 408}
SEED_W = {2: 502, 4: 504, 8: 508}


def _onehot_h(c, chi, nu, j):
    """the case with W at the Dirac start and h zero except h[chi, nu, :, j] = (RE, IM) of the run; var at 64-QAM's spacing-to-noise ratio"""
    c = dict(c)
    c["var"] = (c["var"] * ((c["amp"][1] - c["amp"][0]) / (2.0 / np.sqrt(42.0))) ** 2).astype(np.float32)
    c["W0"] = np.zeros((R, 2, 4, M), np.float32)
    c["W0"][:, 0, 0, M // 2] = c["W0"][:, 1, 1, M // 2] = 1.0
    c["h0"] = np.zeros((R, 2, 2, 2, M), np.float32)
    c["h0"][:, chi, nu, 0, j] = RE
    c["h0"][:, chi, nu, 1, j] = IM
    return c


def _oracle(c, i, dtype):
    return oracle.dp_step_grads(c["rx"][i], c["W0"][i], c["h0"][i], c["amp"], c["P"][i], c["var"][i], float(c["nu_sc"][i]), SPS, dtype)


def _errors(got, ref):
    """(loss rel, var_est rel, dL/dh per tap, dL/dw per tap) of got against ref, the gradients in units of ref's largest magnitude"""
    gh, gW = np.asarray(ref["gh"], np.float64), np.asarray(ref["gW"], np.float64)
    el = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    ev = np.max(np.abs(np.asarray(got["var_est"], np.float64) - ref["var_est"]) / np.abs(ref["var_est"]))
    eh = np.max(np.abs(got["gh"] - gh), axis=(0, 1, 2)) / np.max(np.abs(gh))
    ew = np.max(np.abs(got["gW"] - gW), axis=(0, 1)) / np.max(np.abs(gW))
    return el, ev, eh, ew


def onehot_h_seed_ok(n, seed):
    """the oracle alone: fp32 against float64 within half the tolerances, every one-hot h case of the seed (runs on the CPU)"""
    c0 = _case(R, n, 1, seed)
    for chi in range(2):
        for nu in range(2):
            for j in J_H:
                c = _onehot_h(c0, chi, nu, j)
                for i in range(R):
                    t32 = _oracle(c, i, np.float32)
                    el, ev, eh, ew = _errors(t32, _oracle(c, i, np.float64))
                    if not (el < 5e-6 and ev < 5e-6 and eh.max() < 1e-5 and ew.max() < 5e-5 and np.max(np.abs(t32["gW"])) >= 1.0):
                        return False
    return True


@pytest.mark.parametrize("k", K_W)
@pytest.mark.parametrize("n", [2, 4, 8])
def test_one_hot_w_gives_the_shifted_window_times_the_tap(n, k):
    """One teacher-forced step of 3 runs for every (o, p): y[o] = W[o, p, k] x[p] shifted by k, y[1 - o] = 0."""
    from vae_equalizer_amd import _native as nat
    c = _case(R, n, 1, SEED_W[n])
    x = c["rx"].astype(np.float64)                                        # [R, p, I / Q, 2 B]
    s = np.arange(B) * SPS + k - M // 2                                   # the sample tap k meets at symbol nn (zero outside the window)
    ok = (s >= 0) & (s < B * SPS)
    win = np.where(ok, x[..., np.clip(s, 0, B * SPS - 1)], 0.0)           # [R, p, I / Q, B]
    for o in range(2):
        for p in range(2):
            c["W0"] = np.zeros((R, 2, 4, M), np.float32)
            c["W0"][:, o, p, k] = RE
            c["W0"][:, o, 2 + p, k] = IM
            c["h0"] = np.zeros((R, 2, 2, 2, M), np.float32)
            c["h0"][:, 0, 0, 0, M // 2] = c["h0"][:, 1, 1, 0, M // 2] = 1.0
            eng = _engine(c)
            r = eng.train(_dev(c["rx"]), B, 1, c["lr"], debug_grads=True, no_update=True)
            torch.cuda.synchronize()
            assert nat.last_kernel().startswith(f"vaeq::dp_wave_kernel<{M}, {n}, {B}, true, 1, 1, 0>"), nat.last_kernel()
            y = r["y"].cpu().numpy()[:, 0]                                # [R, o, I / Q, B]
            re, im = RE.astype(np.float64)[:, None], IM.astype(np.float64)[:, None]
            ref = np.stack([re * win[:, p, 0] - im * win[:, p, 1], re * win[:, p, 1] + im * win[:, p, 0]], axis=1)
            err = np.max(np.abs(y[:, o] - ref)) / np.max(np.abs(ref))
            print(f"n_lev {n} W[{o}, {p}, {k}]: y[{o}] {err:.2e} of its largest magnitude")
            assert err < 2e-6, (n, o, p, k, err)
            assert np.all(y[:, 1 - o] == 0.0), (n, o, p, k, "y of the other output polarisation must be exactly zero")


@pytest.mark.parametrize("j", J_H)
@pytest.mark.parametrize("n", [2, 4, 8])
def test_one_hot_h_against_the_oracle(n, j):
    """One teacher-forced step of 3 runs for every (chi, nu): loss, var_est, dL/dh and dL/dw tap by tap against the fp32 C oracle."""
    from vae_equalizer_amd import _native as nat
    c0 = _case(R, n, 1, SEED_H[n])
    for chi in range(2):
        for nu in range(2):
            c = _onehot_h(c0, chi, nu, j)
            eng = _engine(c)
            r = eng.train(_dev(c["rx"]), B, 1, c["lr"], debug_grads=True, no_update=True)
            torch.cuda.synchronize()
            assert nat.last_kernel().startswith(f"vaeq::dp_wave_kernel<{M}, {n}, {B}, true, 1, 1, 0>"), nat.last_kernel()
            loss, ve = r["loss"].cpu().numpy()[:, 0, 0], r["var_est"].cpu().numpy()[:, 0, :, 0]
            gW, gh = r["gW"].cpu().numpy(), r["gh"].cpu().numpy()
            for i in range(R):
                got = dict(loss=loss[i], var_est=ve[i], gW=gW[i], gh=gh[i])
                assert all(np.all(np.isfinite(v)) for v in got.values())
                el, ev, eh, ew = _errors(got, _oracle(c, i, np.float32))
                print(f"n_lev {n} h[{chi}, {nu}, {j}] run {i}: loss {el:.2e}  var_est {ev:.2e}  dL/dh worst tap {int(np.argmax(eh))}: {eh.max():.2e}"
                      f"   dL/dw worst tap {int(np.argmax(ew))}: {ew.max():.2e}")
                assert el < 1e-5 and ev < 1e-5, (n, chi, nu, j, i, el, ev)
                for t in range(M):
                    assert eh[t] < 2e-5, ("dL/dh", n, chi, nu, j, i, t, eh[t])
                    assert ew[t] < 1e-4, ("dL/dw", n, chi, nu, j, i, t, ew[t])

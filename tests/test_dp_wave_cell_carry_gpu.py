"""The carried cells of the convolution-shaped tap loops (FIR, dL/dU, D) in the baked B = 100, M = 25 single-wave DP kernel (CellCarry and
pipe2_carry, csrc/vaeq_dp_wave_kernel.h, csrc/vaeq_wave.h): a stage takes the cells it shares with the stage before from registers.

What can go wrong there and what catches it:
  * a wrong carried operand in the FIR -> y of every symbol against the C oracle; the lanes whose first and last stages read halo cells (symbols
    0, 1 and 98, 99) and a mid-frame pair are asserted by name;
  * a wrong carried operand in D or dL/dU -> dL/dh and dL/dw tap by tap against the C oracle (D feeds the residual, dL/dU feeds dL/dy);
  * one of the kernel's three output forms left behind, or a carry that leaks from one run (workgroup) or array into the next -> loss and taps bit
    for bit between the forms, and between a run trained alone and the same run inside the batch.
Tolerances: the ones tests/test_dp_kernel_gpu.py uses (y 2e-6, dL/dh 2e-5, dL/dw 1e-4 of the largest reference magnitude).  y is compared with the
oracle evaluated in float64, so that the bound covers the kernel's own fp32 sums of 50 products and not two of them.
"""
import numpy as np
import pytest
import torch

import oracle
from test_dp_wave_tapgrad_map_gpu import B, DEV, M, SPS, _case, _dev, _engine, _state

pytestmark = pytest.mark.gpu

# One case per constellation.  With two levels the demapper saturates in most draws of the case builder (Var_q ~ 0: the largest |dL/dw| of a run falls
# from ~100 to 1e-1 .. 3e-4, and the fp32 oracle then differs from its own float64 evaluation by 1e-4 .. 2e-2 of it): 352 is the first seed of
# 302, 312, ... at which the fp32 oracle's own dL/dw is within 5e-5 (half the tolerance) of the float64 one for all three runs -- judged by the oracle alone.
SEED = {2: 352, 4: 304, 8: 308}
NAMED = {"first pair (halo below)": (0, 1), "mid-frame pair": (48, 49), "last pair (halo above)": (98, 99)}


@pytest.mark.parametrize("n", [2, 4, 8])
def test_one_teacher_forced_step_against_the_oracle(n):
    """One step of 3 runs with their own P, var, nu_sc, lr and non-trivial taps: y of every symbol, dL/dw and dL/dh tap by tap."""
    from vae_equalizer_amd import _native as nat
    R = 3
    c = _case(R, n, 1, SEED[n])
    eng = _engine(c)
    r = eng.train(_dev(c["rx"]), B, 1, c["lr"], debug_grads=True)
    torch.cuda.synchronize()
    assert nat.last_kernel().startswith(f"vaeq::dp_wave_kernel<{M}, {n}, {B}, true, 1, 1, 0>"), nat.last_kernel()
    y, gW, gh = r["y"].cpu().numpy()[:, 0], r["gW"].cpu().numpy(), r["gh"].cpu().numpy()
    for i in range(R):
        args = (c["rx"][i], c["W0"][i], c["h0"][i], c["amp"], c["P"][i], c["var"][i], float(c["nu_sc"][i]), SPS)
        t, t64 = oracle.dp_step_grads(*args, np.float32), oracle.dp_step_grads(*args, np.float64)
        ref = np.asarray(t64["out"], np.float64).reshape(2, 2, B)
        sy = np.max(np.abs(ref))
        ey = np.max(np.abs(y[i].astype(np.float64) - ref), axis=(0, 1)) / sy           # per symbol
        sh, sw = np.max(np.abs(t["gh"])), np.max(np.abs(t["gW"]))
        eh = np.max(np.abs(gh[i] - t["gh"]), axis=(0, 1, 2)) / sh                       # per tap j
        ew = np.max(np.abs(gW[i] - t["gW"]), axis=(0, 1)) / sw                          # per tap k
        print(f"n_lev {n} run {i}: y worst symbol {int(np.argmax(ey))}: {ey.max():.2e}   dL/dh worst tap {int(np.argmax(eh))}: {eh.max():.2e}"
              f"   dL/dw worst tap {int(np.argmax(ew))}: {ew.max():.2e}")
        assert np.all(np.isfinite(y[i])) and np.all(np.isfinite(gh[i])) and np.all(np.isfinite(gW[i]))
        for name, syms in NAMED.items():
            for s in syms:
                assert ey[s] < 2e-6, (name, n, i, s, ey[s])
        assert ey.max() < 2e-6, ("y", n, i, int(np.argmax(ey)), ey.max())
        for j in range(M):
            assert eh[j] < 2e-5, ("dL/dh", n, i, j, eh[j])
            assert ew[j] < 1e-4, ("dL/dw", n, i, j, ew[j])


@pytest.mark.parametrize("n", [2, 4, 8])
def test_four_free_steps_in_the_three_output_forms(n):
    """4 free steps of 3 runs in the bench form (q and y of every symbol), the compact form (eq / dec instead of q) and the VAEflex form (stride 10,
    keep_off 45, the centre 10 symbols kept).  The bench and compact forms get the VAEflex form's four windows laid end to end: every step sees
    the same minibatch -- loss, var_est, taps and moments bit for bit the same."""
    from vae_equalizer_amd import _native as nat
    R, steps, fs = 3, 4, 10
    c = _case(R, n, steps, 310 + n, stride=fs)
    rx_flex = c["rx"]
    rx_full = np.concatenate([rx_flex[..., s * fs * SPS:s * fs * SPS + B * SPS] for s in range(steps)], axis=-1)
    got, names = {}, {}
    for form, rx, kw in (("bench", rx_full, {}), ("compact", rx_full, dict(want_q=False, want_compact=True)),
                         ("flex", rx_flex, dict(stride=fs, keep_off=45, keep_len=fs))):
        eng = _engine(c)
        r = eng.train(_dev(rx), B, steps, c["lr"], **kw)
        torch.cuda.synchronize()
        names[form] = nat.last_kernel()
        got[form] = dict(_state(eng), loss=r["loss"].clone(), var_est=r["var_est"].clone())
    assert len(set(names.values())) == 3 and all(f"<{M}, {n}, {B}, " in v for v in names.values()), names
    assert torch.isfinite(got["bench"]["loss"]).all()
    for form in ("compact", "flex"):
        for k in got["bench"]:
            assert torch.equal(got["bench"][k], got[form][k]), (form, k)


@pytest.fixture(scope="module", params=[2, 4, 8])
def four_steps(request):
    """4 free steps of 3 runs as one launch in the bench form: the state and the outputs afterwards."""
    n = request.param
    c = _case(3, n, 4, 320 + n)
    eng = _engine(c)
    r = eng.train(_dev(c["rx"]), B, 4, c["lr"])
    torch.cuda.synchronize()
    return c, _state(eng), {k: r[k].clone() for k in ("loss", "var_est", "y", "q")}


@pytest.mark.parametrize("i", [0, 1, 2])
def test_a_run_trained_alone_equals_the_run_in_the_batch(four_steps, i):
    """R = 1: run i with its own constants equals row i of the R = 3 launch bit for bit -- taps, moments, loss, y and q."""
    c, one, out = four_steps
    eng = _engine(c, slice(i, i + 1))
    r = eng.train(_dev(c["rx"][i:i + 1]), B, 4, c["lr"][i:i + 1])
    torch.cuda.synchronize()
    alone = _state(eng)
    for k in one:
        assert torch.equal(one[k][i:i + 1], alone[k]), k
    for k in out:
        assert torch.equal(out[k][i:i + 1], r[k]), k

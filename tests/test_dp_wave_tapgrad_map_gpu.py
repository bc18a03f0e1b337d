"""The tap-pair lane map of the two tap gradients (dL/dh, dL/dw) in the baked B = 100, M = 25 single-wave DP kernel (TapPairMap,
csrc/vaeq_dp_wave_kernel.h): a lane sums two neighbouring taps of one parity for one chi (resp. o) and ends up owning one of them.

What can go wrong there and what catches it:
  * a chain summed on the wrong lane, a wrong carried operand in the first or last term of a half -> the gradients, tap by tap, against the C oracle;
  * an Adam moment row loaded or stored under the old lane map -> state round trips through the state arrays, bit for bit;
  * one of the kernel's three output forms left behind -> loss and taps of the same run, bit for bit, between the forms.
Tolerances of the gradients: the ones tests/test_dp_kernel_gpu.py uses (dL/dh 2e-5, dL/dw 1e-4 of the largest reference magnitude).
"""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, SPS, M = 100, 2, 25


def _amp(n):
    a = np.arange(-(n - 1), n, 2).astype(np.float64)
    return (a / np.sqrt(2.0 * np.mean(a * a))).astype(np.float32)


def _case(R, n, steps, seed, stride=B):
    """R runs with their own PCS table, noise variances, shaping scale and learning rate; a received signal made of the runs' own symbols through
    a short channel (so that the equalizer's outputs sit near the constellation) and non-trivial taps (Dirac + noise on every tap)."""
    rng = np.random.default_rng(seed)
    amp = _amp(n)
    P = rng.dirichlet(np.ones(n) * 6, R).astype(np.float32)
    var = rng.uniform(0.002, 0.006, (R, 2)).astype(np.float32)
    nu_sc = rng.uniform(0.0, 0.3, R).astype(np.float32)
    lr = rng.uniform(1e-3, 4e-3, R).astype(np.float32)
    S = ((steps - 1) * stride + B) * SPS
    sym = amp[rng.integers(0, n, (R, 2, 2, S // SPS))]
    up = np.repeat(sym, SPS, axis=-1)
    rx = up + 0.25 * np.roll(up, 1, axis=-1) - 0.15 * np.roll(up[:, ::-1], 2, axis=-1) + 0.04 * rng.standard_normal(up.shape)
    W0 = np.zeros((R, 2, 4, M), np.float32)
    h0 = np.zeros((R, 2, 2, 2, M), np.float32)
    W0[:, 0, 0, M // 2] = W0[:, 1, 1, M // 2] = 1.0
    h0[:, 0, 0, 0, M // 2] = h0[:, 1, 1, 0, M // 2] = 1.0
    W0 += 0.03 * rng.standard_normal(W0.shape).astype(np.float32)
    h0 += 0.03 * rng.standard_normal(h0.shape).astype(np.float32)
    return dict(amp=amp, P=P, var=var, nu_sc=nu_sc, lr=lr, rx=np.ascontiguousarray(rx, np.float32), W0=W0, h0=h0)


def _engine(c, runs=None):
    from vae_equalizer_amd.engine import DPEngine
    i = slice(None) if runs is None else runs
    eng = DPEngine(len(c["lr"][i]), M, c["amp"], c["P"][i], c["var"][i], c["nu_sc"][i], DEV, SPS)
    eng.set_state(c["W0"][i], c["h0"][i])
    return eng


def _state(eng):
    return {k: getattr(eng, k).clone() for k in ("W", "h", "mW", "vW", "mh", "vh", "step")}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("n", [8, 2, 4])
def test_tap_gradients_against_the_oracle_tap_by_tap(n):
    """One teacher-forced step of 3 runs: debug_grads against the fp32 C oracle, every tap of dL/dh and dL/dw on its own."""
    from vae_equalizer_amd import _native as nat
    R = 3
    c = _case(R, n, 1, 100 + n)
    eng = _engine(c)
    r = eng.train(_dev(c["rx"]), B, 1, c["lr"], debug_grads=True)
    torch.cuda.synchronize()
    assert nat.last_kernel().startswith(f"vaeq::dp_wave_kernel<{M}, {n}, {B}, true, 1, 1, 0>"), nat.last_kernel()
    gW, gh = r["gW"].cpu().numpy(), r["gh"].cpu().numpy()
    for i in range(R):
        t = oracle.dp_step_grads(c["rx"][i], c["W0"][i], c["h0"][i], c["amp"], c["P"][i], c["var"][i], float(c["nu_sc"][i]), SPS, np.float32)
        sh, sw = np.max(np.abs(t["gh"])), np.max(np.abs(t["gW"]))
        eh = np.max(np.abs(gh[i] - t["gh"]), axis=(0, 1, 2)) / sh       # per tap j
        ew = np.max(np.abs(gW[i] - t["gW"]), axis=(0, 1)) / sw          # per tap k
        print(f"n_lev {n} run {i}: dL/dh worst tap {int(np.argmax(eh))}: {eh.max():.2e}   dL/dw worst tap {int(np.argmax(ew))}: {ew.max():.2e}")
        assert np.all(np.isfinite(gh[i])) and np.all(np.isfinite(gW[i]))
        for j in range(M):
            assert eh[j] < 2e-5, ("dL/dh", n, i, j, eh[j])
            assert ew[j] < 1e-4, ("dL/dw", n, i, j, ew[j])


@pytest.fixture(scope="module")
def four_steps():
    """4 free steps of 3 runs as one launch: the state afterwards."""
    c = _case(3, 8, 4, 7)
    eng = _engine(c)
    eng.train(_dev(c["rx"]), B, 4, c["lr"], want_q=False)
    torch.cuda.synchronize()
    return c, _state(eng)


def test_state_round_trip_through_the_state_arrays(four_steps):
    """The same 4 steps as 2 + 2 launches: taps, all four Adam moment arrays and the step counts come back bit for bit."""
    c, one = four_steps
    eng = _engine(c)
    half = 2 * B * SPS
    eng.train(_dev(c["rx"][..., :half]), B, 2, c["lr"], want_q=False)
    eng.train(_dev(c["rx"][..., half:]), B, 2, c["lr"], want_q=False)
    torch.cuda.synchronize()
    two = _state(eng)
    for k in one:
        assert torch.equal(one[k], two[k]), k
    assert float(one["mh"].abs().min()) > 0.0 and float(one["vW"].abs().min()) > 0.0      # every moment was written


@pytest.mark.parametrize("i", [0, 1, 2])
def test_a_run_trained_alone_equals_the_run_in_the_batch(four_steps, i):
    """R = 1: run i with its own constants, as one launch and as 2 + 2, equals row i of the R = 3 launch bit for bit."""
    c, one = four_steps
    half = 2 * B * SPS
    for split in (False, True):
        eng = _engine(c, slice(i, i + 1))
        if split:
            eng.train(_dev(c["rx"][i:i + 1, ..., :half]), B, 2, c["lr"][i:i + 1], want_q=False)
            eng.train(_dev(c["rx"][i:i + 1, ..., half:]), B, 2, c["lr"][i:i + 1], want_q=False)
        else:
            eng.train(_dev(c["rx"][i:i + 1]), B, 4, c["lr"][i:i + 1], want_q=False)
        torch.cuda.synchronize()
        alone = _state(eng)
        for k in one:
            assert torch.equal(one[k][i:i + 1], alone[k]), (k, split)


def test_the_three_output_forms_train_the_same_run():
    """3 steps of 2 runs in the bench form (q and y of every symbol), the compact form (eq / dec instead of q) and the VAEflex form (stride 10, the
    centre 10 symbols kept): the bench and compact forms get the VAEflex form's three windows laid end to end, so every step sees the same
    minibatch -- loss, var_est, taps and moments bit for bit the same."""
    from vae_equalizer_amd import _native as nat
    R, steps, fs = 2, 3, 10
    c = _case(R, 8, steps, 11, stride=fs)
    rx_flex = c["rx"]
    rx_full = np.concatenate([rx_flex[..., s * fs * SPS:s * fs * SPS + B * SPS] for s in range(steps)], axis=-1)
    got, names = {}, {}
    for form, rx, kw in (("bench", rx_full, {}), ("compact", rx_full, dict(want_q=False, want_compact=True)),
                         ("flex", rx_flex, dict(stride=fs, keep_off=(B - fs) // 2, keep_len=fs))):
        eng = _engine(c)
        r = eng.train(_dev(rx), B, steps, c["lr"], **kw)
        torch.cuda.synchronize()
        names[form] = nat.last_kernel()
        got[form] = dict(_state(eng), loss=r["loss"].clone(), var_est=r["var_est"].clone())
    assert len(set(names.values())) == 3 and all(f"<{M}, 8, {B}, " in v for v in names.values()), names
    for form in ("compact", "flex"):
        for k in got["bench"]:
            assert torch.equal(got["bench"][k], got[form][k]), (form, k)

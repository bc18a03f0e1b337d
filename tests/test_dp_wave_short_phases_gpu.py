"""Pinned bits of the short phases of the baked B = 100 DP wave kernel -- the wave sums and prefix scans, the half combines and the two Adam
updates -- on inputs that the random frames of tests/test_dp_wave_bits_gpu.py and tests/test_dp_wave_b100_more_bits_gpu.py never produce.
Every array must equal, bit for bit, what the kernel computed when `tests/golden/G23_dp_wave_b100_short_phases.npz` was recorded
(tools/capture_dp_wave_short_phases.py, on an MI355X, with the library of the commit named in the fixture's `parent_commit`: the one before
the masked DPP steps kept their destination and the Adam updates ran on (re, im) pairs).

Floats are compared as uint32 views: np.array_equal calls -0 and +0 equal, and a -0 that turns into +0 is exactly what a DPP step that keeps
its destination (instead of adding a masked zero) could hide.

R = 5 runs, B = 100, M = 25, 2 samples per symbol, one frame of 3 steps from the Dirac start.  The runs (see make_rx):
  0  an all-zero frame: every input of every sum and scan is +-0 or the same positive constant
  1  polarisation 0 is zero, polarisation 1 a random frame
  2  constellation points on the symbol samples, 1e-3 noise between them, var = 1e-4: q is one-hot, the variance moments underflow to 0,
     the residuals are tiny
  3  a random frame
  4  a random frame whose second window is all zero (a zero window after the taps have moved)
Forms:
  qam64_all    64-QAM, q, y and the compact outputs                 -> vaeq::dp_wave_kernel<25, 8, 100, true, 0, 1, 0>
  qam64_cmp    64-QAM, the compact outputs without q                -> vaeq::dp_wave_kernel<25, 8, 100, true, 2, 1, 0>
  qam64_flex   64-QAM VAEflex: stride 10, keep_off 45, keep_len 10  -> vaeq::dp_wave_kernel<25, 8, 100, false, 1, 1, 0>
  qam4         4-QAM, q and y                                       -> vaeq::dp_wave_kernel<25, 2, 100, true, 1, 1, 0>
  qam16        16-QAM, q and y                                      -> vaeq::dp_wave_kernel<25, 4, 100, true, 1, 1, 0>
  qam64_grads  64-QAM, debug_grads: the last step's gW, gh          -> vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>
  qam64_noupd  64-QAM, no_update: taps and Adam state stay put      -> vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>
q is compared (and stored) on every Q_STRIDE-th column; every other array whole.  A run launched alone must give the bits it gives in the batch.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G23_dp_wave_b100_short_phases"
R, B, M, SPS, STEPS = 5, 100, 25, 2, 3
Q_STRIDE = 4
FLEX = dict(stride=10, keep_off=45, keep_len=10)
CASES = {
    "qam64_all": dict(levels=8, train=dict(want_q=True, want_compact=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 0, 1, 0>"),
    "qam64_cmp": dict(levels=8, train=dict(want_q=False, want_compact=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 2, 1, 0>"),
    "qam64_flex": dict(levels=8, train=dict(want_q=True, **FLEX), kernel="vaeq::dp_wave_kernel<25, 8, 100, false, 1, 1, 0>"),
    "qam4": dict(levels=2, train=dict(want_q=True), kernel="vaeq::dp_wave_kernel<25, 2, 100, true, 1, 1, 0>"),
    "qam16": dict(levels=4, train=dict(want_q=True), kernel="vaeq::dp_wave_kernel<25, 4, 100, true, 1, 1, 0>"),
    "qam64_grads": dict(levels=8, train=dict(want_q=False, debug_grads=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
    "qam64_noupd": dict(levels=8, train=dict(want_q=False, no_update=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
}
ALONE = "qam64_all"                                        # the form whose runs are also launched one by one
STATE = ("W", "h", "mW", "vW", "mh", "vh", "step")
OUTPUTS = ("loss", "var_est", "y", "q", "gW", "gh", "eq", "dec")
SHAPING = np.array([0.0, 0.3, 0.8, 1.4, 2.0])
VAR = np.array([[0.0025, 0.0025], [0.004, 0.0015], [1e-4, 1e-4], [0.006, 0.006], [0.0012, 0.03]], np.float32)
LR_W = np.array([2.5e-3, 1e-3, 5e-3, 2e-3, 4e-3], np.float32)
LR_H = np.array([2.5e-3, 2e-3, 1e-3, 4e-3, 3e-3], np.float32)


def amplitudes(n):
    amp = np.arange(-(n - 1), n, 2).astype(np.float64)
    return (amp / np.sqrt(2.0 * np.mean(amp ** 2))).astype(np.float32)          # unit-power square QAM


def make_rx(name):
    """The received samples of a form: seeded on the host, [R, 1 frame, 2 polarisations, I / Q, S] float32 (the five runs: see the module docstring)."""
    c = CASES[name]
    stride = c["train"].get("stride", B)
    S = ((STEPS - 1) * stride + B) * SPS
    rng = np.random.default_rng(23 + sorted(CASES).index(name))
    rx = (0.4 * rng.standard_normal((R, 1, 2, 2, S))).astype(np.float32)
    rx[0] = 0.0
    rx[1, :, 0] = 0.0
    amp = amplitudes(c["levels"])
    rx[2] = (1e-3 * rng.standard_normal((1, 2, 2, S))).astype(np.float32)
    rx[2, ..., 0::SPS] = amp[rng.integers(0, len(amp), (1, 2, 2, S // SPS))]     # the Dirac taps pick the even samples: y lands on the levels
    rx[4, ..., stride * SPS:stride * SPS + B * SPS] = 0.0
    return rx


def rx_digest(rx):
    return hashlib.sha256(np.ascontiguousarray(rx).tobytes()).hexdigest()


def bits(a):
    """The array as integers: float32 as its uint32 view (so that -0 and +0, and two NaNs of different payload, differ)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_case(name, rx, runs=None):
    """One launch of the form on cuda:0 from the Dirac initialisation, of all runs or of the listed ones -> ({array name: numpy array}, kernel name)."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import DPEngine

    c = CASES[name]
    sel = np.arange(R) if runs is None else np.asarray(runs)
    amp = amplitudes(c["levels"])
    P = np.exp(-SHAPING[:, None] * amp.astype(np.float64)[None, :] ** 2)
    P = (P / P.sum(axis=1, keepdims=True)).astype(np.float32)
    eng = DPEngine(len(sel), M, amp, P[sel], VAR[sel], SHAPING.astype(np.float32)[sel], "cuda:0", SPS)
    out = eng.train(torch.from_numpy(np.ascontiguousarray(rx[sel])).cuda(), B, STEPS, LR_W[sel], lr_h=LR_H[sel], **c["train"])
    torch.cuda.synchronize()
    kernel = nat.last_kernel()
    got = {k: getattr(eng, k).cpu().numpy() for k in STATE}
    got.update({k: out[k].cpu().numpy() for k in OUTPUTS if out.get(k) is not None})
    if "q" in got:
        got["q"] = np.ascontiguousarray(got["q"][..., ::Q_STRIDE])
    return got, kernel


@pytest.fixture(scope="module")
def recorded():
    return load_golden(FIXTURE)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dp_wave_b100_short_phases(name, recorded):
    rx = make_rx(name)
    assert rx_digest(rx) == str(recorded[name + "/rx_sha256"]), "the seeded input is not the one the fixture was recorded with"
    got, kernel = run_case(name, rx)
    assert kernel == CASES[name]["kernel"]
    want = {k[len(name) + 1:]: v for k, v in recorded.items() if k.startswith(name + "/") and k != name + "/rx_sha256"}
    t = CASES[name]["train"]
    assert set(got) == set(want) and {"loss", "var_est", "y"} | set(STATE) <= set(want)
    assert ("q" in want) == t["want_q"] and ("gW" in want) == ("gh" in want) == bool(t.get("debug_grads"))
    assert ("eq" in want) == ("dec" in want) == bool(t.get("want_compact"))
    assert int(got["step"][0]) == (0 if t.get("no_update") else STEPS) and np.isfinite(got["loss"]).all()
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        g, w = bits(got[k]), bits(want[k])
        assert np.array_equal(g, w), "%s/%s: %d of %d elements differ in their bits" % (name, k, int(np.sum(g != w)), w.size)


@pytest.mark.parametrize("run", range(R))
def test_run_alone_equals_run_in_batch(run, recorded):
    rx = make_rx(ALONE)
    got, kernel = run_case(ALONE, rx, runs=[run])
    assert kernel == CASES[ALONE]["kernel"]
    for k in sorted(got):
        w = recorded[ALONE + "/" + k][run:run + 1]
        assert got[k].shape == w.shape, k
        assert np.array_equal(bits(got[k]), bits(w)), "run %d alone, %s: bits differ from the same run inside the batch" % (run, k)

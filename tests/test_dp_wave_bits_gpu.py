"""The bits of the B = 100 DP wave kernel, pinned: every output of three launch forms must equal, array for array and bit for bit, what the
kernel computed when `tests/golden/G18_dp_wave_b100_bits.npz` was recorded (tools/capture_dp_wave_bits.py, on an MI355X, with the library of the
commit before the kernel's instruction schedule was first touched).  After a handful of chaotic fp32 Adam steps any change of summation order, of
an operand or of a rounding shows up in these arrays, so a change that only moves instructions passes and nothing else does.

Forms (R = 3 runs, B = 100, M = 25, 64-QAM, 2 samples per symbol, 2 frames per launch):
  bench    4 steps per frame, q and y written                   -> vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>  (the benchmark's kernel)
  compact  4 steps per frame, eq / dec instead of q             -> vaeq::dp_wave_kernel<25, 8, 100, true, 2, 1, 0>
  flex     12 VAEflex windows per frame: stride 10, the 10 centre symbols kept (keep_off 45: scalar stores)
                                                                -> vaeq::dp_wave_kernel<25, 8, 100, false, 1, 1, 0>
The runs differ in their symbol prior, noise variances, nu scale and learning rates, so no per-run constant is pinned at one value only.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G18_dp_wave_b100_bits"
R, B, M, SPS, FRAMES = 3, 100, 25, 2, 2
CASES = {
    "bench": dict(steps=4, train=dict(want_q=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
    "compact": dict(steps=4, train=dict(want_q=False, want_compact=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 2, 1, 0>"),
    "flex": dict(steps=12, train=dict(want_q=True, stride=10, keep_off=45, keep_len=10), kernel="vaeq::dp_wave_kernel<25, 8, 100, false, 1, 1, 0>"),
}
STATE = ("W", "h", "mW", "vW", "mh", "vh", "step")
OUTPUTS = ("loss", "var_est", "y", "q", "eq", "dec")


def make_rx(name):
    """The received samples of a form: seeded on the host, [R, FRAMES, 2 polarisations, I / Q, S] float32."""
    c = CASES[name]
    stride = c["train"].get("stride", B)
    S = ((c["steps"] - 1) * stride + B) * SPS
    rng = np.random.default_rng(18 + sorted(CASES).index(name))
    return (0.4 * rng.standard_normal((R, FRAMES, 2, 2, S))).astype(np.float32)


def rx_digest(rx):
    return hashlib.sha256(np.ascontiguousarray(rx).tobytes()).hexdigest()


def run_case(name, rx):
    """One launch of the form on cuda:0 from the Dirac initialisation -> ({array name: numpy array}, kernel name)."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import DPEngine

    c = CASES[name]
    amp = (np.arange(-7, 8, 2) / np.sqrt(42.0)).astype(np.float32)
    P = np.stack([np.full(8, 1 / 8), np.exp(-0.8 * amp.astype(np.float64) ** 2), np.exp(-2.0 * amp.astype(np.float64) ** 2)])
    P = (P / P.sum(axis=1, keepdims=True)).astype(np.float32)
    var = np.array([[0.0025, 0.0025], [0.004, 0.0015], [0.01, 0.02]], np.float32)
    nu_sc = np.array([0.0, 0.8, 2.0], np.float32)
    eng = DPEngine(R, M, amp, P, var, nu_sc, "cuda:0", SPS)
    out = eng.train(torch.from_numpy(rx).cuda(), B, c["steps"], np.array([2.5e-3, 1e-3, 5e-3], np.float32),
                    lr_h=np.array([2.5e-3, 2e-3, 1e-3], np.float32), **c["train"])
    torch.cuda.synchronize()
    kernel = nat.last_kernel()
    got = {k: getattr(eng, k).cpu().numpy() for k in STATE}
    got.update({k: out[k].cpu().numpy() for k in OUTPUTS if out.get(k) is not None})
    return got, kernel


@pytest.fixture(scope="module")
def recorded():
    return load_golden(FIXTURE)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dp_wave_b100_bits(name, recorded):
    rx = make_rx(name)
    assert rx_digest(rx) == str(recorded[name + "/rx_sha256"]), "the seeded input is not the one the fixture was recorded with"
    got, kernel = run_case(name, rx)
    assert kernel == CASES[name]["kernel"]
    want = {k[len(name) + 1:]: v for k, v in recorded.items() if k.startswith(name + "/") and k != name + "/rx_sha256"}
    assert set(got) == set(want) and {"loss", "var_est", "y"} | set(STATE) <= set(want)
    assert ("q" in want) == CASES[name]["train"]["want_q"]
    assert int(got["step"][0]) == FRAMES * CASES[name]["steps"] and np.isfinite(got["loss"]).all()
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), "%s/%s: %d of %d elements differ" % (name, k, int(np.sum(got[k] != want[k])), want[k].size)

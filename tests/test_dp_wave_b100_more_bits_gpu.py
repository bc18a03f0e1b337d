"""More pinned bits of the baked B = 100 DP wave kernel: the instantiations and launch modes that tests/test_dp_wave_bits_gpu.py does not reach.
Every array must equal, bit for bit, what the kernel computed when `tests/golden/G21_dp_wave_b100_more_bits.npz` was recorded
(tools/capture_dp_wave_more_bits.py, on an MI355X, with the library of the commit named in the fixture's `parent_commit`: the one before the
D phase was re-mapped to three tau per lane).

Forms (R = 5 runs with distinct P / var / nu_sc / lr, B = 100, M = 25, 2 samples per symbol, 2 frames x 3 steps from the Dirac start: the first step,
later steps with every tap non-zero, and a frame boundary):
  qam4        4-QAM, q and y written                                -> vaeq::dp_wave_kernel<25, 2, 100, true, 1, 1, 0>
  qam16       16-QAM, q and y written                               -> vaeq::dp_wave_kernel<25, 4, 100, true, 1, 1, 0>
  qam16_flex  16-QAM VAEflex: stride 10, keep_off 45, keep_len 10   -> vaeq::dp_wave_kernel<25, 4, 100, false, 1, 1, 0>
  qam64_grads 64-QAM, debug_grads: the last step's gW, gh           -> vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>
  qam64_noupd 64-QAM, no_update: taps and Adam state stay put       -> vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>
q is compared (and stored) on every Q_STRIDE-th column, which keeps the fixture below the size of G18; every other array whole.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G21_dp_wave_b100_more_bits"
R, B, M, SPS, FRAMES, STEPS = 5, 100, 25, 2, 2, 3
Q_STRIDE = 4
FLEX = dict(stride=10, keep_off=45, keep_len=10)
CASES = {
    "qam4": dict(levels=2, train=dict(want_q=True), kernel="vaeq::dp_wave_kernel<25, 2, 100, true, 1, 1, 0>"),
    "qam16": dict(levels=4, train=dict(want_q=True), kernel="vaeq::dp_wave_kernel<25, 4, 100, true, 1, 1, 0>"),
    "qam16_flex": dict(levels=4, train=dict(want_q=True, **FLEX), kernel="vaeq::dp_wave_kernel<25, 4, 100, false, 1, 1, 0>"),
    "qam64_grads": dict(levels=8, train=dict(want_q=False, debug_grads=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
    "qam64_noupd": dict(levels=8, train=dict(want_q=False, no_update=True), kernel="vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>"),
}
STATE = ("W", "h", "mW", "vW", "mh", "vh", "step")
OUTPUTS = ("loss", "var_est", "y", "q", "gW", "gh")


def make_rx(name):
    """The received samples of a form: seeded on the host, [R, FRAMES, 2 polarisations, I / Q, S] float32."""
    stride = CASES[name]["train"].get("stride", B)
    S = ((STEPS - 1) * stride + B) * SPS
    rng = np.random.default_rng(21 + sorted(CASES).index(name))
    return (0.4 * rng.standard_normal((R, FRAMES, 2, 2, S))).astype(np.float32)


def rx_digest(rx):
    return hashlib.sha256(np.ascontiguousarray(rx).tobytes()).hexdigest()


def run_case(name, rx):
    """One launch of the form on cuda:0 from the Dirac initialisation -> ({array name: numpy array}, kernel name)."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import DPEngine

    c = CASES[name]
    n = c["levels"]
    amp = np.arange(-(n - 1), n, 2).astype(np.float64)
    amp = (amp / np.sqrt(2.0 * np.mean(amp ** 2))).astype(np.float32)          # unit-power square QAM: 1/sqrt(2), 1/sqrt(10), 1/sqrt(42)
    shaping = np.array([0.0, 0.3, 0.8, 1.4, 2.0])
    P = np.exp(-shaping[:, None] * amp.astype(np.float64)[None, :] ** 2)
    P = (P / P.sum(axis=1, keepdims=True)).astype(np.float32)
    var = np.array([[0.0025, 0.0025], [0.004, 0.0015], [0.01, 0.02], [0.006, 0.006], [0.0012, 0.03]], np.float32)
    eng = DPEngine(R, M, amp, P, var, shaping.astype(np.float32), "cuda:0", SPS)
    out = eng.train(torch.from_numpy(rx).cuda(), B, STEPS, np.array([2.5e-3, 1e-3, 5e-3, 2e-3, 4e-3], np.float32),
                    lr_h=np.array([2.5e-3, 2e-3, 1e-3, 4e-3, 3e-3], np.float32), **c["train"])
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
def test_dp_wave_b100_more_bits(name, recorded):
    rx = make_rx(name)
    assert rx_digest(rx) == str(recorded[name + "/rx_sha256"]), "the seeded input is not the one the fixture was recorded with"
    got, kernel = run_case(name, rx)
    assert kernel == CASES[name]["kernel"]
    want = {k[len(name) + 1:]: v for k, v in recorded.items() if k.startswith(name + "/") and k != name + "/rx_sha256"}
    t = CASES[name]["train"]
    assert set(got) == set(want) and {"loss", "var_est", "y"} | set(STATE) <= set(want)
    assert ("q" in want) == t["want_q"] and ("gW" in want) == ("gh" in want) == bool(t.get("debug_grads"))
    assert int(got["step"][0]) == (0 if t.get("no_update") else FRAMES * STEPS) and np.isfinite(got["loss"]).all()
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), "%s/%s: %d of %d elements differ" % (name, k, int(np.sum(got[k] != want[k])), want[k].size)

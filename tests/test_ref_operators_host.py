"""Pins the float64 operator restatement (tests/_ref_operators.py) on the CPU, independently of the kernels:
  - against the values and gradients captured from the reference itself (G1 / G4 / G8), with the bounds the GPU tests use;
  - against the float64 C oracle at shapes the goldens do not have (sps 1 / 3 / 4, M 1 / 3 / 63, B at its minimum, n_lev 2 / 4 / 8).
The GPU envelope tests (test_operator_envelope_gpu.py) then measure the HIP operator kernels against this restatement."""
import numpy as np
import pytest
import torch

import _ref_operators as ref
import oracle
from conftest import load_golden, relerr

G1 = ["G1_dp_step_64qam_pcs", "G1_dp_step_64qam", "G1_dp_step_16qam", "G1_dp_step_4qam", "G1_dp_step_64qam_nu0872", "G1_dp_step_64qam_nu1222"]
G4 = ["G4_awgn_16qam_cfg1", "G4_awgn_64qam_pcs_free10", "G4_awgn_4qam_small"]
G8 = ["G8_vaenn_64qam", "G8_vaenn_16qam_small", "G8_vaenn_4qam_k5"]


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def _np(t):
    return t.detach().numpy()


def _dp_step(x, W, h, amp, P, var, nu_sc, sps):
    Wt, ht = _t(W, True), _t(h, True)
    q, out = ref.dp_forward(_t(x), Wt, _t(amp), _t(var), float(nu_sc), sps)
    loss, ve = ref.dp_loss(q, _t(x), ht, _t(amp), _t(P))
    gW, gh = torch.autograd.grad(loss, (Wt, ht))
    return dict(q=_np(q), out=_np(out), loss=float(loss.detach()), var_est=_np(ve), gW=_np(gW), gh=_np(gh))


def _awgn_step(x, W, h, amp, P, amp_mean, var, sps):
    Wt, ht = _t(W, True), _t(h, True)
    q, out = ref.awgn_forward(_t(x), Wt, _t(amp), float(amp_mean), float(var), sps)
    loss = ref.awgn_loss(q, _t(x), ht, _t(amp), None if P is None else _t(P))
    gW, gh = torch.autograd.grad(loss, (Wt, ht))
    return dict(q=_np(q), out=_np(out), loss=float(loss.detach()), gW=_np(gW), gh=_np(gh))


def _nn_step(x, theta, amp, k1, k2, M, sps):
    th = _t(theta, True)
    q, h = ref.vaenn_net(_t(x), th, len(amp), k1, k2, sps, M)
    loss = ref.awgn_loss(q, _t(x), h, _t(amp), None)
    (g,) = torch.autograd.grad(loss, (th,))
    return dict(q=_np(q), loss=float(loss.detach()), g=_np(g))


@pytest.mark.parametrize("name", G1)
def test_dp_restatement_matches_reference_capture(name):
    g = load_golden(name)
    B, sps = int(g["B"]), int(g["sps"])
    x = g["rx"][:, :, :B * sps]
    r = _dp_step(x, g["W0"], g["h0"], g["amp_levels"], g["P"], g["var"], g["nu_sc"], sps)
    assert relerr(r["out"], g["out0"]) < 2e-6
    assert np.max(np.abs(r["q"] - g["q0"])) < 2e-4
    assert abs(r["loss"] - g["loss0"]) / abs(g["loss0"]) < 1e-5
    assert relerr(r["var_est"], g["var_est0"]) < 1e-5
    assert relerr(r["gh"], g["gh0"]) < 2e-5
    # config 5's heaviest shaping (var 1.5e-4, logits ~1e4): the reference's own fp32 gradient sits 1.1e-4 of its max from the f64
    # truth, the same allowance test_oracle_golden gives the f64 oracle; the restatement meets that truth to 1e-9 below
    assert relerr(r["gW"], g["gW0"]) < (2e-4 if name.endswith("nu1222") else 1e-4)
    loss, ve = ref.dp_loss(_t(g["q0"]), _t(x), _t(g["h0"]), _t(g["amp_levels"]), _t(g["P"]))
    assert abs(float(loss) - g["loss0"]) / abs(g["loss0"]) < 1e-5 and relerr(_np(ve), g["var_est0"]) < 1e-5
    q = ref.soft_dec(_t(g["out0"]), _t(g["var"]), _t(g["amp_levels"]), float(g["nu_sc"]))
    assert np.max(np.abs(_np(q) - g["q0"])) < 2e-4


@pytest.mark.parametrize("name", G4)
def test_awgn_restatement_matches_reference_capture(name):
    g = load_golden(name)
    B, sps = int(g["B"]), int(g["sps"])
    x = g["rx"][:, :B * sps]
    r = _awgn_step(x, g["W0"], g["h0"], g["amp_levels"], g["P"], g["amp_mean"], g["var"], sps)
    assert relerr(r["out"], g["out0"]) < 2e-6
    assert np.max(np.abs(r["q"] - g["q0"])) < 5e-4
    assert abs(r["loss"] - g["loss"][0]) / abs(g["loss"][0]) < 1e-5
    assert relerr(r["gh"], g["gh0"]) < 2e-5
    assert relerr(r["gW"], g["gW0"]) < 1e-4


@pytest.mark.parametrize("name", G8)
def test_vaenn_loss_restatement_matches_reference_capture(name):
    g = load_golden(name)
    B, sps, k1, k2, M = int(g["B"]), int(g["sps"]), int(g["k1"]), int(g["k2"]), int(g["M_est"])
    x = g["rx"][:, :B * sps]
    r = _nn_step(x, g["theta0"], g["amp_levels"], k1, k2, M, sps)
    assert np.max(np.abs(r["q"] - g["q0"])) < 5e-6
    assert abs(r["loss"] - g["loss"][0]) / abs(g["loss"][0]) < 1e-5
    o = np.cumsum([0, 2 * len(g["amp_levels"]) * 2 * k1, 2 * len(g["amp_levels"]), (2 * len(g["amp_levels"])) ** 2 * k2,
                   2 * len(g["amp_levels"]), 2 * M])
    for a, b in zip(o[:-1], o[1:]):
        assert relerr(r["g"][a:b], g["g0"][a:b]) < 2e-4, (a, b)


# (sps, M, B, n_lev): every shape minimal (B = M, the smallest B the loss accepts) except where noted
OFF_GOLDEN = [(1, 1, 1, 2), (3, 1, 1, 8), (4, 3, 3, 4), (1, 3, 3, 8), (3, 63, 63, 2), (4, 63, 63, 8), (1, 63, 63, 4), (3, 3, 17, 4),
              (4, 1, 5, 2)]
CASES = [(sps, M, B, n, k) for k, (sps, M, B, n) in enumerate(OFF_GOLDEN)]


def _levels(n):
    return (np.arange(-(n - 1), n, 2) / np.sqrt((n * n - 1) / 3.0 * 2)).astype(np.float64)


def _prior(rng, n):
    p = rng.uniform(0.2, 1.0, n)
    p = (p + p[::-1]) / 2
    return p / p.sum()


@pytest.mark.parametrize("sps,M,B,n,seed", CASES)
def test_dp_restatement_matches_f64_oracle(sps, M, B, n, seed):
    rng = np.random.default_rng(100 + seed)
    x = 0.5 * rng.standard_normal((2, 2, B * sps))
    W = 0.3 * rng.standard_normal((2, 4, M)) / np.sqrt(M)
    W[0, 0, M // 2] += 1.0
    W[1, 1, M // 2] += 1.0
    h = 0.3 * rng.standard_normal((2, 2, 2, M))
    amp, P, var, nu = _levels(n), _prior(rng, n), rng.uniform(0.01, 0.05, 2), float(rng.uniform(0, 1))
    o = oracle.dp_step_grads(x, W, h, amp, P, var, nu, sps, np.float64)
    r = _dp_step(x, W, h, amp, P, var, nu, sps)
    for k in ("out", "q", "var_est", "gW", "gh"):
        assert relerr(r[k], o[k]) < 1e-9, k
    assert abs(r["loss"] - o["loss"]) / abs(o["loss"]) < 1e-9


@pytest.mark.parametrize("sps,M,B,n,seed", CASES)
def test_awgn_restatement_matches_f64_oracle(sps, M, B, n, seed):
    rng = np.random.default_rng(200 + seed)
    x = 0.5 * rng.standard_normal((2, B * sps))
    W = 0.3 * rng.standard_normal((1, 2, M)) / np.sqrt(M)
    W[0, 0, M // 2] += 1.0
    h = 0.3 * rng.standard_normal((2, M))
    amp, P = _levels(n), _prior(rng, n)
    amp_mean, var = float(np.mean(np.abs(amp))), float(rng.uniform(0.02, 0.1))
    o = oracle.awgn_step_grads(x, W, h, amp, P, amp_mean, var, sps, np.float64)
    r = _awgn_step(x, W, h, amp, P, amp_mean, var, sps)
    for k in ("out", "q", "gW", "gh"):
        assert relerr(r[k], o[k]) < 1e-9, k
    assert abs(r["loss"] - o["loss"]) / abs(o["loss"]) < 1e-9


@pytest.mark.parametrize("sps,M,B,n,seed", CASES)
def test_vaenn_restatement_matches_f64_oracle(sps, M, B, n, seed):
    rng = np.random.default_rng(300 + seed)
    k1, k2 = (3, 5) if seed % 2 else (5, 3)
    x = 0.5 * rng.standard_normal((2, B * sps))
    theta = 0.3 * rng.standard_normal(oracle.nn_param_count(n, k1, k2, M))
    amp = _levels(n)
    o = oracle.nn_step_grads(x, theta, amp, k1, k2, M, sps, np.float64)
    r = _nn_step(x, theta, amp, k1, k2, M, sps)
    assert relerr(r["q"], o["q"]) < 1e-9
    assert abs(r["loss"] - o["loss"]) / abs(o["loss"]) < 1e-9
    assert relerr(r["g"], o["g"]) < 1e-9


def test_heavy_shaping_gradient_matches_f64_oracle():
    """The one golden where the restatement needs the wider gW bound above: there it equals the f64 oracle to 1e-9."""
    g = load_golden("G1_dp_step_64qam_nu1222")
    B, sps = int(g["B"]), int(g["sps"])
    x = g["rx"][:, :, :B * sps]
    o = oracle.dp_step_grads(x, g["W0"], g["h0"], g["amp_levels"], g["P"], g["var"], float(g["nu_sc"]), sps, np.float64)
    r = _dp_step(x, g["W0"], g["h0"], g["amp_levels"], g["P"], g["var"], g["nu_sc"], sps)
    assert relerr(r["gW"], o["gW"]) < 1e-9 and relerr(r["gh"], o["gh"]) < 1e-9


def test_ragged_length_gives_ceil_outputs():
    """Conv1d(padding=M//2, stride=sps) of L samples has ceil(L/sps) outputs; zero-padding x to that many whole symbols changes none."""
    rng = np.random.default_rng(7)
    x, W = _t(rng.standard_normal((2, 2, 201))), _t(rng.standard_normal((2, 4, 9)))
    y = ref.dp_fir(x, W, 2)
    assert y.shape[-1] == 101
    assert torch.equal(y, ref.dp_fir(torch.nn.functional.pad(x, (0, 1)), W, 2))
    xa, Wa = _t(rng.standard_normal((2, 301))), _t(rng.standard_normal((1, 2, 9)))
    ya = ref.awgn_fir(xa, Wa, 4)
    assert ya.shape[-1] == 76 and torch.equal(ya, ref.awgn_fir(torch.nn.functional.pad(xa, (0, 3)), Wa, 4))

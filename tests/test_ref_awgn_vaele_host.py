"""The float64 model of the AWGN VAE-LE training loop (tests/_ref_awgn_vaele.py) pinned on the CPU: against the reference's G4 captures with the
bounds tests/test_awgn_kernel_gpu.py holds the kernel to, its hand-written AMSGrad against torch.optim.Adam, the whole loop against the C oracle in
float64 at shapes the goldens lack, and the conditioning of every envelope case that tests/test_awgn_vaele_envelope_gpu.py compares kernels on."""
import numpy as np
import pytest
import torch

import _ref_awgn_vaele as rv
import oracle
from conftest import load_golden, relerr

AWGN = ["G4_awgn_16qam_cfg1", "G4_awgn_64qam_pcs_free10", "G4_awgn_4qam_small"]


def _train_golden(g, steps):
    return rv.train(g["rx"], g["W0"], g["h0"], None, steps, int(g["B"]), g["amp_levels"], g["P"], float(g["amp_mean"]), float(g["var"]), float(g["lr"]),
                    int(g["sps"]))


@pytest.mark.parametrize("name", AWGN)
def test_model_against_g4_teacher_forced_step(name):
    """The bounds of test_awgn_teacher_forced_step, entry for entry: y, q, loss, both gradients, the taps after one AMSGrad step with the same
    exclusion of the entries whose golden gradient is rounding noise (the scale direction of the Dirac start: +-lr on a coin flip)."""
    g = load_golden(name)
    B, lr = int(g["B"]), float(g["lr"])
    r = _train_golden(g, 1)
    assert relerr(r["y"], g["out0"]) < 2e-6
    assert np.max(np.abs(r["q"] - g["q0"])) < 5e-4
    assert abs(r["loss"][0] - g["loss"][0]) / abs(g["loss"][0]) < 1e-5
    assert relerr(r["gh"][0], g["gh0"]) < 2e-5
    assert relerr(r["gW"][0], g["gW0"].reshape(2, -1)) < 1e-4
    ok = np.abs(g["gW0"].reshape(2, -1)) > 1e-6 * np.abs(g["gW0"]).max()
    assert np.max(np.abs(r["W"] - g["W1"].reshape(2, -1))[ok]) < 1e-5
    assert np.max(np.abs(r["W"] - g["W1"].reshape(2, -1))) < 2.01 * lr
    assert np.max(np.abs(r["h"] - g["h1"])) < 1e-5
    assert r["step"] == 1 and r["y"].shape == (2, B) and r["q"].shape == g["q0"].shape


@pytest.mark.parametrize("name", AWGN)
def test_model_against_g4_free_run(name):
    """The bounds of test_awgn_freerun_perturbed_start (non-Dirac start: losses, taps, AMSGrad maxima) and, from the Dirac start, of
    test_awgn_freerun_dirac_within_coinflip (the trajectory is pinned up to the coin flip of the scale tap)."""
    g = load_golden(name)
    ns, lr = int(g["n_steps"]), float(g["lr"])
    r = _train_golden(g, ns)
    dl = np.max(np.abs(r["loss"] - g["loss"]) / np.abs(g["loss"]))
    dW, dh = np.max(np.abs(r["W"] - g[f"W{ns}"].reshape(2, -1))), np.max(np.abs(r["h"] - g[f"h{ns}"]))
    if np.count_nonzero(g["W0"]) == 1:
        assert dl < 2e-3 and dW < 2.5 * lr and dh < 2.5 * lr
    else:
        assert dl < 2e-5 and dW < 2e-5 and dh < 2e-5
        assert relerr(r["xW"], g["vmaxW"].reshape(2, -1)) < 1e-4 and relerr(r["xh"], g["vmaxh"]) < 1e-4
    assert r["step"] == ns


def test_hand_written_amsgrad_equals_torch_adam():
    """Eight steps on the same float64 gradients, gradients that shrink so that the maximum binds: parameters, both moments and the maximum
    agree with torch.optim.Adam(amsgrad=True) to 1e-12 relative."""
    rng = np.random.default_rng(8)
    p0 = rng.standard_normal((2, 25))
    grads = [rng.standard_normal((2, 25)) * (3.0 if s < 3 else 0.2) for s in range(8)]
    tp = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, amsgrad=True)
    p, m, v, x = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0)
    for s, g in enumerate(grads):
        tp.grad = torch.tensor(g.copy())
        opt.step()
        rv.amsgrad_step(p, g, m, v, x, s + 1, 3e-3)
        st = opt.state[tp]
        assert relerr(p, tp.detach().numpy()) <= 1e-12
        assert relerr(m, st["exp_avg"].numpy()) <= 1e-12 and relerr(v, st["exp_avg_sq"].numpy()) <= 1e-12
        assert relerr(x, st["max_exp_avg_sq"].numpy()) <= 1e-12
    assert np.any(x > v)                                                      # the maximum did bind


ORACLE_SHAPES = [  # B, sps, M, n_lev: sps 1 and 3, M 9 and 63, B at its minimum 2 (M / 2) + 1, every level count
    (9, 1, 9, 2), (9, 3, 9, 4), (63, 1, 63, 8), (63, 3, 63, 2), (40, 1, 9, 8), (70, 3, 63, 4), (9, 2, 9, 8),
]


@pytest.mark.parametrize("B,sps,M,n", ORACLE_SHAPES)
def test_model_against_the_c_oracle_in_float64(B, sps, M, n):
    """Two independent float64 derivations (autograd here, the closed-form backward of the C oracle) over 4 steps: losses and taps to 1e-9."""
    case = dict(seed=B * 1000 + sps * 100 + M + n, R=1, steps=4, B=B, M=M, n_lev=n, sps=sps, edge=None)
    d = rv.build(case)
    r = rv.train(d["rx"][0], d["W0"][0], d["h0"][0], None, 4, B, d["amp"], d["P"][0], d["amp_mean"][0], d["var"][0], d["lr"][0], sps)
    st = oracle.AWGNState(M, np.float64, d["W0"][0], d["h0"][0])
    loss = oracle.awgn_train(st, d["rx"][0], 4, B, d["amp"], d["P"][0], float(d["amp_mean"][0]), float(d["var"][0]), float(d["lr"][0]), sps, np.float64)
    assert np.max(np.abs(r["loss"] - loss) / np.abs(loss)) <= 1e-9
    assert relerr(r["W"], st.W[0]) <= 1e-9 and relerr(r["h"], st.h) <= 1e-9
    assert relerr(r["xW"], st.vmaxW[0]) <= 1e-9 and relerr(r["xh"], st.vmaxh) <= 1e-9
    assert st.step.value == r["step"] == 4


def test_adam_travel_bound():
    """The factor the issue of a coin-flip entry is held to: 1 at the first step, 1.08 at the fourth from a fresh state, 10 for an old run."""
    assert rv.adam_travel_bound(0.9, 0.999, 0, 1) == pytest.approx(1.0, abs=1e-12)
    per_step = [rv.adam_travel_bound(0.9, 0.999, t - 1, t) for t in range(1, 5)]
    assert per_step == sorted(per_step) and 1.07 < per_step[3] < 1.08
    assert rv.adam_travel_bound(0.9, 0.999, 0, 4) == pytest.approx(sum(per_step))
    assert 9.9 < rv.adam_travel_bound(0.9, 0.999, 3999, 4000) < 10.0
    # and it is a bound: the worst single-entry history (one large gradient after small ones) stays inside it
    p, m, v, x = np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    for t, g in enumerate([1e-3, 1e-3, 1e-3, 1.0]):
        before = p.copy()
        rv.amsgrad_step(p, np.array([g]), m, v, x, t + 1, 1.0)
        assert abs(p - before)[0] <= rv.adam_travel_bound(0.9, 0.999, t, t + 1)


CASES = rv.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_case_is_conditioned(case):
    """For every run and both tap groups the model alone leaves at least two thirds of the entries conditioned (gradient >= 1e-2 of the group's
    largest at every step); the model's run is finite and its taps move."""
    data, runs = rv.model(case)
    assert len(runs) == case["R"] == 3 and case["steps"] == 4
    assert len({float(v) for v in data["var"]}) == (1 if case["edge"] == "steep" else 3) and len({float(v) for v in data["lr"]}) == 3
    for r, m in enumerate(runs):
        assert np.all(np.isfinite(m["loss"])) and np.all(np.isfinite(m["W"])) and np.all(np.isfinite(m["h"])), (case["id"], r)
        for grp in ("gW", "gh"):
            frac = rv.conditioned(m[grp]).mean()
            assert frac >= 2 / 3, (case["id"], r, grp, frac)
        assert np.abs(m["W"] - data["W0"][r]).max() > 0.1 * data["lr"][r]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_case_is_float32_conditioned(case):
    """The float32 evaluation of the model stays within GAP_LIMIT (a quarter of the suite's ceilings) of the float64 model in every quantity the
    case is compared on: what a kernel is held to there is not rounding noise amplified by the loop itself."""
    data, runs = rv.model(case)
    gap = rv.float32_gap(case, data, runs)
    over = {k: (gap[k], rv.GAP_LIMIT[k]) for k in rv.held(case) if not gap[k] <= rv.GAP_LIMIT[k]}
    assert not over, (case["id"], over)
    assert set(rv.held(case)) == set(rv.GAP_LIMIT) or case["edge"] == "steep"


def test_the_steep_demapper_takes_float32_past_the_moment_ceiling():
    """Why the moments of the var = 1e-3 cases have no 1e-4 ceiling in tests/test_awgn_vaele_envelope_gpu.py: after their 4 steps the float32
    evaluation of the model is itself further than that from the float64 model (4 GAP_LIMIT = the ceiling) in the moments of the multi-wave
    and the generic steep case, while every quantity held() keeps for them stays within GAP_LIMIT (test_every_case_is_float32_conditioned).
    Should this stop being true, the exemption goes."""
    steep = [c for c in CASES if c["edge"] == "steep"]
    assert len(steep) == 3
    over = {}
    for c in steep:
        gap = rv.float32_gap(c, *rv.model(c))
        over[c["id"]] = max(gap[k] / (4 * rv.GAP_LIMIT[k]) for k in ("m", "v", "x"))
        assert set(rv.GAP_LIMIT) - set(rv.held(c)) == {"m", "v", "x", "q", "gW", "gh"}
    assert over["edge-steep-wave-B386"] > 1 and over["edge-steep-generic-B41"] > 1, over
    for c in CASES:
        if c["edge"] != "steep":
            assert set(rv.held(c)) == set(rv.GAP_LIMIT)


def test_lds_ceiling_is_the_one_the_library_names():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "vae_equalizer_amd", "csrc", "vaeq_launch.h")).read()
    m = re.search(r"constexpr size_t LDS_MAX = (\d+) \* 1024;", text)
    assert m and int(m.group(1)) * 1024 == rv.LDS_MAX


def test_case_list_covers_the_envelope():
    wave = rv.cases("wave")
    grid = [c for c in wave if c["edge"] is None]
    classes = {}
    for c in grid:
        k = c["kernel"].split("<")[1].rstrip(">").split(", ")
        classes.setdefault((int(k[2]), int(k[3])), []).append(c)
    assert set(classes) == {(1, 1), (2, 1), (3, 1), (2, 2), (2, 3), (2, 4)}
    for cl, cs in classes.items():
        assert {c["M"] for c in cs} == {9, 17, 25} and {c["n_lev"] for c in cs} == {2, 4, 8}, cl
    Bs = {c["B"] for c in grid}
    assert {10, 18, 26, 126, 128, 130, 254, 256, 258, 382, 384, 386, 510, 512, 514, 766, 768, 770, 1022, 1024, 348, 350, 352} <= Bs
    assert {c["B"] % 4 for c in grid} == {0, 2}
    assert {c["n_lev"] for c in grid if c["kernel"].endswith(", 3, 1, 350>")} == {2, 4, 8}
    assert rv.case_by_id("wave-B350-M17-n8")["kernel"] == "vaeq::awgn_wave_kernel<17, 8, 3, 1, 0>"
    gen = [c for c in rv.cases("generic") if c["edge"] is None]
    assert {c["threads"] for c in gen} == {64, 128, 256} and {c["sps"] for c in gen} == {1, 2, 3, 4}
    assert {1, 3, 13, 31, 63} <= {c["M"] for c in gen} and {41, 351} <= {c["B"] for c in gen}
    assert {(c["sps"], c["M"]) for c in gen if c["B"] == 2 * (c["M"] // 2) + 1} >= {(1, 13), (3, 31), (4, 3), (2, 63), (1, 3)}
    Bmax = rv.largest_generic_B(2, 25)
    assert rv.generic_lds_bytes(Bmax, 2, 25) <= rv.LDS_MAX < rv.generic_lds_bytes(Bmax + 1, 2, 25)


def test_a_minibatch_of_exact_zeros_has_no_finite_model_value():
    """Why that edge is not among the cases: mean |y| = 0 makes the normalised output 0 / 0."""
    case = rv.case_by_id("wave-B10-M9-n4")
    d = rv.build(case)
    x = np.zeros((2, 20), np.float32)
    loss, y, q, gW, gh = rv.step_grads(x, d["W0"][0].astype(np.float64), d["h0"][0].astype(np.float64), d["amp"], d["P"][0], d["amp_mean"][0],
                                       d["var"][0], 2)
    assert np.all(y == 0) and not np.isfinite(loss)

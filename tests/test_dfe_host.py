"""CPU-side checks of the known-channel LMMSE / DFE baselines (AWGN_channel/DFE_MQAM_shaping.py): the call surface and constants, a
side-effect-free import, the host filter design, the seeded host generator and the torch mirrors against the reference's own outputs
(G16), and the host-side shape refusals of vaeq_awgn_lmmse_eval / vaeq_awgn_dfe."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

CASES = ["G16_dfe_64qam_h1_15dB", "G16_dfe_64qam_h1_22dB", "G16_dfe_16qam_h2_18dB", "G16_dfe_4qam_proakis_a_8dB"]


def relerr(a, b):
    """max |a-b| / max |b| for complex arrays."""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _mod():
    from vae_equalizer_amd import DFE_MQAM_shaping as d
    return d


def _consts(g):
    d = _mod()
    q = d.qam_constants(str(g["mod"]))
    return q, torch.tensor(g["h_channel"], dtype=torch.cfloat)


def test_call_surface_and_constants_match_reference():
    d = _mod()
    pos = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos(d.rcfir) == ["T", "sps", "beta"] and pos(d.rrcfir) == ["T", "sps", "beta"]
    assert pos(d.generate_data_shaping) == ["N", "amp_levels", "SNR", "h_channel", "nu"]
    assert pos(d.SER_func)[:2] == ["rx", "tx"]
    assert pos(d.find_shift_symb) == ["rx", "tx", "N_shift"]
    assert pos(d.compute_lmmse) == ["channel", "SNR", "order", "n1"]
    assert pos(d.compute_feedforward) == ["channel", "SNR", "order"]
    assert pos(d.compute_feedback_filter) == ["channel", "feedforward"]
    assert pos(d.dfe)[:4] == ["feedforward_output", "feedforward_filter", "feedback_filter", "init_decisions_idxs"]
    assert pos(d.nearest_neighbor)[:1] == ["rx_syms"] and pos(d.compl_conv) == ["rx", "h"]
    assert d.mod == '64-QAM' and d.sps == 1 and d.M == 5
    assert np.array_equal(d.SNR_vec, np.arange(15, 23)) and d.nu == 0.0270955
    assert (d.N_valid, d.N_cut, d.lmmse_filter_order, d.M_dfe, d.num_epochs, d.n1) == (128000, 20, 20, 11, 5, 10)
    assert d.base_seed is None and d.generator is None
    g = load_golden(CASES[0])
    np.testing.assert_allclose(d.h_channel, g["h_channel"], rtol=1e-6)
    np.testing.assert_array_equal(d.amp_levels.numpy(), g["amp_levels"])
    c = d.const_torch.numpy()
    assert c[1].real == c[0].real and c[8].real > c[0].real                # I-major: index = iI * n + iQ


def test_import_runs_no_sweep():
    code = "import time; t = time.time(); import vae_equalizer_amd.DFE_MQAM_shaping as d; print(time.time() - t)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines() == [r.stdout.strip().splitlines()[-1]]   # nothing printed but the timing
    assert float(r.stdout.strip()) < 30


@pytest.mark.parametrize("case", CASES)
def test_filters_match_reference(case):
    d, g = _mod(), load_golden(case)
    _, h = _consts(g)
    SNR = g["SNR"].item()
    lm = d.compute_lmmse(h, SNR, d.lmmse_filter_order, d.lmmse_filter_order // 2 + 1).numpy()
    ff = d.compute_feedforward(h, SNR, d.M_dfe)
    fb = d.compute_feedback_filter(h, ff).numpy()
    assert relerr(lm, g["lmmse"]) <= 1e-5 and relerr(ff.numpy(), g["ff"]) <= 1e-5 and relerr(fb, g["fb"]) <= 1e-5
    assert fb.shape == (len(g["h_channel"]) - 1,)


@pytest.mark.parametrize("case", CASES)
def test_seeded_host_generator_reproduces_reference(case):
    from vae_equalizer_amd import channel as ch
    d, g = _mod(), load_golden(case)
    st = ch.SeededStreams(int(g["seed"]))
    rx, data, P = d.generate_data_shaping(int(g["N"]), g["amp_levels"], np.int64(g["SNR"]), g["h_channel"], float(g["nu"]),
                                          rng=st.next_rng(), noise=st.noise)
    np.testing.assert_array_equal(data.numpy(), g["data"])
    np.testing.assert_array_equal(P.numpy(), g["P"])
    np.testing.assert_array_equal(rx.numpy(), g["rx"])


@pytest.mark.parametrize("case", CASES)
def test_torch_mirrors_reproduce_reference(case):
    d, g = _mod(), load_golden(case)
    q, _ = _consts(g)
    nc = int(g["N_cut"])
    rx = torch.from_numpy(g["rx"])
    data = torch.from_numpy(g["data"])
    rxc = torch.complex(rx[0], rx[1])
    out = d.compl_conv(rxc, torch.from_numpy(g["lmmse"]))
    assert out.shape[-1] == rx.shape[-1] + 1 and relerr(out.numpy(), g["lmmse_out"]) <= 1e-5
    out = torch.from_numpy(g["lmmse_out"])
    idx = d.nearest_neighbor(out[1:], q["const_torch"]).numpy()
    np.testing.assert_array_equal(idx, g["lmmse_dec"])
    sh = int(d.find_shift_symb(torch.view_as_real(out).T, data, 21))
    assert sh == int(g["lmmse_shift"])
    ser = d.SER_func(torch.view_as_real(out).T[:, nc + 11 + sh:-11 - nc].clone(), data[:, nc + 11:-11 - sh - nc], q["amp_levels"])
    assert float(ser) == pytest.approx(float(g["lmmse_SER"]), abs=1e-7)
    ffo = d.compl_conv(rxc, torch.from_numpy(g["ff"]))
    assert ffo.shape[-1] == rx.shape[-1] and relerr(ffo.numpy(), g["ff_out"]) <= 1e-5
    hard = torch.view_as_real(q["const_torch"][torch.from_numpy(g["dfe_dec"]).long()]).T
    sh = int(d.find_shift_symb(hard, data, 24))
    assert sh == int(g["dfe_shift"])
    ser = d.SER_func(hard[:, nc + 11 + sh:-11 - nc].clone(), data[:, nc + 11:-11 - sh - nc], q["amp_levels"])
    assert float(ser) == pytest.approx(float(g["dfe_SER"]), abs=1e-7)


def test_host_side_shape_refusals():
    from vae_equalizer_amd import _native as nat
    L = nat.lib()
    lm = lambda N, sps=1, n_lev=8, K=20, n_shift=21, n_cut=20: L.vaeq_awgn_lmmse_eval(1, N, sps, n_lev, K, n_shift, n_cut, *([None] * 10))
    assert lm(128000) == -1 and lm(4000) == -1                            # valid shapes reach the pointer checks (no GPU touched)
    assert lm(128000, sps=2) == -2                                        # the script implements 1 sps only
    assert lm(1000 + 21 + 40 + 22 - 1) == -2 and lm(1000 + 21 + 40 + 22) == -1   # shift window + cuts
    assert lm(4000, n_lev=3) == -2 and lm(4000, n_lev=16) == -2
    assert lm(4000, K=21) == -2 and lm(4000, K=66) == -2                  # odd / too long LMMSE filter
    assert lm(4000, n_shift=70) == -2
    assert L.vaeq_awgn_lmmse_eval(0, 4000, 1, 8, 20, 21, 20, *([None] * 10)) == 0
    assert L.vaeq_awgn_lmmse_eval_ws_bytes(3, 4000, 20) == 3 * 4001 * 8

    def dfe(N=128000, sps=1, n_lev=8, K1=11, K2=4, C=1000, W=32, evaluate=True):
        return L.vaeq_awgn_dfe(1, N, sps, n_lev, K1, K2, C, W, 24, 20, *([None] * 8), 1 if evaluate else None, *([None] * 4))
    assert dfe() == -1 and dfe(C=1) == -1 and dfe(K2=10) == -1
    assert dfe(sps=2) == -2 and dfe(n_lev=3) == -2
    assert dfe(K2=0) == -2 and dfe(K2=11) == -2                           # K2 = L <= 10 (Proakis A)
    assert dfe(C=0) == -2 and dfe(C=8193) == -2 and dfe(N=4000, C=1500) == -2   # chunks shorter than K2
    assert dfe(W=-1) == -2
    assert dfe(N=1100) == -2 and dfe(N=1100, C=4, evaluate=False) == -1   # N rule only when evaluating
    assert L.vaeq_awgn_dfe_ws_bytes(2, 4000, 10) == 2 * 4000 * 8 + 2 * 10 * 16


def test_new_module_never_imports_the_oracle_or_the_reference():
    src = open(os.path.join(ROOT, "vae_equalizer_amd", "DFE_MQAM_shaping.py")).read()
    assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M)
    assert "/root/" not in src

"""CPU-side checks of the AWGN constant-modulus baseline (AWGN_channel/func_CMA_MQAM_shaping.py, Eval_run_shaping_cma.py): the call
surface, the sweep order, the host-side shape refusals of vaeq_awgn_cma / vaeq_awgn_cma_validate, and the torch mirrors against the
reference's own CPE / find_shift_symb / SER_CMA outputs (G15)."""
import inspect
import os
import re

import numpy as np
import torch

from conftest import ROOT, load_golden


def test_processing_signature_matches_reference():
    from vae_equalizer_amd import func_CMA_MQAM_shaping as cm
    pos = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos(cm.processing) == ["mod", "sps", "SNR", "nu", "M_est", "lr_optim", "N_valid", "N_train", "num_epochs", "epe", "channel"]
    kw = {p.name: p.default for p in inspect.signature(cm.processing).parameters.values() if p.kind == p.KEYWORD_ONLY}
    assert kw == {"seed": None, "device": None, "verbose": True, "generator": None}
    assert pos(cm.CMA) == ["Rx", "R", "h", "lr", "sps", "eval"]
    assert pos(cm.find_shift_symb) == ["rx", "tx", "N_shift"]
    assert pos(cm.SER_CMA)[:5] == ["rx", "tx", "sps", "amp_levels", "num_lev"]
    assert pos(cm.generate_data)[:8] == ["N", "M", "amps", "SNR", "h_channel", "sps", "device", "P"]


def test_sweep_points_follow_the_reference_loop_nest(monkeypatch):
    from vae_equalizer_amd import Eval_run_shaping_cma as ev
    assert (ev.mod, ev.sps, ev.channel, ev.M_vec, ev.lr_optim_vec, ev.SNR_vec, ev.nu_vec) == ('64-QAM', 2, 'h1', [25], [0.5e-4], [22], [0])
    assert (ev.iter, ev.N_valid, ev.train_len, ev.num_epochs, ev.epe) == (3, 15000, 4000, 500, 2)
    monkeypatch.setattr(ev, "lr_optim_vec", [1e-4, 2e-4]); monkeypatch.setattr(ev, "M_vec", [9, 25]); monkeypatch.setattr(ev, "SNR_vec", [18, 20, 22])
    monkeypatch.setattr(ev, "nu_vec", [0, 0.1]); monkeypatch.setattr(ev, "iter", 2)
    pts = list(ev.sweep_points())
    expect = []
    for l, lr in enumerate(ev.lr_optim_vec):                   # lr -> M -> SNR -> nu -> iter
        for m, M in enumerate(ev.M_vec):
            for s, SNR in enumerate(ev.SNR_vec):
                for nu in ev.nu_vec:
                    for i in range(ev.iter):
                        expect.append(((s, 0, 0, m, l, 0, i), dict(lr=lr, M=M, SNR=SNR, nu=nu)))
    assert pts == expect
    shape = (len(ev.SNR_vec), 1, 1, len(ev.M_vec), len(ev.lr_optim_vec), 1, ev.iter)
    assert all(all(0 <= a < b for a, b in zip(idx, shape)) for idx, _ in pts)


def test_host_side_shape_refusals():
    from vae_equalizer_amd import _native as nat
    L = nat.lib()
    train = lambda R, N, sps, M: L.vaeq_awgn_cma(R, N, sps, M, 1, None, 1.0, None, None, None, None, None, None)
    assert train(1, 4000, 2, 24) == -2                         # even M
    assert train(1, 4000, 2, 65) == -2                         # more taps than a wave has lanes
    assert train(1, 4000, 0, 25) == -2 and train(1, 4000, 9, 25) == -2 and train(1, 4001, 2, 25) == -2
    assert train(1, 40, 2, 25) == -2                           # fewer symbols than taps
    assert train(1, 4000, 2, 25) == -1 and train(1, 4000, 2, 63) == -1   # valid shapes reach the pointer checks (no GPU touched)
    assert train(0, 4000, 2, 25) == 0                          # empty batch

    val = lambda N, sps=2, M=25, n_lev=4, n_shift=21: L.vaeq_awgn_cma_validate(1, N, sps, M, n_lev, n_shift, *([None] * 9))
    assert val(2 * 1020) == -2                                 # the shift search reads 1000 + n_shift symbols
    assert val(2 * 1021) == -1 and val(30000) == -1 and val(100000) == -1
    assert val(30000, M=26) == -2 and val(30000, M=65) == -2 and val(30000, sps=0) == -2 and val(30000, sps=9) == -2
    assert val(30000, n_lev=3) == -2 and val(30000, n_shift=20) == -2 and val(30000, n_shift=25) == -2
    assert L.vaeq_awgn_cma_validate_ws_bytes(3, 30000, 2) == 0                    # N_valid = 15 000: the track lives in LDS
    assert L.vaeq_awgn_cma_validate_ws_bytes(3, 100000, 2) == 3 * 2 * 50000 * 8   # N_valid = 50 000: global workspace
    assert L.vaeq_awgn_cma_validate_ws_bytes(3, 30001, 2) == -2


def test_new_modules_never_import_the_oracle_or_the_reference():
    for f in ("func_CMA_MQAM_shaping.py", "Eval_run_shaping_cma.py"):
        src = open(os.path.join(ROOT, "vae_equalizer_amd", f)).read()
        assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), f
        assert "/root/" not in src, f


def test_cpe_mirror_against_reference_cpu():
    """The torch CPE mirror on the drifting constellation: the reference's CPE does not unwrap, so its output jumps by pi/2 where the
    drift crosses +-pi/4 -- an unwrapping CPE (the DP one) would not."""
    from vae_equalizer_amd.func_CMA_MQAM_shaping import CPE
    g = load_golden("G15_awgn_cma_cpe")
    out = CPE(torch.from_numpy(g["cpe_in"])).numpy()
    assert np.max(np.abs(out - g["cpe_out"])) < 2e-5


def test_shift_and_ser_mirrors_against_reference_cpu():
    from vae_equalizer_amd.func_CMA_MQAM_shaping import SER_CMA, find_shift_symb
    for name in ("G15_awgn_cma_16qam", "G15_awgn_cma_64qam"):
        g = load_golden(name)
        cpe, data = torch.from_numpy(g["cpe"].copy()), torch.from_numpy(g["data_valid"])
        s = int(find_shift_symb(cpe, data, 21))
        assert s == int(g["shift"]), name
        ser = SER_CMA(cpe[:, 11 + s:-11], data[:, 11:-11 - s], 2, torch.from_numpy(g["amp_levels"]), len(g["amp_levels"]))
        assert abs(float(ser) - float(g["SER"])) <= 2.0 / (cpe.shape[-1] - 22 - s), name
        assert not torch.equal(cpe, torch.from_numpy(g["cpe"]))                 # SER_CMA rescaled its window of cpe in place

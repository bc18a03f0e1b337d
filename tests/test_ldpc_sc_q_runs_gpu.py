"""fec= with an ScLdpcCode and the SC-only key fixed = dict(bits, ...) through the runners and a sweep script, as tests/test_ldpc_sc_runs_gpu.py checks
the float window decoder: the figures under "fec" are the fixed-point window decoder's integer model (tests/_ref_ldpc_sc_q.py) applied to the LLRs
and TX bits the same call returns, bit for bit; fec alone gives the same figures; the sweep script's .mat gains the four keys with the runner's
values.  What fec=None, an LdpcCode and an ScLdpcCode without fixed give is pinned by the existing tests.

sc_array_code(2, 4, 31, 12) (1488 bits) behind t0 = 13, window 5, 8 iterations per position, fixed = dict(bits=5): two chains in a 16-QAM DP frame of
400 symbols (w = 8) and two in an AWGN validation of 1000 symbols (w = 4)."""
import numpy as np
import pytest
import torch
from scipy import io

import _ref_ldpc_sc_q as S

pytestmark = pytest.mark.gpu

T0, W, ITERS, N_CHAIN = 13, 5, 8, 1488
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max")


def _fec(**over):
    from vae_equalizer_amd.engine import sc_array_code
    return dict(dict(code=sc_array_code(2, 4, 31, 12), t0=T0, window=W, iters=ITERS, fixed=dict(bits=5)), **over)


def _check_fec(fec, llr, bits, tag):
    """fec: the runner's dict; llr, bits [R, w, N] on the device."""
    R, w, N = llr.shape
    C = (N - T0) * w // N_CHAIN
    want = S.decode_batch(S.A, 31, 12, llr.cpu().numpy(), bits.cpu().numpy(), T0, C, W, S.DEFAULT, ITERS)[0]
    got = np.stack([fec[k].cpu().numpy() for k in FIGS], -1)
    print(f"{tag}: C = {C}; iters {want[..., 0].tolist()} ok {want[..., 1].tolist()} pre_err {want[..., 3].tolist()} erased {want[..., 4].tolist()} "
          f"post_err {want[..., 2].tolist()} iters_max {want[..., 5].tolist()}; kernel differs in {int((got != want).sum())} counters")
    assert C == 2 and all(fec[k].is_cuda and tuple(fec[k].shape) == (R, C) for k in FIGS) and fec["positions"] == 10
    assert "post" not in fec and "pos_err" not in fec and fec["quant"] == S.DEFAULT and np.array_equal(got, want)
    assert (want[..., 3] > 0).any() and (want[..., 0] > 0).any()                  # there was something to decode
    assert np.array_equal(fec["BER_post"].cpu().numpy(), (want[..., 2].sum(1) / np.float32(C * N_CHAIN)).astype(np.float32))
    assert np.array_equal(fec["BER_pre"].cpu().numpy(), (want[..., 3].sum(1) / np.float32(C * N_CHAIN)).astype(np.float32))
    assert np.array_equal(fec["FER"].cpu().numpy(), (want[..., 2] > 0).mean(1).astype(np.float32))


def _same_fec(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


def test_check_fec_takes_fixed_with_an_sc_code_only():
    from vae_equalizer_amd.engine import FEC_KEYS, FEC_SC_ONLY, BchCode, array_code, check_fec
    assert "fixed" in FEC_KEYS and "fixed" in FEC_SC_ONLY and FEC_KEYS[-1] == "outer" and FEC_KEYS.index("fixed") == len(FEC_KEYS) - 2
    check_fec(_fec())
    check_fec(_fec(fixed=None))
    check_fec(_fec(fixed=dict(bits=4, scale=0.5, app_bits=4, num=8, beta=1), test=2, outer=dict(code=BchCode(7, 2))))
    for bad in (dict(code=array_code(4, 24, 31), fixed=dict(bits=5)),             # fixed belongs to the window decoder
                _fec(alpha=0.75),                                                 # alpha belongs to the float decoder
                _fec(fixed=dict(bits=5, width=3)), _fec(fixed=dict(scale=1.0)), _fec(fixed=dict(bits=5.5)), _fec(fixed=5),
                _fec(quant=dict(bits=5)), {k: v for k, v in _fec(quant=dict(bits=5)).items() if k != "fixed"}):   # quant stays the block decoder's
        with pytest.raises(ValueError):
            check_fec(bad)


def test_fec_figures_sizes_its_chunks_by_the_int16_post(monkeypatch):
    """With an outer code fec_figures walks the runs in chunks whose post stays within OUTER_POST_BYTES: 2 bytes per value with fixed, 4 without,
    and the figures are those of one call either way."""
    from vae_equalizer_amd import engine, fec as fec_module     # fec_figures resolves ldpc_sc_decode and OUTER_POST_BYTES in fec
    from vae_equalizer_amd.engine import BchCode
    llr, bits = (torch.from_numpy(x).cuda() for x in S.grid_case(12, 8, 7, 1))
    fec = dict(_fec(t0=7, iters=1), outer=dict(code=BchCode(7, 2)))
    whole = engine.fec_figures(dict(llr=llr, bits=bits), fec)
    calls = []
    real = fec_module.ldpc_sc_decode
    monkeypatch.setattr(fec_module, "ldpc_sc_decode", lambda L, *a, **kw: (calls.append(L.shape[0]), real(L, *a, **kw))[1])
    monkeypatch.setattr(fec_module, "OUTER_POST_BYTES", 2 * S.C_ * N_CHAIN * 2)   # room for the int16 post of two runs, the float32 post of one
    parts = engine.fec_figures(dict(llr=llr, bits=bits), fec)
    assert calls == [2, 1]
    calls.clear()
    engine.fec_figures(dict(llr=llr, bits=bits), {k: v for k, v in fec.items() if k != "fixed"})
    assert calls == [1, 1, 1]
    assert set(whole) == set(parts) and whole["quant"] == parts["quant"] == S.DEFAULT
    assert all(torch.equal(whole[k], parts[k]) for k in FIGS) and all(torch.equal(whole["outer"][k], parts["outer"][k]) for k in whole["outer"])
    assert int(whole["outer"]["pre_err"].sum()) > 0


def test_run_dp_batch_sc_fixed_fec():
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    kw = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
              phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)
    runs = [DPRun(10 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]
    a = run_dp_batch(runs, want_llr=True, fec=_fec(), **kw)
    b = run_dp_batch(runs, fec=_fec(), **kw)
    c = run_dp_batch(runs, want_llr=True, fec=None, **kw)
    assert set(a) - set(c) == {"fec"} and set(a) - set(b) == {"llr"} and "fec" not in c
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    assert torch.equal(llr, c["llr"]["llr"]) and torch.equal(bits, c["llr"]["bits"])
    _check_fec(a["fec"], llr.reshape(4, 8, 400), bits.reshape(4, 8, 400), "run_dp_batch")
    assert _same_fec(a["fec"], b["fec"])
    for k in ("SER", "Var_est", "var"):
        for other in (b, c):
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(other[k], nan=-1.0)), k
    for bad in (_fec(alpha=0.75), _fec(fixed=dict(bits=5, width=3)), _fec(quant=dict(bits=5))):
        with pytest.raises(ValueError):
            run_dp_batch(runs, fec=bad, **kw)


def test_run_awgn_batch_sc_fixed_fec():
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    args = ("16-QAM", 2, 25, 100, 1000, 300, 4, 2, "h1")
    runs = [dict(SNR=snr, nu=0.0, lr_optim=5e-3, seed=400 + i) for i, snr in enumerate((8, 10, 12, 14))]
    run = lambda **kw: run_awgn_batch(runs, *args, generator="hip", seed=11, **kw)  # noqa: E731
    a, b, plain = run(want_llr=True, fec=_fec()), run(fec=_fec()), run()
    assert len(a) == 3 and len(b) == 3 and set(a[2]) == {"llr", "fec"} and set(b[2]) == {"fec"}
    assert torch.equal(torch.nan_to_num(a[0], nan=-1.0), torch.nan_to_num(plain, nan=-1.0)) and torch.equal(torch.nan_to_num(b[0], nan=-1.0), torch.nan_to_num(plain, nan=-1.0))
    _check_fec(a[2]["fec"], a[2]["llr"]["llr"], a[2]["llr"]["bits"], "run_awgn_batch")
    assert _same_fec(a[2]["fec"], b[2]["fec"])
    with pytest.raises(ValueError):
        run(fec=_fec(alpha=1.0))


def test_eval_run_shaping_vaele_sc_fixed_fec(tmp_path, monkeypatch):
    from vae_equalizer_amd import Eval_run_shaping_vaele as ev
    from vae_equalizer_amd import sweep
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    const = dict(mod="16-QAM", SNR_vec=[12], iter=2, num_epochs=4, N_valid=1000, train_len=700, base_seed=3)

    def main(fec):
        for k, v in dict(const, savePATH=str(tmp_path) + "/", fec_metrics=fec).items():
            monkeypatch.setattr(ev, k, v)
        name, d = ev.main()
        m = io.loadmat(name)["dict"]
        assert set(d) == set(m.dtype.names)
        return d, m

    d0, _ = main(None)
    d, m = main(_fec())
    assert sweep.FEC_KEYS == ("BER_post", "FER", "BER_pre_fec", "fec_iters") and set(d) == set(d0) | set(sweep.FEC_KEYS)
    for k in d0:                                            # every other key: unchanged
        assert np.array_equal(np.asarray(d[k]), np.asarray(d0[k]), equal_nan=True), k
    runs = [dict(SNR=12, nu=0, lr_optim=5e-3, seed=3 + 1000 * i) for i in range(2)]
    f = run_awgn_batch(runs, "16-QAM", 2, 25, 350, 1000, 700, 4, 2, "h1", generator=None, seed=3, fec=_fec())[2]["fec"]
    want = dict(BER_post=f["BER_post"], FER=f["FER"], BER_pre_fec=f["BER_pre"], fec_iters=f["iters"].double().mean(1).float())
    print({k: d[k].ravel().tolist() for k in sweep.FEC_KEYS}, "runner: iters", f["iters"].tolist(), "pre_err", f["pre_err"].tolist())
    assert f["quant"] == S.DEFAULT and int(f["pre_err"].sum()) > 0 and int(f["iters"].sum()) > 0 and tuple(f["iters"].shape) == (2, 2)
    for k in sweep.FEC_KEYS:
        assert d[k].shape == d["SER"].shape[:-1] and d[k].dtype == np.float32 and np.array_equal(d[k].ravel(), want[k].cpu().numpy()), k
        assert np.array_equal(np.asarray(m[k][0, 0]).ravel(), want[k].cpu().numpy()), k

"""run_dp_batch(fec=...) and run_cma_batch(fec=...): the figures under "fec" are the float32 model of tests/_ref_ldpc.py applied to the LLRs and
TX bits the same call returns under "llr" (bit for bit: tests/test_ldpc_gpu.py's comparison), fec without want_llr gives the same figures and
no "llr", and fec=None leaves the outputs as they were.  R = 4 runs of 16-QAM (w = 4 b = 8), two frames of 400 symbols, device generator."""
import numpy as np
import pytest
import torch

import _ref_ldpc as M

pytestmark = pytest.mark.gpu

KW = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
          phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip")
T0, MAX_ITER, ALPHA = 13, 8, 0.75
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased")


def _runs(lr, snr0):
    from vae_equalizer_amd.dp_runs import DPRun
    return [DPRun(snr0 + 2 * i, 0.0, 0.01, 0.3, lr, 90e9, seed=700 + i) for i in range(4)]


def _fec():
    from vae_equalizer_amd.engine import array_code
    return dict(code=array_code(4, 24, 31), t0=T0, max_iter=MAX_ITER, alpha=ALPHA)


def _check(a, b, c, N):
    """a: want_llr and fec, b: fec alone, c: want_llr alone."""
    assert set(a) - set(c) == {"fec"} and set(a) - set(b) == {"llr"} and "fec" not in c
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    assert tuple(llr.shape) == (4, 2, 4, N) and torch.equal(llr, c["llr"]["llr"]) and torch.equal(bits, c["llr"]["bits"])
    C = (N - T0) * 8 // 744
    want_out, _ = M.decode_batch(M.array_shifts(4, 24, 31), 31, llr.reshape(4, 8, N).cpu().numpy(), bits.reshape(4, 8, N).cpu().numpy(), T0, C,
                                 MAX_ITER, ALPHA)
    fec = a["fec"]
    got = np.stack([fec[k].cpu().numpy() for k in FIGS], -1)
    print(f"C = {C}; iters {want_out[..., 0].tolist()} ok {want_out[..., 1].tolist()} pre_err {want_out[..., 3].tolist()} "
          f"post_err {want_out[..., 2].tolist()} erased {want_out[..., 4].tolist()}; kernel differs in {int((got != want_out).sum())} counters")
    assert C >= 3 and all(fec[k].is_cuda and tuple(fec[k].shape) == (4, C) for k in FIGS) and "post" not in fec
    assert np.array_equal(got, want_out)
    assert (want_out[..., 3] > 0).any() and (want_out[..., 0] > 0).any()          # there was something to decode
    assert np.array_equal(fec["BER_post"].cpu().numpy(), (want_out[..., 2].sum(1) / np.float32(C * 744)).astype(np.float32))
    assert np.array_equal(fec["BER_pre"].cpu().numpy(), (want_out[..., 3].sum(1) / np.float32(C * 744)).astype(np.float32))
    assert np.array_equal(fec["FER"].cpu().numpy(), (want_out[..., 2] > 0).mean(1).astype(np.float32))
    for k in fec:
        assert torch.equal(fec[k], b["fec"][k]), k
    for k in ("SER", "Var_est", "var"):
        for other in (b, c):
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(other[k], nan=-1.0)), k


def test_run_dp_batch_fec():
    from vae_equalizer_amd.dp_runs import run_dp_batch
    kw = dict(KW, N_frame_max=400)
    runs = _runs(2.5e-3, 12)
    a = run_dp_batch(runs, want_llr=True, fec=_fec(), **kw)
    b = run_dp_batch(runs, fec=_fec(), **kw)
    c = run_dp_batch(runs, want_llr=True, fec=None, **kw)
    _check(a, b, c, 400)
    with pytest.raises(ValueError):
        run_dp_batch(runs, fec=dict(t0=T0), **kw)


@pytest.mark.parametrize("mode", ["CMA", "CMAflex"])
def test_run_cma_batch_fec(mode):
    from vae_equalizer_amd import cma_runs
    kw = dict(KW, N_train_max=400)
    runs = _runs(1e-4 if mode == "CMA" else 1e-5, 12)
    a = cma_runs.run_cma_batch(runs, mode, want_llr=True, fec=_fec(), **kw)
    b = cma_runs.run_cma_batch(runs, mode, fec=_fec(), **kw)
    c = cma_runs.run_cma_batch(runs, mode, want_llr=True, **kw)
    _check(a, b, c, 400 - 2 * cma_runs.N_CUT)

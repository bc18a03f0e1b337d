"""fec=dict(..., quant=dict(bits=5)) through the batch runners: run_dp_batch and run_dfe_batch return the integer model's figures
(tests/_ref_ldpc_q.py) on the LLRs and TX bits the same call returns, the same calls without quant return the float32 model's figures
(tests/_ref_ldpc.py) as before and every other output unchanged, and a bad quant dict is a ValueError before any launch.  The shapes are those of
tests/test_ldpc_runs_gpu.py (R = 4 runs of 16-QAM, two frames of 400 symbols) and tests/test_awgn_fec_gpu.py (two SNRs x two frames of 1100)."""
import numpy as np
import pytest
import torch

import _ref_ldpc as M
import _ref_ldpc_il as IL
import _ref_ldpc_q as Q

pytestmark = pytest.mark.gpu

KW = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
          phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)
T0, MAX_ITER, N_CODE = 13, 8, 744
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased")
PRM = dict(bits=5, scale=1.0, app_bits=7, num=6, beta=0)                          # what quant=dict(bits=5) resolves to
SHIFTS = M.array_shifts(4, 24, 31)


def _fec(**over):
    from vae_equalizer_amd.engine import array_code
    return dict(dict(code=array_code(4, 24, 31), t0=T0, max_iter=MAX_ITER), **over)


def _got(fec, shape):
    return np.stack([fec[k].cpu().numpy() for k in FIGS], -1).reshape(shape)


def _report(tag, want, got):
    print(f"{tag}: iters {want[..., 0].tolist()} ok {want[..., 1].tolist()} pre_err {want[..., 3].tolist()} post_err {want[..., 2].tolist()} "
          f"erased {want[..., 4].tolist()}; kernel differs in {int((got != want).sum())} counters")


def _no_launch(call):
    """call() raises ValueError, and does so before it allocated anything on the device (the runners check fec first, then generate and launch)."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for bad in (dict(bitz=5), dict()):
        with pytest.raises(ValueError):
            call(_fec(quant=bad))
    assert torch.cuda.memory_allocated() == before


def test_run_dp_batch_quant():
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    runs = [DPRun(12 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]
    N, C = 400, (400 - T0) * 8 // N_CODE
    a = run_dp_batch(runs, want_llr=True, fec=_fec(quant=dict(bits=5)), **KW)
    f = run_dp_batch(runs, want_llr=True, fec=_fec(), **KW)
    c = run_dp_batch(runs, want_llr=True, **KW)
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    assert tuple(llr.shape) == (4, 2, 4, N) and all(torch.equal(a["llr"][k], c["llr"][k]) and torch.equal(f["llr"][k], c["llr"][k]) for k in ("llr", "bits"))
    ln, bn = llr.reshape(4, 8, N).cpu().numpy(), bits.reshape(4, 8, N).cpu().numpy()
    want, _ = Q.decode_batch(SHIFTS, 31, ln, bn, T0, C, PRM, MAX_ITER)
    got = _got(a["fec"], want.shape)
    _report("run_dp_batch quant", want, got)
    assert C >= 3 and a["fec"]["quant"] == PRM and "post" not in a["fec"]
    assert np.array_equal(got, want) and (want[..., 3] > 0).any() and (want[..., 0] > 0).any()
    assert np.array_equal(a["fec"]["BER_post"].cpu().numpy(), (want[..., 2].sum(1) / np.float32(C * N_CODE)).astype(np.float32))
    want_f, _ = M.decode_batch(SHIFTS, 31, ln, bn, T0, C, MAX_ITER, 0.75)                 # without quant: the float decoder, as before
    got_f = _got(f["fec"], want_f.shape)
    _report("run_dp_batch float", want_f, got_f)
    assert "quant" not in f["fec"] and np.array_equal(got_f, want_f) and np.array_equal(got[..., 3], got_f[..., 3])
    for k in ("SER", "Var_est", "var"):
        for other in (f, c):
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(other[k], nan=-1.0)), k
    _no_launch(lambda fec: run_dp_batch(runs, fec=fec, **KW))


def test_run_dfe_batch_quant():
    from vae_equalizer_amd import DFE_MQAM_shaping as D
    args, kw, N = ([12, 16], 2, 1100, "16-QAM"), dict(nu=0.0872449, seed=5, generator="hip"), 1100
    S = 186
    C = (N - T0) // S
    a = D.run_dfe_batch(*args, **kw, want_llr=True, fec=_fec(depth=C, quant=dict(bits=5)))
    f = D.run_dfe_batch(*args, **kw, want_llr=True, fec=_fec(depth=C))
    c = D.run_dfe_batch(*args, **kw, want_llr=True)
    for k in c:                                                                  # every other key, bit for bit, whatever the decoder
        for other in (a, f):
            if isinstance(c[k], torch.Tensor):
                assert torch.equal(torch.nan_to_num(c[k], nan=-1.0), torch.nan_to_num(other[k], nan=-1.0)), k
            elif isinstance(c[k], dict):
                assert all(torch.equal(c[k][j], other[k][j]) for j in c[k]), k
            else:
                assert np.array_equal(np.asarray(c[k]), np.asarray(other[k])), k
    for tag in ("mmse", "dfe"):
        out = a["llr_" + tag]
        ln, bn = out["llr"].reshape(4, 4, N).cpu().numpy(), out["bits"].reshape(4, 4, N).cpu().numpy()
        want, _ = Q.decode_batch(SHIFTS, 31, ln, bn, T0, C, PRM, MAX_ITER, depth=C)
        fec = a["fec_" + tag]
        got = _got(fec, want.shape)
        _report("run_dfe_batch quant " + tag, want, got)
        assert fec["quant"] == PRM and all(tuple(fec[k].shape) == (2, 2, C) for k in FIGS) and tuple(fec["FER"].shape) == (2, 2)
        assert np.array_equal(got, want) and (want[..., 3] > 0).any() and (want[..., 0] > 0).any()
        want_f, _ = IL.decode_batch_il(SHIFTS, 31, ln, bn, T0, C, C, MAX_ITER, 0.75)
        got_f = _got(f["fec_" + tag], want_f.shape)
        _report("run_dfe_batch float " + tag, want_f, got_f)
        assert "quant" not in f["fec_" + tag] and np.array_equal(got_f, want_f)
    _no_launch(lambda fec: D.run_dfe_batch(*args, **kw, fec=fec))

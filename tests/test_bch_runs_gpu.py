"""outer= of the runners' fec= and of the sweep scripts' fec_metrics: run_dp_batch and run_awgn_batch at the small shapes of
tests/test_ldpc_runs_gpu.py and tests/test_awgn_fec_gpu.py, Eval_run_shaping_vaele at tests/test_eval_fec_gpu.py's.  What a runner returns under
"fec"["outer"] is the two numpy models chained on the LLRs and TX bits the same call returns -- tests/_ref_ldpc.py (behind tests/_ref_ldpc_il.py's
interleaver on the AWGN path) and then tests/_ref_bch.py on its final LLRs -- bit for bit, and everything else in the return value is what the
call without outer returns.  The sweep script's .mat gains exactly BER_outer and FER_outer, the runner's values; every other key is unchanged.
array_code(4, 24, 31) (n = 744, payload (24 - 4) 31 = 620) in front of BchCode(8, 4) (255 bits, bit-interleaved over the run)."""
import numpy as np
import pytest
import scipy.io as io
import torch

import _ref_bch as B
import _ref_ldpc as M
import _ref_ldpc_il as IL

pytestmark = pytest.mark.gpu

T0, MAX_ITER, ALPHA, N_CODE, S, K = 13, 8, 0.75, 744, 186, 620
OUT = ("status", "pre_err", "bit_err", "nflip")


def _fec(depth=None, outer=True):
    from vae_equalizer_amd.engine import BchCode, array_code
    d = dict(code=array_code(4, 24, 31), t0=T0, max_iter=MAX_ITER, alpha=ALPHA, depth=depth)
    return dict(d, outer=dict(code=BchCode(8, 4))) if outer else d


def _same(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if torch.is_tensor(x):
        x, y = (torch.view_as_real(v) if v.is_complex() else v for v in (x, y))
        return x.dtype == y.dtype and torch.equal(torch.nan_to_num(x.float(), nan=-1.0), torch.nan_to_num(y.float(), nan=-1.0))
    if isinstance(x, (bool, int, float, str, list, tuple, np.ndarray, type(None))):
        return type(x) is type(y) and np.array_equal(np.asarray(x), np.asarray(y))
    return type(x) is type(y)                               # (a run's own objects, such as the DP runner's engine)


def _check_outer(got, llr, bits, depth, tag):
    """got: the runner's "fec" dict; llr, bits [R, w, N] on the device: the two models chained."""
    R, w, N = llr.shape
    C = (N - T0) // S if depth else (N - T0) * w // N_CODE
    shifts = M.array_shifts(4, 24, 31)
    if depth:
        want_ldpc, post = IL.decode_batch_il(shifts, 31, llr.cpu().numpy(), bits.cpu().numpy(), T0, C, depth, MAX_ITER, ALPHA)
    else:
        want_ldpc, post = M.decode_batch(shifts, 31, llr.cpu().numpy(), bits.cpu().numpy(), T0, C, MAX_ITER, ALPHA)
    C_o = C * K // 255
    want, _, count = B.outer(post, bits.cpu().numpy(), 8, 4, 255, C_o, K, 1, T0, depth)
    o = got["outer"]
    have = np.stack([o[k].cpu().numpy() for k in OUT], -1)
    print(f"{tag}: C = {C}, C_o = {C_o}; LDPC post_err {want_ldpc[..., 2].tolist()}; outer status {want[..., 0].tolist()} pre_err {want[..., 1].tolist()} "
          f"post_err {want[..., 2].tolist()}; {dict(count)}; kernel differs in {int((have != want).sum())} counters")
    assert C_o >= 1 and have.shape == want.shape and np.array_equal(have, want)
    assert np.array_equal(np.stack([got[k].cpu().numpy() for k in ("iters", "ok", "bit_err", "pre_err", "erased")], -1), want_ldpc)
    assert int(want[..., 1].sum()) > 0 and "post" not in got and "loc" not in o   # the outer code had errors to see
    for k, v in B.figures(want, 255).items():
        assert np.array_equal(o[k].cpu().numpy(), v), k
    return o


def test_run_dp_batch_outer():
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    kw = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
              phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)
    runs = [DPRun(12 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]
    a = run_dp_batch(runs, want_llr=True, fec=_fec(), **kw)
    plain = run_dp_batch(runs, want_llr=True, fec=_fec(outer=False), **kw)
    assert set(a) == set(plain) and set(a["fec"]) == set(plain["fec"]) | {"outer"}
    for k in plain:                                         # everything else is what the call without outer returns
        assert _same({x: v for x, v in a[k].items() if x != "outer"} if k == "fec" else a[k], plain[k]), k
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    _check_outer(a["fec"], llr.reshape(4, 8, 400), bits.reshape(4, 8, 400), None, "run_dp_batch")
    with pytest.raises(ValueError):
        run_dp_batch(runs, fec=dict(_fec(), outer=dict(code=_fec()["code"])), **kw)


def test_run_awgn_batch_outer():
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    args = ("16-QAM", 2, 25, 100, 1000, 300, 4, 2, "h1")
    runs = [dict(SNR=snr, nu=0.0, lr_optim=5e-3, seed=400 + i) for i, snr in enumerate((10, 12, 14, 16))]
    run = lambda **kw: run_awgn_batch(runs, *args, generator="hip", seed=11, **kw)  # noqa: E731
    a = run(want_info=True, want_llr=True, fec=_fec(5))
    plain = run(want_info=True, want_llr=True, fec=_fec(5, outer=False))
    assert len(a) == 3 and _same(a[0], plain[0]) and _same(a[1], plain[1]) and _same(a[2]["llr"], plain[2]["llr"])
    assert set(a[2]) == set(plain[2]) and set(a[2]["fec"]) == set(plain[2]["fec"]) | {"outer"}
    assert _same({k: v for k, v in a[2]["fec"].items() if k != "outer"}, plain[2]["fec"])
    _check_outer(a[2]["fec"], a[2]["llr"]["llr"], a[2]["llr"]["bits"], 5, "run_awgn_batch")
    with pytest.raises(ValueError):
        run(fec=dict(_fec(5), outer=dict(code=None)))


def test_eval_run_shaping_vaele_outer(tmp_path, monkeypatch):
    from vae_equalizer_amd import Eval_run_shaping_vaele as ev
    from vae_equalizer_amd import sweep
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    const = dict(mod="16-QAM", SNR_vec=[14], iter=2, num_epochs=4, N_valid=1000, train_len=700, base_seed=3)

    def main(fec):
        for k, v in dict(const, savePATH=str(tmp_path) + "/", fec_metrics=fec).items():
            monkeypatch.setattr(ev, k, v)
        name, d = ev.main()
        m = io.loadmat(name)["dict"]
        assert set(d) == set(m.dtype.names)
        return d, m

    d0, _ = main(_fec(5, outer=False))
    d, m = main(_fec(5))
    assert sweep.FEC_KEYS == ("BER_post", "FER", "BER_pre_fec", "fec_iters") and sweep.FEC_OUTER_KEYS == ("BER_outer", "FER_outer")
    assert set(d) == set(d0) | set(sweep.FEC_OUTER_KEYS) and set(sweep.FEC_KEYS) <= set(d0)
    for k in d0:                                            # every other key: unchanged
        assert np.array_equal(np.asarray(d[k]), np.asarray(d0[k]), equal_nan=True), k
    runs = [dict(SNR=14, nu=0, lr_optim=5e-3, seed=3 + 1000 * i) for i in range(2)]
    r = run_awgn_batch(runs, "16-QAM", 2, 25, 350, 1000, 700, 4, 2, "h1", generator=None, seed=3, fec=_fec(5))
    o = r[2]["fec"]["outer"]
    print({k: d[k].ravel().tolist() for k in sweep.FEC_OUTER_KEYS}, "runner", o["BER_outer"].tolist(), o["FER_outer"].tolist(), "BER_in", o["BER_in"].tolist())
    for k in sweep.FEC_OUTER_KEYS:
        assert d[k].shape == d["SER"].shape[:-1] and d[k].dtype == np.float32 and np.array_equal(d[k].ravel(), o[k].cpu().numpy()), k
        assert np.array_equal(np.asarray(m[k][0, 0]).ravel(), o[k].cpu().numpy()), k
    assert tuple(o["status"].shape) == (2, 12)

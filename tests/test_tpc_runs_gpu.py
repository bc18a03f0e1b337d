"""fec= with a ProductCode through the runners, as tests/test_staircase_runs_gpu.py checks the staircase code, and the decoder's stream as the input
of another decoder.

run_dp_batch and run_awgn_batch with fec = dict(code=ProductCode(...), ...): the figures under "fec" are engine.tpc_decode's, called by hand on the
LLRs and TX bits the same call returns, and model (1)'s (tests/_ref_tpc.py) under the scale the call resolved -- the default scale is a device
reduction whose last bit numpy need not share, every figure behind it is exact.  fec alone gives the same figures.  The extended (32, 26)^2 code
behind t0 = 13: three blocks in a 16-QAM DP frame of 400 symbols (w = 8) and three in an AWGN validation of 1000 symbols (w = 4).
A sweep script's .mat gains the four keys with the runner's values, fec_iters being the mean over the blocks of the half-iterations executed.
Then engine.staircase_decode on the kernel's stream against tests/_ref_staircase.py on the model's stream: the stream is a valid [R, 1, C n]
input, bit for bit."""
import numpy as np
import pytest
import torch
from scipy import io

import _ref_staircase as S
import _ref_tpc as T
import _tpc_cases as K

pytestmark = pytest.mark.gpu

T0, ITERS, P, N_BLOCK = 13, 3, 4, 1024
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "pay_err", "nstat2", "nbeta")
KEYS = set(FIGS) | {"BER_post", "BER_pre", "BER_payload", "FER", "alpha", "beta", "scale", "clip"}


def _code():
    from vae_equalizer_amd.engine import ProductCode, hamming_code
    return ProductCode(hamming_code(5), hamming_code(5))


def _fec(**over):
    return dict(dict(code=_code(), t0=T0, iters=ITERS, patterns=P), **over)


def _same_fec(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


def _check_fec(fec, llr, bits, tag):
    """fec: the runner's dict; llr, bits [R, w, N] on the device."""
    from vae_equalizer_amd.engine import tpc_decode
    R, w, N = llr.shape
    C = (N - T0) * w // N_BLOCK
    hand = tpc_decode(llr, bits, _code(), t0=T0, iters=ITERS, patterns=P)
    assert set(fec) == KEYS and _same_fec(fec, hand)
    cols = K.CODES["e32"][0]
    scale = fec["scale"].cpu().numpy()
    want = T.decode(llr.cpu().numpy(), bits.cpu().numpy(), cols, cols, P, ITERS, T.schedule(T.ALPHA, ITERS), T.schedule(T.BETA, ITERS), scale, T.CLIP,
                    26, 26, T0, C)[0]
    got = np.stack([fec[k].cpu().numpy() for k in FIGS], -1)
    print(f"{tag}: C = {C}; scale {scale.tolist()} half-iterations {want[..., 0].tolist()} ok {want[..., 1].tolist()} pre_err {want[..., 3].tolist()} "
          f"post_err {want[..., 2].tolist()} nbeta {want[..., 7].tolist()}; kernel differs in {int((got != want).sum())} counters")
    assert C == 3 and all(fec[k].is_cuda and tuple(fec[k].shape) == (R, C) for k in FIGS) and tuple(fec["scale"].shape) == (R,)
    assert np.array_equal(got, want)
    assert (want[..., 3] > 0).any() and (want[..., 0] > 1).any()                  # there was something to decode
    for k, v in T.figures(want, N_BLOCK, 26 * 26).items():
        assert np.array_equal(fec[k].cpu().numpy(), v), k
    finite = np.where(np.isfinite(llr.cpu().numpy()), np.abs(llr.cpu().numpy()), 0.0)
    assert np.allclose(scale, finite.reshape(R, -1).mean(1, dtype=np.float64), rtol=1e-5)


def test_run_dp_batch_tpc_fec():
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    kw = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
              phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)
    runs = [DPRun(10 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]
    a = run_dp_batch(runs, want_llr=True, fec=_fec(), **kw)
    b = run_dp_batch(runs, fec=_fec(), **kw)
    assert set(a) - set(b) == {"llr"} and "fec" in b
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    _check_fec(a["fec"], llr.reshape(4, 8, 400), bits.reshape(4, 8, 400), "run_dp_batch")
    assert _same_fec(a["fec"], b["fec"])
    for bad in (_fec(window=2), _fec(max_iter=8), _fec(outer=dict(code=None)), _fec(patterns=7), _fec(alpha=[0.5])):
        with pytest.raises(ValueError):
            run_dp_batch(runs, fec=bad, **kw)


def test_run_awgn_batch_tpc_fec():
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    args = ("16-QAM", 2, 25, 100, 1000, 300, 4, 2, "h1")
    runs = [dict(SNR=snr, nu=0.0, lr_optim=5e-3, seed=400 + i) for i, snr in enumerate((8, 10, 12, 14))]
    run = lambda **kw: run_awgn_batch(runs, *args, generator="hip", seed=11, **kw)  # noqa: E731
    a, b = run(want_llr=True, fec=_fec()), run(fec=_fec())
    assert len(a) == 3 and len(b) == 3 and set(a[2]) == {"llr", "fec"} and set(b[2]) == {"fec"}
    _check_fec(a[2]["fec"], a[2]["llr"]["llr"], a[2]["llr"]["bits"], "run_awgn_batch")
    assert _same_fec(a[2]["fec"], b[2]["fec"])
    with pytest.raises(ValueError):
        run(fec=_fec(depth=5))


def test_eval_run_shaping_vaele_tpc_fec(tmp_path, monkeypatch):
    from vae_equalizer_amd import Eval_run_shaping_vaele as ev
    from vae_equalizer_amd import sweep
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    for k, v in dict(mod="16-QAM", SNR_vec=[12], iter=2, num_epochs=4, N_valid=1000, train_len=700, base_seed=3, savePATH=str(tmp_path) + "/",
                     fec_metrics=_fec()).items():
        monkeypatch.setattr(ev, k, v)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    assert set(d) == set(m.dtype.names) and set(sweep.FEC_KEYS) <= set(d)
    runs = [dict(SNR=12, nu=0, lr_optim=5e-3, seed=3 + 1000 * i) for i in range(2)]
    f = run_awgn_batch(runs, "16-QAM", 2, 25, 350, 1000, 700, 4, 2, "h1", generator=None, seed=3, fec=_fec())[2]["fec"]
    want = dict(BER_post=f["BER_post"], FER=f["FER"], BER_pre_fec=f["BER_pre"], fec_iters=f["iters"].double().mean(1).float())
    print({k: d[k].ravel().tolist() for k in sweep.FEC_KEYS}, "runner: half-iterations", f["iters"].tolist(), "pre_err", f["pre_err"].tolist())
    assert int(f["pre_err"].sum()) > 0 and tuple(f["iters"].shape) == (2, 3)
    for k in sweep.FEC_KEYS:
        assert d[k].shape == d["SER"].shape[:-1] and d[k].dtype == np.float32 and np.array_equal(d[k].ravel(), want[k].cpu().numpy()), k
        assert np.array_equal(np.asarray(m[k][0, 0]).ravel(), want[k].cpu().numpy()), k


def test_staircase_on_the_tpc_stream():
    from vae_equalizer_amd.engine import BchCode, HammingCode, ProductCode, StaircaseCode, staircase_decode, tpc_decode
    case = next(c for c in K.CASES if c.col == "e32" and c.p == 4)
    stair, chain = (5, 1, 12, 3), 432                          # m, t, s, L of StaircaseCode(BchCode(5, 1, n=24), 3)
    llr, bits = K.tensors(case)
    out, s_llr, s_bits = K.expected(case)[:3]
    chains = case.C * N_BLOCK // chain
    want = S.decode(s_llr[:, None, :], s_bits[:, None, :], *stair, 2, 8, 0, chains)
    alpha, beta = K.schedules(case)
    scale = K.scale_of(case, llr)
    first = tpc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), ProductCode(HammingCode(*K.CODES["e32"]), HammingCode(*K.CODES["e32"])),
                       t0=case.t0, blocks=case.C, iters=case.iters, patterns=case.p, alpha=alpha, beta=beta, clip=case.clip, payload=(case.K1, case.K2),
                       scale=torch.ones(case.R, device="cuda") if scale is None else torch.from_numpy(scale).cuda(), want_stream=True)
    got = staircase_decode(first["stream"]["llr"], first["stream"]["bits"], StaircaseCode(BchCode(5, 1, n=24), 3), 2, iters=8, want_hard=True)
    torch.cuda.synchronize()
    fig = np.stack([got[k].cpu().numpy() for k in ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max", "nflip", "bad_flips")], -1)
    print(f"product code: pre_err {out[..., 3].tolist()} post_err {out[..., 2].tolist()}; staircase on {chains} chains: pre_err {want[0][..., 3].tolist()} "
          f"post_err {want[0][..., 2].tolist()}; differs in {int((fig != want[0]).sum())} counters, "
          f"{int((got['hard'].cpu().numpy() != want[1]).sum())} decisions")
    assert chains == 7 and tuple(got["iters"].shape) == (case.R, chains)
    assert np.array_equal(first["stream"]["llr"].cpu().numpy()[:, 0], s_llr) and np.array_equal(first["stream"]["bits"].cpu().numpy()[:, 0], s_bits)
    assert np.array_equal(fig, want[0]) and np.array_equal(got["hard"].cpu().numpy(), want[1])
    assert np.array_equal(want[0][..., 3].sum(1), ((s_llr < 0) != (s_bits == 1))[:, :chains * chain].sum(1))     # its input errors are the stream's

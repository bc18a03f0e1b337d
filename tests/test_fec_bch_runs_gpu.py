"""fec= over (extended) t = 2 BCH words through the runners, at the frames of tests/test_tpc_runs_gpu.py and tests/test_chase_staircase_gpu.py:
400-symbol 16-QAM DP frames (w = 8) and 1000-symbol AWGN validations (w = 4), t0 = 13.

run_dp_batch and run_awgn_batch with fec = dict(code=ProductCode(ebch_code(5), ebch_code(5)), ...): the figures under "fec" are
engine.tpc_decode's, called by hand on the LLRs and TX bits the same call returns, and model (1)'s (tests/_ref_ebch.py) under the scale the call
resolved.  run_dp_batch with fec = dict(code=StaircaseCode(...), window, inner=dict(code=ebch_code(5), patterns=4)): "inner" is
engine.chase_decode's dict, the staircase figures are engine.staircase_decode's on its stream, both by hand, and equal model (1) followed by
tests/_ref_staircase.py on the model's stream.  No runner or sweep script knows the kind of code: the dispatch is engine.fec_figures'."""
import numpy as np
import pytest
import torch

import _ebch_cases as K
import _ref_ebch as E
import _ref_staircase as S
import _ref_tpc as T

pytestmark = pytest.mark.gpu

T0, ITERS, P, N_BLOCK = 13, 3, 4, 1024
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "pay_err", "nstat2", "nbeta")
KEYS = set(FIGS) | {"BER_post", "BER_pre", "BER_payload", "FER", "alpha", "beta", "scale", "clip"}
STAIR, WINDOW, S_ITERS, N_CHAIN = (5, 1, 12, 3), 2, 8, 432     # m, t, s, L of StaircaseCode(BchCode(5, 1, n=24), 3)
S_FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max", "nflip", "bad_flips")
S_KEYS = set(S_FIGS) | {"BER_post", "BER_pre", "FER", "positions"}
DP = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
          phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)


def _code():
    from vae_equalizer_amd.engine import ProductCode, ebch_code
    return ProductCode(ebch_code(5), ebch_code(5))


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
    x32 = K.CODES["x32"]
    scale = fec["scale"].cpu().numpy()
    want = E.decode_tpc(llr.cpu().numpy(), bits.cpu().numpy(), x32, x32, P, ITERS, T.schedule(T.ALPHA, ITERS), T.schedule(T.BETA, ITERS), scale, T.CLIP,
                        21, 21, T0, C)[0]
    got = np.stack([fec[k].cpu().numpy() for k in FIGS], -1)
    print(f"{tag}: C = {C}; scale {scale.tolist()} half-iterations {want[..., 0].tolist()} ok {want[..., 1].tolist()} pre_err {want[..., 3].tolist()} "
          f"post_err {want[..., 2].tolist()} nbeta {want[..., 7].tolist()}; kernel differs in {int((got != want).sum())} counters")
    assert C == 3 and all(fec[k].is_cuda and tuple(fec[k].shape) == (R, C) for k in FIGS) and tuple(fec["scale"].shape) == (R,)
    assert np.array_equal(got, want)
    assert (want[..., 3] > 0).any() and (want[..., 0] > 1).any()                  # there was something to decode
    for k, v in T.figures(want, N_BLOCK, 21 * 21).items():
        assert np.array_equal(fec[k].cpu().numpy(), v), k


def _dp_runs():
    from vae_equalizer_amd.dp_runs import DPRun
    return [DPRun(10 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]


def test_run_dp_batch_tpc_bch_fec():
    from vae_equalizer_amd.dp_runs import run_dp_batch
    runs = _dp_runs()
    a = run_dp_batch(runs, want_llr=True, fec=_fec(), **DP)
    b = run_dp_batch(runs, fec=_fec(), **DP)
    assert set(a) - set(b) == {"llr"} and "fec" in b
    _check_fec(a["fec"], a["llr"]["llr"].reshape(4, 8, 400), a["llr"]["bits"].reshape(4, 8, 400), "run_dp_batch")
    assert _same_fec(a["fec"], b["fec"])
    for bad in (_fec(window=2), _fec(max_iter=8), _fec(patterns=7), _fec(alpha=[0.5])):
        with pytest.raises(ValueError):
            run_dp_batch(runs, fec=bad, **DP)


def test_run_awgn_batch_tpc_bch_fec():
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


def test_run_dp_batch_inner_bch_fec():
    from vae_equalizer_amd.dp_runs import run_dp_batch
    from vae_equalizer_amd.engine import BchCode, StaircaseCode, chase_decode, ebch_code, staircase_decode
    x32, stair = ebch_code(5), StaircaseCode(BchCode(5, 1, n=24), 3)
    runs = _dp_runs()
    fec = dict(code=stair, t0=T0, window=WINDOW, iters=S_ITERS, inner=dict(code=x32, patterns=4))
    a = run_dp_batch(runs, want_llr=True, fec=fec, **DP)
    assert set(a["fec"]) == S_KEYS | {"inner"}
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    inner = chase_decode(llr, bits, x32, t0=T0, patterns=4, spread=True, want_stream=True)
    words = (400 - T0) * 8 // 32
    chains = words * 21 // N_CHAIN
    assert tuple(inner["status"].shape) == (4, words) and inner["stream"]["llr"].shape == (4, 1, words * 21)
    outer = staircase_decode(inner["stream"]["llr"], inner["stream"]["bits"], stair, WINDOW, iters=S_ITERS)
    f = a["fec"]
    print(f"inner: BER_pre {inner['BER_pre'].tolist()} BER_payload {inner['BER_payload'].tolist()}; staircase on {chains} chains: pre_err "
          f"{outer['pre_err'].tolist()} bit_err {outer['bit_err'].tolist()}")
    assert "stream" not in f["inner"] and set(f["inner"]) == set(inner) - {"stream"}
    for k in f["inner"]:
        assert torch.equal(f["inner"][k], inner[k]), k
    assert torch.equal(f["BER_pre"], inner["BER_pre"]) and int(inner["pre_err"].sum()) > 0
    assert tuple(f["iters"].shape) == (4, chains) and f["positions"] == outer["positions"] == 2
    for k in S_KEYS - {"BER_pre", "positions"}:
        assert torch.equal(f[k], outer[k]), k
    # the model on the same LLRs: the inner decoder's counters and the staircase's on its stream
    m_out, m_llr, m_bits, _ = E.decode_chase(llr.reshape(4, 8, 400).cpu().numpy(), bits.reshape(4, 8, 400).cpu().numpy(), K.CODES["x32"], 4, 21, T0,
                                             words, 0, 1)
    assert np.array_equal(np.stack([inner[k].cpu().numpy() for k in ("status", "pre_err", "bit_err", "nflip", "erased", "pay_err")], -1), m_out)
    assert np.array_equal(inner["stream"]["llr"].cpu().numpy()[:, 0], m_llr) and np.array_equal(inner["stream"]["bits"].cpu().numpy()[:, 0], m_bits)
    want = S.decode(m_llr[:, None, :], m_bits[:, None, :], *STAIR, WINDOW, S_ITERS, 0, chains)[0]
    assert np.array_equal(np.stack([f[k].cpu().numpy() for k in S_FIGS], -1), want)

"""The concatenated scheme: engine.chase_decode's payload stream as the input of engine.staircase_decode, and fec= with inner= through a runner.

The stream is a [R, 1, C K] tensor pair like any other, so the staircase decoder behind the inner code must give what tests/_ref_staircase.py
gives on the stream of tests/_ref_chase.py: all eight counters and the hard decisions, bit for bit.  Words of the extended (16, 11) Hamming code
into StaircaseCode(BchCode(5, 1, n=24), 3) (chains of 432 bits), window 2.  Then one run_dp_batch with fec = dict(code, window, inner) at the frame
of tests/test_staircase_runs_gpu.py: "inner" comes back, BER_pre is the inner decoder's, and the figures are those of the two engine calls made by
hand on the LLRs the same call returns.  A fec dict without inner returns the keys it always did."""
import numpy as np
import pytest
import torch

import _chase_cases as K
import _ref_chase as X
import _ref_staircase as S

pytestmark = pytest.mark.gpu

STAIR = (5, 1, 12, 3)                                      # m, t, s, L of StaircaseCode(BchCode(5, 1, n=24), 3)
WINDOW, ITERS, N_CHAIN = 2, 8, 432
FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max", "nflip", "bad_flips")
KEYS = set(FIGS) | {"BER_post", "BER_pre", "FER", "positions"}
CASE = K.Case("e16-concat", "e16", 3, 4, 5, 0, 11, 1, 0.45, 3, 80, 9950)


def _codes():
    from vae_equalizer_amd.engine import BchCode, StaircaseCode, hamming_code
    return hamming_code(4), StaircaseCode(BchCode(5, 1, n=24), 3)


def test_staircase_on_the_chase_stream():
    from vae_equalizer_amd.engine import chase_decode, staircase_decode
    ham, stair = _codes()
    llr, bits = K.tensors(CASE)
    out, s_llr, s_bits, _ = K.expected(CASE)
    chains = CASE.C * CASE.K // N_CHAIN
    want = S.decode(s_llr[:, None, :], s_bits[:, None, :], *STAIR, WINDOW, ITERS, 0, chains)
    inner = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), ham, t0=CASE.t0, codewords=CASE.C, patterns=CASE.p,
                         payload=CASE.K, spread=True, want_stream=True)
    got = staircase_decode(inner["stream"]["llr"], inner["stream"]["bits"], stair, WINDOW, iters=ITERS, want_hard=True)
    torch.cuda.synchronize()
    fig = np.stack([got[k].cpu().numpy() for k in FIGS], -1)
    print(f"inner: pre_err {int(out[..., 1].sum())} pay_err {int(out[..., 5].sum())} of {CASE.R * CASE.C * CASE.K}; staircase on {chains} chains: "
          f"pre_err {want[0][..., 3].tolist()} post_err {want[0][..., 2].tolist()} nflip {want[0][..., 6].tolist()}; differs in "
          f"{int((fig != want[0]).sum())} counters, {int((got['hard'].cpu().numpy() != want[1]).sum())} decisions")
    assert chains == 2 and tuple(got["iters"].shape) == (CASE.R, chains)
    assert np.array_equal(inner["stream"]["llr"].cpu().numpy()[:, 0], s_llr) and np.array_equal(inner["stream"]["bits"].cpu().numpy()[:, 0], s_bits)
    assert np.array_equal(fig, want[0]) and np.array_equal(got["hard"].cpu().numpy(), want[1])
    assert (want[0][..., 3] > 0).any() and (want[0][..., 6] > 0).any()          # the inner code left the staircase something to do
    assert np.array_equal(want[0][..., 3].sum(1), ((s_llr < 0) != (s_bits == 1))[:, :chains * N_CHAIN].sum(1))     # its input errors are the stream's


def test_run_dp_batch_inner_fec():
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    from vae_equalizer_amd.engine import chase_decode, staircase_decode
    ham, stair = _codes()
    kw = dict(mod="16-QAM", sps=2, M_est=25, batch_len=100, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
              phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip", N_frame_max=400)
    runs = [DPRun(10 + 2 * i, 0.0, 0.01, 0.3, 2.5e-3, 90e9, seed=700 + i) for i in range(4)]
    plain = dict(code=stair, t0=13, window=WINDOW, iters=ITERS)
    fec = dict(plain, inner=dict(code=ham, patterns=3, spread=True))
    a = run_dp_batch(runs, want_llr=True, fec=fec, **kw)
    b = run_dp_batch(runs, fec=plain, **kw)
    assert set(a["fec"]) == KEYS | {"inner"} and set(b["fec"]) == KEYS                  # without inner: the keys it always returned
    llr, bits = a["llr"]["llr"], a["llr"]["bits"]
    inner = chase_decode(llr, bits, ham, t0=13, patterns=3, spread=True, want_stream=True)
    words = (400 - 13) * 8 // 16
    assert tuple(inner["status"].shape) == (4, words) and inner["stream"]["llr"].shape == (4, 1, words * 11)
    outer = staircase_decode(inner["stream"]["llr"], inner["stream"]["bits"], stair, WINDOW, iters=ITERS)
    f = a["fec"]
    print(f"inner: BER_pre {inner['BER_pre'].tolist()} BER_payload {inner['BER_payload'].tolist()}; staircase: pre_err {outer['pre_err'].tolist()} "
          f"bit_err {outer['bit_err'].tolist()}")
    assert "stream" not in f["inner"] and set(f["inner"]) == set(inner) - {"stream"}
    for k in f["inner"]:
        assert torch.equal(f["inner"][k], inner[k]), k
    assert torch.equal(f["BER_pre"], inner["BER_pre"]) and int(inner["pre_err"].sum()) > 0
    assert tuple(f["iters"].shape) == (4, words * 11 // N_CHAIN) and f["positions"] == outer["positions"] == 2
    for k in KEYS - {"BER_pre", "positions"}:
        assert torch.equal(f[k], outer[k]), k
    # the model on the same LLRs: the inner decoder's counters and the staircase's on its stream
    m_out, m_llr, m_bits, _ = X.decode(llr.reshape(4, 8, 400).cpu().numpy(), bits.reshape(4, 8, 400).cpu().numpy(), ham.cols, 3, 11, 13, words, 0, 1)
    assert np.array_equal(np.stack([inner[k].cpu().numpy() for k in ("status", "pre_err", "bit_err", "nflip", "erased", "pay_err")], -1), m_out)
    want = S.decode(m_llr[:, None, :], m_bits[:, None, :], *STAIR, WINDOW, ITERS, 0, words * 11 // N_CHAIN)[0]
    assert np.array_equal(np.stack([f[k].cpu().numpy() for k in FIGS], -1), want)

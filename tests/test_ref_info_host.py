"""The float64 model of the information-rate figures (tests/_ref_info.py) against closed forms, and the preconditions the GPU cases of
tests/test_epilogue_info_gpu.py rely on: posteriors at the transmitted level >= 1e-30 (float32 and float64 logs agree), decision margins
above the floor tests/test_ref_epilogue_host.py uses (a float32 demapper decides as the model does)."""
import numpy as np
import pytest

import _ref_epilogue as E
import _ref_info as I
from conftest import load_golden


def _frame(n, N, seed, nu=0.0):
    rng = np.random.default_rng(seed)
    amp = E.amp_levels(n)
    P = I.pmf(n, nu)
    lev = rng.choice(n, size=(2, 2, N), p=P)
    return amp, P, lev, amp[lev].astype(np.float16)


def _onehot(lev, n):
    q = np.zeros((2, 2, n, lev.shape[-1]))
    np.put_along_axis(q, lev[:, :, None, :], 1.0, axis=2)
    return q.reshape(2, 2 * n, -1)


@pytest.mark.parametrize("n,nu", [(2, 0.0), (4, 0.3), (8, I.NU_SHAPED)])
def test_one_hot_q_reaches_the_entropy(n, nu):
    amp, P, lev, tx = _frame(n, 200, 1, nu)
    m = I.info_q(_onehot(lev, n), tx, P, (0, 0), 0)
    H = I.entropy(P)
    assert np.allclose(m["AIR"], 2 * H, atol=1e-12) and np.allclose(m["GMI"], 2 * H, atol=1e-12)
    assert np.array_equal(m["BER"], [0, 0]) and np.allclose(m["NGMI"], 1.0, atol=1e-12)
    assert np.array_equal(m["sym_err"], [0, 0]) and np.array_equal(m["hyp"], [0, 0]) and np.array_equal(m["kept"], [200 - 22] * 2)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_uniform_q_carries_nothing(n):
    amp, P, lev, tx = _frame(n, 120, 2, 0.1)
    q = np.full((2, 2 * n, 120), 1.0 / n)
    m = I.info_q(q, tx, P, (0, 0), 0)
    H, b = I.entropy(P), np.log2(n)
    assert np.allclose(m["AIR"], 2 * H - 2 * b, atol=1e-12) and np.allclose(m["GMI"], 2 * H - 2 * b, atol=1e-12)
    assert np.allclose(m["NGMI"], 0.0, atol=1e-12)


def test_hand_built_four_level_case():
    """4 levels, labels g = 00, 01, 11, 10.  Kept symbols 11 .. 32 of N = 44; all decided right except, in polarisation 0, symbol 12
    (I: 0 -> 2, labels 00 -> 11: 2 bits), symbol 13 (Q: 1 -> 2, 01 -> 11: 1 bit) and symbol 14 (I: 3 -> 0, 10 -> 00: 1 bit; Q: 2 -> 1,
    11 -> 01: 1 bit), and in polarisation 1 symbol 20 (Q: 0 -> 3, 00 -> 10: 1 bit).  A wrong decision outside the window counts nothing."""
    n, N = 4, 44
    amp = E.amp_levels(n)
    lev = np.zeros((2, 2, N), np.int64)
    lev[0, 0, 12], lev[0, 1, 13], lev[0, 0, 14], lev[0, 1, 14], lev[1, 1, 20] = 0, 1, 3, 2, 0
    lev[:, :, 15:19] = [[[1, 2, 3, 0]], [[3, 1, 0, 2]]]                       # other levels occur too: no other hypothesis can win
    rx = lev.copy()
    rx[0, 0, 12], rx[0, 1, 13], rx[0, 0, 14], rx[0, 1, 14], rx[1, 1, 20] = 2, 2, 0, 1, 3
    rx[1, 0, 5] = 3                                                           # outside the kept window [11, 33)
    q = 0.7 * _onehot(rx, n) + 0.1 * (1 - _onehot(rx, n))                     # 0.7 at the decided level, 0.1 elsewhere
    m = I.info_q(q, amp[lev].astype(np.float16), np.full(4, 0.25), (0, 0), 0)
    assert np.array_equal(m["kept"], [22, 22]) and np.array_equal(m["hyp"], [0, 0])
    assert np.array_equal(m["sym_err"], [3, 1]) and np.array_equal(m["bit_err"], [5, 1])
    assert np.array_equal(m["BER"], np.float32([5, 1]) / np.float32(2 * 2 * 22))
    # AIR: a right axis contributes log2 0.7, a wrong one log2 0.1; 2 H = 4
    assert np.allclose(m["AIR"], [4 + (40 * np.log2(0.7) + 4 * np.log2(0.1)) / 22, 4 + (43 * np.log2(0.7) + np.log2(0.1)) / 22], atol=1e-12)
    # GMI: a bit the decision gets right sees 0.7 + 0.1, a wrong bit 0.1 + 0.1
    assert np.allclose(m["GMI"], [4 + (83 * np.log2(0.8) + 5 * np.log2(0.2)) / 22, 4 + (87 * np.log2(0.8) + np.log2(0.2)) / 22], atol=1e-12)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("hyp", range(8))
def test_planted_hypothesis_is_recovered(n, hyp):
    """tx is transformed so that hypothesis hyp, and no other, reads the untouched q and y as the original frame: the model finds hyp and
    the figures of the untransformed frame."""
    x = I.make_run(seed=50 + n, N=300, n=n, shift=(3, -4), r=0, hyp=0, batch_len=None, nu=0.05, var=(0.004, 0.005), n_err=(3, 5))
    S = n - 1
    lev = E.tx_levels(x["tx"], n)
    tI, tQ = lev[:, 0], lev[:, 1]
    pI, pQf = [(tI, tQ), (S - tI, S - tQ), (S - tQ, tI), (tQ, S - tI)][hyp & 3]  # q'_I[pI] = q_I[tI] and q'_Q[pQf] = q_Q[tQ] under the rotation
    planted = x["amp"][np.stack([pI, S - pQf if hyp >> 2 else pQf], axis=1)].astype(np.float16)
    for f in (lambda tx: I.info_q(x["q"], tx, x["P"], x["shift"], x["r"]),
              lambda tx: I.info_y(x["y"], tx, x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"])):
        m0, m1 = f(x["tx"]), f(planted)
        assert np.array_equal(m0["hyp"], [0, 0]) and np.array_equal(m1["hyp"], [hyp, hyp])
        for k in ("kept", "sym_err", "bit_err"):
            assert np.array_equal(m0[k], m1[k]), k
        assert np.array_equal(m0["sym_err"], [3, 5]) and (m0["bit_err"] >= m0["sym_err"]).all()
        for k in ("AIR", "GMI", "NGMI", "BER"):
            assert np.allclose(m0[k], m1[k], rtol=0, atol=1e-9), k


def test_symbol_errors_are_the_stored_q_ser():
    g = load_golden("G5_dp_epilogue")
    n = int(g["amp_levels"].shape[0])
    m = I.info_q(g["out_train"], g["data"], g["P"], g["shifts"][-1, 0], int(g["rs"][-1, 0]), int(g["B"]))
    ser = m["sym_err"].astype(np.float32) / m["kept"].astype(np.float32)
    assert ser.dtype == np.float32 and np.array_equal(ser, g["SER_valid"][2:4, -1])
    assert m["sym_err"].min() > 0 and (m["bit_err"] >= m["sym_err"]).all() and n == 8
    assert (5.5 < m["GMI"]).all() and (m["GMI"] < 6).all() and (5.5 < m["AIR"]).all() and (m["AIR"] < 6).all()   # uniform 64-QAM at 23 dB, converged
    assert m["min_post"] >= I.MIN_POST_FLOOR or m["min_post"] == 0.0          # (a converged frame: a stored q may underflow to exactly 0)


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_gpu_cases_meet_their_preconditions(name):
    xs, mq, my = I.build_launch(name)
    for x, a, b in zip(xs, mq, my):
        assert np.array_equal(a["kept"], b["kept"])
        if a["kept"][0] == 0:
            assert np.isnan(a["AIR"]).all() and np.isnan(b["GMI"]).all() and not a["sym_err"].any() and not b["bit_err"].any()
            continue
        assert a["min_post"] >= I.MIN_POST_FLOOR                              # float32 and float64 logs agree
        assert a["qgap"] > E.QGAP_FLOOR and b["qgap"] > E.QGAP_FLOOR          # the decisions do not hang on a rounding
        assert np.array_equal(a["hyp"], [x["hyp"]] * 2) and np.array_equal(b["hyp"], [x["hyp"]] * 2)
        assert np.array_equal(a["sym_err"], b["sym_err"]) and np.array_equal(a["bit_err"], b["bit_err"])


def test_underflow_case_precondition():
    """The underflow case of the GPU suite: a q of exactly 0 at a transmitted level costs log2(FLT_MIN) = -126 bit in q-mode."""
    x = I.make_run(seed=7, N=300, n=8, shift=(0, 0), r=0, hyp=0, batch_len=None, nu=0.0, var=(0.004, 0.004), n_err=(0, 0))
    q = x["q"].copy()
    lev = E.tx_levels(x["tx"], 8)
    t = int(lev[0, 0, 100])
    was = float(q[0, t, 100])
    q[0, t, 100] = 0.0
    m0, m1 = I.info_q(x["q"], x["tx"], x["P"], x["shift"], 0), I.info_q(q, x["tx"], x["P"], x["shift"], 0)
    K = m0["kept"][0]
    assert m1["min_post"] == 0.0
    assert np.isclose(m1["AIR"][0] - m0["AIR"][0], (-126 - np.log2(was)) / K, atol=1e-12)
    assert np.isfinite(I.info_y(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], 0)["GMI"]).all()


def test_float32_cost_of_y_mode_is_what_the_gpu_bound_is_built_on():
    """tests/test_epilogue_info_gpu.py holds y-mode to three times Y_DEV.  The largest deviation of the kernel's operation order in numpy
    float32 from the float64 model over the GPU cases is 1.27e-5 bit: the exponent of a wrong symbol has a magnitude of hundreds and carries
    the float32 rounding of that, divided by a kept count as small as 11."""
    worst = max(d for name in I.LAUNCHES for d in map(I.y_mode_float32_deviation, I.build_launch(name)[0]) if d is not None)
    print(f"y-mode in float32, largest deviation from the model: {worst:.3e} bit")
    assert worst <= I.Y_DEV

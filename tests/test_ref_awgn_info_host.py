"""The float64 model of the AWGN information-rate figures (tests/_ref_awgn_info.py) against closed forms that do not go through
tests/_ref_info.py, the window arithmetic against the reference's own Python slices, and the preconditions the GPU cases of
tests/test_awgn_info_gpu.py rely on: a decision margin of the whole normalised row, posteriors at the transmitted level >= 1e-30, a top-two
posterior gap, and the planted hypothesis and error count recovered wherever at least 11 symbols are kept."""
import numpy as np
import pytest

import _ref_awgn_info as A


def _frame(n, N, seed, nu=0.0):
    rng = np.random.default_rng(seed)
    amp, P = A.amp_levels(n), A.pmf(n, nu)
    lev = rng.choice(n, size=(2, N), p=P)
    return amp, P, lev, amp[lev].astype(np.float16)


def _onehot(lev, n):
    q = np.zeros((2, n, lev.shape[-1]))
    np.put_along_axis(q, lev[:, None, :], 1.0, axis=1)
    return q.reshape(2 * n, -1)


@pytest.mark.parametrize("n,nu", [(2, 0.0), (4, 0.3), (8, A.NU_SHAPED)])
def test_one_hot_q_reaches_the_entropy(n, nu):
    amp, P, lev, tx = _frame(n, 200, 1, nu)
    m = A.info_q(_onehot(lev, n), tx, P, 0)
    H = A.entropy(P)
    assert abs(m["AIR"] - 2 * H) <= 1e-12 and abs(m["GMI"] - 2 * H) <= 1e-12 and abs(m["NGMI"] - 1.0) <= 1e-12
    assert m["BER"] == 0 and m["sym_err"] == 0 and m["bit_err"] == 0 and m["hyp"] == 0 and m["kept"] == 200 - 22


@pytest.mark.parametrize("n", [2, 4, 8])
def test_uniform_q_carries_nothing(n):
    amp, P, lev, tx = _frame(n, 120, 2, 0.1)
    m = A.info_q(np.full((2 * n, 120), 1.0 / n), tx, P, 3)
    H, b = A.entropy(P), np.log2(n)
    assert abs(m["AIR"] - (2 * H - 2 * b)) <= 1e-12 and abs(m["GMI"] - (2 * H - 2 * b)) <= 1e-12 and abs(m["NGMI"]) <= 1e-12
    assert m["kept"] == 120 - 22 - 3


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("mode", ["q", "y"])
def test_one_adjacent_single_axis_error_is_one_bit(n, mode):
    """Adjacent Gray labels differ in one bit: one planted error of one axis to the neighbouring level is one symbol error and one bit error."""
    amp, P, lev, tx = _frame(n, 80, 3)
    rx = lev.copy()
    rx[1, 40] += 1 if rx[1, 40] < n - 1 else -1
    if mode == "q":
        m = A.info_q(0.9 * _onehot(rx, n) + 0.1 / n, tx, P, 0)
    else:
        P_amp = float((P * np.abs(amp.astype(np.float64))).sum())
        a = amp[rx].astype(np.float64)
        y = a * (1.3 * P_amp / np.abs(a).mean(1))[:, None]                    # mean|y_c| = 1.3 amp_mean: the normalisation returns the levels
        m = A.info_y(y.astype(np.float32), tx, P, amp, P_amp, 0.005, 0)
    assert (m["kept"], m["hyp"], m["sym_err"], m["bit_err"]) == (58, 0, 1, 1)
    assert m["BER"] == float(np.float32(1) / np.float32(2 * np.log2(n) * 58))


@pytest.mark.parametrize("N", [23, 24, 40, 257])
def test_window_is_the_reference_slices(N):
    """SER_q(q[:, 11+sh:-11], data[:, 11:-11-sh]) (func_VAELE_MQAM_shaping.py:318): where both slices hold the same, positive number of symbols
    the window is those; everywhere else (sh <= -11: data[:, 11:-11-sh] ends before it starts or q[:, 11+sh:-11] starts behind its end; len <= 0)
    it is empty."""
    idx = np.arange(N)
    for sh in range(-12, 13):
        qs, ds = idx[11 + sh:-11], idx[11:-11 - sh]
        ri, ti = A.window(N, sh)
        if sh <= -11 or N - 22 - sh <= 0:
            assert len(ri) == 0 and len(ti) == 0, (N, sh)
            assert len(ds) == 0 or len(qs) == 0 or sh <= -11
        else:
            assert np.array_equal(ri, qs) and np.array_equal(ti, ds), (N, sh)
            assert ri.min() >= 0 and ri.max() < N and ti.max() < N


def test_no_int32_shift_leaves_the_row():
    for N in (1, 22, 23, 1000):
        for sh in (-2 ** 31, -2 ** 31 + 1, -12, -11, -10, N - 23, N - 22, 2 ** 31 - 1):
            ri, ti = A.window(N, sh)
            assert len(ri) == len(ti) and (len(ri) == 0 or (0 <= ri.min() and ri.max() < N and 0 <= ti.min() and ti.max() < N))


@pytest.mark.parametrize("hyp", range(4))
def test_planted_hypothesis_is_recovered_with_the_same_figures(hyp):
    """tx is transformed so that hypothesis hyp, and no other, reads the untouched q and y as the original frame: the model finds hyp and the
    figures of the untransformed frame, in both modes."""
    x = A.make_run(seed=77, N=300, n=8, shift=4, hyp=0, nu=0.05, var=0.0063, n_err=4)
    S = 7
    tI, tQ = A.tx_levels(x["tx"], 8)
    pI, pQ = [(tI, tQ), (S - tI, S - tQ), (S - tQ, tI), (tQ, S - tI)][hyp]     # q'_I[pI] = q_I[tI] and q'_Q[pQ] = q_Q[tQ] under the rotation
    planted = x["amp"][np.stack([pI, pQ])].astype(np.float16)
    for f in (lambda tx: A.info_q(x["q"], tx, x["P"], x["shift"]), lambda tx: A.info_y(x["y"], tx, x["P"], x["amp"], x["amp_mean"], x["var"], x["shift"])):
        m0, m1 = f(x["tx"]), f(planted)
        assert m0["hyp"] == 0 and m1["hyp"] == hyp and m0["kept"] == m1["kept"] == 300 - 22 - 4
        assert m0["sym_err"] == m1["sym_err"] == 4 and m0["bit_err"] == m1["bit_err"] >= 4
        for k in ("AIR", "GMI", "NGMI", "BER"):
            assert abs(m0[k] - m1[k]) <= 1e-9, k


def test_zero_component_has_no_normalisation():
    x = A.make_run(seed=5, N=60, n=4, shift=0, hyp=0, nu=0.0, var=0.01, n_err=0)
    y = x["y"].copy()
    y[1] = 0
    m = A.info_y(y, x["tx"], x["P"], x["amp"], x["amp_mean"], x["var"], 0)
    assert np.isnan(m["GMI"]) and np.isnan(m["AIR"]) and np.isnan(m["BER"]) and (m["kept"], m["sym_err"], m["bit_err"], m["hyp"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_gpu_cases_meet_their_preconditions(name):
    xs, mq, my = A.build_launch(name)
    N = xs[0]["y"].shape[-1]
    assert [x["shift"] for x in xs] == [-10, 0, 10]
    for x, a, b in zip(xs, mq, my):
        assert a["kept"] == b["kept"] == max(N - 22 - x["shift"], 0)
        assert b["margin"] >= 0.05                                            # the whole row: the validation kernel decides on all of it
        if a["kept"] == 0:
            assert np.isnan(a["AIR"]) and np.isnan(b["GMI"]) and a["sym_err"] == 0 and b["bit_err"] == 0
            continue
        assert a["min_post"] >= 1e-30                                         # float32 and float64 logs agree
        assert a["qgap"] > 0.05 and b["qgap"] > 0.05                          # the decisions do not hang on a rounding
        assert a["sym_err"] == b["sym_err"] and a["bit_err"] == b["bit_err"] and a["hyp"] == b["hyp"]
        if a["kept"] >= 11:
            assert a["hyp"] == x["hyp"] and a["sym_err"] == x["n_err"]
    assert {x["n"] for x in xs} == {xs[0]["n"]}


def test_launches_cover_what_they_are_meant_to():
    L = A.launches()
    assert len(L) == 21 and {s["N"] for v in L.values() for s in v} == {23, 24, 33, 60, 257, 1030, 2100}
    assert {s["hyp"] for v in L.values() for s in v} == {0, 1, 2, 3} and {s["nu"] for v in L.values() for s in v} == {0.0, A.NU_SHAPED}
    assert {s["var"] for v in L.values() for s in v} == {0.004, 0.0063, 0.01}
    kept = {name: [m["kept"] for m in A.build_launch(name)[1]] for name in ("N23-n8", "N33-n4", "N257-n2")}
    assert kept == {"N23-n8": [11, 1, 0], "N33-n4": [21, 11, 1], "N257-n2": [245, 235, 225]}


def test_float32_cost_of_y_mode_is_what_the_gpu_bound_is_built_on():
    """tests/test_awgn_info_gpu.py holds y-mode to three times Y_DEV: the largest deviation of the kernel's operation order in numpy float32 from
    the float64 model over the GPU cases (1.71e-4 bit, set by two kept symbols that are both wrong by up to three 16-QAM levels: terms of about
    -1300 bit carry the float32 spacing at that magnitude, 1.2e-4)."""
    worst, where = 0.0, None
    for name in A.LAUNCHES:
        xs, _, my = A.build_launch(name)
        for x, b in zip(xs, my):
            d = A.y_mode_float32_deviation(x, b)
            if d is not None and d > worst:
                worst, where = d, (name, x["shift"])
    print(f"y-mode in float32, largest deviation from the model: {worst:.3e} bit at {where}")
    assert worst <= A.Y_DEV

"""The float64 model of the AWGN baselines (tests/_ref_awgn.py) is right, on the CPU: against the vectors captured from the reference (G15,
G16), against the package's torch mirrors on random frames, and against a direct convolution; and every conditioned fixture that
tests/test_awgn_baselines_envelope_gpu.py feeds to the kernels meets its own conditions, so a bad fixture fails here and not as a kernel
failure."""
import numpy as np
import pytest
import torch

import _ref_awgn as ra
from conftest import load_golden, relerr

DFE_CASES = ["G16_dfe_64qam_h1_15dB", "G16_dfe_64qam_h1_22dB", "G16_dfe_16qam_h2_18dB", "G16_dfe_4qam_proakis_a_8dB"]
MARGIN = 1e-3            # of a level spacing: >= 60 x the float32 error of a sliced value (<= 42 roundings of terms below 2 ~ 5e-6; spacing >= 0.31)


def crel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("name", ["G15_awgn_cma_16qam", "G15_awgn_cma_64qam"])
def test_cma_model_against_reference(name):
    g = load_golden(name)
    sps = int(g["sps"])
    out, h, e, loss = ra.awgn_cma(g["rx"], g["h0"], float(g["lr"]), sps, True)
    assert relerr(out, g["out"]) < 1e-5 and relerr(e, g["e"]) < 1e-5 and relerr(h, g["h"]) < 1e-5
    assert abs(loss - np.mean(np.abs(g["e"].astype(np.float64)))) < 1e-5 * loss
    v = ra.validate(g["rx_valid"], g["h_valid"], g["data_valid"], g["amp_levels"], sps, 21)
    assert relerr(v["out"], g["out_valid"]) < 1e-5
    assert relerr(ra.awgn_cma(g["rx_valid"], g["h_valid"], 0.0, sps, False)[2], g["e_valid"]) < 1e-5
    flags = ra.cpe_flags(v["modulus"], v["dist"])
    assert not flags.any()
    assert relerr(v["cpe"], g["cpe"]) < 1e-5
    assert v["shift"] == int(g["shift"])
    K = g["cpe"].shape[1]
    assert v["L"] == K - 22 - v["shift"]
    near = int((v["margin"].min(axis=0) < 1e-5 * (g["amp_levels"][1] - g["amp_levels"][0])).sum())
    assert abs(v["counts"].min() - float(g["SER"]) * v["L"]) <= near + 1e-3, (v["counts"], float(g["SER"]) * v["L"], near)


def test_cpe_model_against_reference():
    g = load_golden("G15_awgn_cma_cpe")
    y, mod, dist = ra.cpe(g["cpe_in"])
    assert not ra.cpe_flags(mod, dist).any()
    assert relerr(y, g["cpe_out"]) < 1e-5


@pytest.mark.parametrize("case", DFE_CASES)
def test_lmmse_and_dfe_model_against_reference(case):
    g = load_golden(case)
    lev, n_cut = g["amp_levels"], int(g["N_cut"])
    d = float(lev[1] - lev[0])
    v = ra.lmmse(g["rx"], g["lmmse"], g["data"], lev, 21, n_cut)
    assert crel(v["out"], g["lmmse_out"]) < 1e-5
    diff = np.nonzero(v["dec"] != g["lmmse_dec"])[0]
    assert np.all(v["dec_margin"][diff] < 1e-5 * d), (diff, v["dec_margin"][diff] / d)
    assert v["shift"] == int(g["lmmse_shift"]) and v["Lr"] == v["L"] + 1
    near = int((v["margin"].min(axis=0) < 1e-5 * d).sum())
    assert abs(v["counts"].min() - float(g["lmmse_SER"]) * v["L"]) <= near + 1e-3
    x = g["rx"].astype(np.float64)
    assert crel(ra.compl_conv(x[0] + 1j * x[1], g["ff"]), g["ff_out"]) < 1e-5
    dec, margin = ra.dfe(g["ff_out"], g["fb"], g["lmmse_dec"], lev)         # the reference's own float32 feed-forward output and start
    assert margin >= 1e-5 * d, margin / d                                   # no sliced value of these four frames is a near-tie
    assert np.array_equal(dec, g["dfe_dec"])
    ev = ra.dfe_eval(g["dfe_dec"], g["data"], lev, 24, n_cut)
    assert ev["shift"] == int(g["dfe_shift"])
    assert abs(ev["counts"].min() - float(g["dfe_SER"]) * ev["L"]) <= 1e-3


# ------------------------------------------------------------------ the package's torch mirrors, on CPU tensors
@pytest.mark.parametrize("seed,n_lev,K", [(1, 2, 1500), (2, 4, 2600), (3, 8, 4000)])
def test_model_against_torch_mirrors(seed, n_lev, K):
    from vae_equalizer_amd import DFE_MQAM_shaping as dm
    from vae_equalizer_amd import func_CMA_MQAM_shaping as cm
    rng = np.random.default_rng(seed)
    lev = ra.qam_levels(n_lev)
    rx, h0 = ra.cma_frame(seed, K, 1, 5, n_lev, drift=2.5)
    y = rx.astype(np.float64)
    yc, mod, dist = ra.cpe(y)
    ok = ~ra.cpe_flags(mod, dist)
    got = cm.CPE(torch.from_numpy(rx)).numpy()
    assert np.max(np.abs(got - yc)[:, ok]) < 2e-5 * np.max(np.abs(yc)) and ok.mean() > 0.99
    iI, iQ = rng.integers(0, n_lev, K), rng.integers(0, n_lev, K)
    data = np.stack([lev[iI], lev[iQ]]).astype(np.float16)
    for lag, rot in ((3, 0), (-5, 1), (0, 2)):
        track = np.roll((1j ** rot) * (lev[iI] + 1j * lev[iQ]), lag) + 0.05 * (rng.standard_normal(K) + 1j * rng.standard_normal(K))
        tr = np.stack([track.real, track.imag]).astype(np.float32)
        for n_shift in (1, 21, 24):
            s, cI, cQ, branch = ra.find_shift(tr[0], data, n_shift, K)
            assert int(cm.find_shift_symb(torch.from_numpy(tr), torch.from_numpy(data), n_shift)) == s, (lag, rot, n_shift, branch)
        s = lag
        a, b = tr[:, 11 + s:K - 11], data[:, 11:K - 11 - s]
        counts, winner, margin, _ = ra.ser(a, b, lev)
        near = int((margin.min(axis=0) < 1e-5).sum())
        for f in (lambda r_, t_: cm.SER_CMA(r_, t_, 1, torch.from_numpy(lev), n_lev), lambda r_, t_: dm.SER_func(r_, t_, torch.from_numpy(lev), n_lev)):
            got = float(f(torch.from_numpy(a.copy()), torch.from_numpy(b)))
            assert abs(got * b.shape[1] - counts.min()) <= near + 1e-2, (lag, rot, got * b.shape[1], counts)
        a1 = tr[:, 11 + s:K - 10]                                           # one sample longer than the data: it enters the scale
        c1 = ra.ser(a1, b, lev)[0]
        got = float(dm.SER_func(torch.from_numpy(a1.copy()), torch.from_numpy(b), torch.from_numpy(lev), n_lev))
        assert abs(got * b.shape[1] - c1.min()) <= near + 1e-2, (lag, rot, got * b.shape[1], c1)
    for Kt in (1, 2, 11, 20, 64):
        taps = (rng.standard_normal(Kt) + 1j * rng.standard_normal(Kt)).astype(np.complex64)
        x = (rx[0] + 1j * rx[1]).astype(np.complex64)
        want = ra.compl_conv(x, taps)
        got = dm.compl_conv(torch.from_numpy(x), torch.from_numpy(taps)).numpy().reshape(-1)
        assert got.shape == want.shape == (K + 2 * (Kt // 2) - Kt + 1,) and crel(got, want) < 1e-5
    q = dm.qam_constants({2: "4-QAM", 4: "16-QAM", 8: "64-QAM"}[n_lev])
    pts = torch.from_numpy((rx[0] + 1j * rx[1]).astype(np.complex64))
    nn = dm.nearest_neighbor(pts, q["const_torch"]).numpy()
    dI, mI = ra.slice_axis(y[0], lev)
    dQ, mQ = ra.slice_axis(y[1], lev)
    far = np.minimum(mI, mQ) > 1e-5
    assert np.array_equal(nn[far], (dI * n_lev + dQ)[far])


# ------------------------------------------------------------------ the conditioned fixtures meet their own conditions
def _check_eval(v, lev, length, want_shift, want_count, want_branch, tag):
    d = float(lev[1] - lev[0])
    assert v["shift"] == want_shift, (tag, v["shift"], want_shift)
    assert v["branch"] == want_branch, (tag, v["branch"], want_branch)
    ratio, off = ra.shift_conditions(v["cI"], v["cQ"], v["branch"], length)
    assert ratio >= 1.5 and off >= 0.02, (tag, ratio, off)
    assert v["margin"].min() >= MARGIN * d, (tag, v["margin"].min() / d)
    assert v["counts"].min() == want_count and sorted(v["counts"])[1] > 10 * max(want_count, 1), (tag, v["counts"], want_count)


def test_validator_fixtures_are_conditioned():
    winners, branches, lags = set(), set(), {}
    for b in ra.validator_cases():
        for fr, r, br in zip(ra.build_validator_batch(b), b["runs"], b["branches"]):
            v = fr["model"]
            _check_eval(v, fr["levels"], b["K"], r["lag"], r["n_err"], br, (b["K"], r))
            assert r["n_err"] > 0
            assert ra.cpe_flags(v["modulus"], v["dist"]).mean() <= 0.005
            winners.add((b["n_lev"], v["winner"]))
            branches.add(v["branch"])
            lags.setdefault(b["n_shift"], set()).add(v["shift"])
    assert {w for _, w in winners} == {0, 1, 2, 3} and {n for n, _ in winners} == {2, 4, 8}
    assert branches == {"I", "Q", "I kept"}
    assert lags[21] == set(range(-10, 11)) and lags[23] == set(range(-10, 12)) and lags[1] == {0}


def test_validator_model_raises_where_the_reference_slice_is_empty():
    fr = ra.conditioned_eval_frame(5, 4001, 4, 0, -11, 2, validator=(1, 3, 0.0))
    with pytest.raises(ValueError, match="empty"):
        ra.validate(fr["rx"], fr["h"], fr["data"], fr["levels"], 1, 23)


def test_lmmse_fixtures_are_conditioned():
    winners = set()
    for case in ra.lmmse_cases():
        K, N, n_cut, n_shift, n_lev = case
        for r in range(3):
            fr, lag = ra.build_lmmse_case(case, r)
            v = ra.lmmse(fr["rx"], fr["taps"], fr["data"], fr["levels"], n_shift, n_cut)
            _check_eval(v, fr["levels"], N + 1, lag, 4 + r, v["branch"], (case, r))
            assert v["dec_margin"].min() >= MARGIN * float(fr["levels"][1] - fr["levels"][0])
            assert v["Lr"] == v["L"] + 1
            winners.add(v["winner"])
    assert winners == {0, 1, 2, 3}


def test_longer_slice_fixture_turns_on_the_extra_sample():
    fr = ra.longer_slice_frame()
    lev = fr["levels"]
    d = float(lev[1] - lev[0])
    v = ra.lmmse(fr["rx"], fr["taps"], fr["data"], lev, 21, 20)
    _check_eval(v, lev, 1101, 3, 3, "I", "longer slice")
    r0 = 20 + 11 + 3
    tr = np.stack([v["out"].real, v["out"].imag])[:, r0:r0 + v["Lr"]]
    tx = fr["data"].astype(np.float64)[:, 31:31 + v["L"]]
    with_, without = ra.ser(tr, tx, lev), ra.ser(tr[:, :v["L"]], tx, lev)
    assert np.array_equal(with_[0], v["counts"]) and without[0].min() == 4 and without[2].min() >= MARGIN * d
    changed = np.nonzero(np.any(with_[3] != without[3], axis=0))[0]
    assert list(changed) == [fr["pulled"]]


def test_dfe_fixtures_are_conditioned():
    for n_lev, K2, N, outliers, chunkings in ra.dfe_cases():
        assert N < 10 ** 5
        for seed in ra.dfe_run_seeds(n_lev, K2, N):
            fr = ra.conditioned_dfe_frame(seed, N, n_lev, K2, outliers)
            d = float(fr["levels"][1] - fr["levels"][0])
            dec, margin = ra.dfe(fr["ff"], fr["fb"], fr["init"], fr["levels"])
            assert margin >= MARGIN * d and np.array_equal(dec, fr["expected"])
            sym = np.rint((n_lev - 1) / 2 * fr["data"].astype(np.float64) + (n_lev - 1) / 2).astype(np.int64)
            assert int(np.any(np.stack([dec // n_lev, dec % n_lev]) != sym, axis=0).sum()) == outliers > 0
            assert np.max(np.abs(np.concatenate([fr["ff"].real, fr["ff"].imag]))) < 8 and np.abs(fr["fb"]).max() < 0.5
            if (7, 0) in chunkings:                                         # seven chunks, no warm-up: some chunk starts from a wrong state
                CH = -(-(N - K2) // 7)
                starts = [K2 + c * CH for c in range(1, 7)]
                assert any(np.any(fr["init"][s - K2:s] != dec[s - K2:s]) for s in starts)
        for C, W in chunkings:                                              # legal for the kernel: C <= N - K2, CH >= K2, C <= 8192
            CH = -(-(N - K2) // C)
            assert 1 <= C <= min(8192, N - K2) and (C == 1 or CH >= K2) and W >= 0
    for n_lev, K2, N, outliers, _ in ra.dfe_cases()[:12]:
        fr = ra.conditioned_dfe_frame(100 * n_lev + K2, 1200, n_lev, K2, 7)
        for n_shift, n_cut, lag in ((1, 0, 0), (1, 20, 0), (24, 20, -12), (24, 20, 11), (24, 20, 5)):
            ev = ra.dfe_eval(fr["expected"], ra.shifted_data(fr["data"], lag, K2), fr["levels"], n_shift, n_cut)
            assert ev["shift"] == lag and ev["branch"] == "I", (n_lev, K2, n_shift, lag, ev["shift"])
            ratio, off = ra.shift_conditions(ev["cI"], ev["cQ"], "I", 1200)
            assert ratio >= 1.5 and off >= 0.02
            assert ev["margin"].min() >= MARGIN * float(fr["levels"][1] - fr["levels"][0]) and 0 < ev["counts"].min() <= 7


# ------------------------------------------------------------------ the index map
def test_symbol_index_map_is_a_permutation_and_lr0_is_a_convolution():
    for sps in (1, 2, 3, 4):
        for M in (1, 3, 31, 33, 63):
            K = 2 * M + 5
            kk = ra.cma_symbol_indices(K * sps, sps, M)
            assert sorted(kk) == list(range(K)), (sps, M)
            mh = M // 2
            joff = mh - mh // sps
            assert np.array_equal(kk, (np.arange(K) - joff) % K)
            rx, h0 = ra.cma_frame(10 * M + sps, K * sps, sps, M)
            out, h, e, loss = ra.awgn_cma(rx, h0, 0.0, sps, True)
            x = rx[0].astype(np.float64) + 1j * rx[1].astype(np.float64)
            hc = h0[0].astype(np.float64) + 1j * h0[1].astype(np.float64)
            full = np.convolve(x, hc[::-1])                                 # full[n] = sum_t x[n - (M-1) + t] h[t]
            sym = full[mh + sps * np.arange(K)]                             # symbol j: window starting at sample sps j - mh
            assert np.array_equal(h, h0.astype(np.float64))
            assert np.max(np.abs((out[0] + 1j * out[1])[kk] - sym)) < 1e-12
            assert np.max(np.abs(e[kk] - (1 - np.abs(sym) ** 2))) < 1e-12 and abs(loss - np.mean(np.abs(e))) < 1e-12

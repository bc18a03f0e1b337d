"""The AWGN baselines over their envelope, against the float64 model of tests/_ref_awgn.py: vaeq_awgn_cma (both <HALF> instantiations, 1 to 8
samples per symbol, frames from K = M up, both sides of the look-ahead and of the 64-symbol flush), vaeq_awgn_cma_validate (both <LDS> forms,
the chunk rule, the LDS ceiling, every lag and branch of the shift search, the four relabelings, exact error counts), vaeq_awgn_lmmse_eval
(the one-sample-longer slice) and vaeq_awgn_dfe (every <NL, K2M> instantiation, chunkings up to the cap, warm-ups longer than a chunk).

Decisions, shifts, error counts and untouched taps are exact: tests/test_ref_awgn_host.py shows that every conditioned fixture used here keeps
1e-3 of a level spacing between any sliced value and a decision boundary.  The real-valued outputs are held to BOUND, see there."""
import numpy as np
import pytest
import torch

import _ref_awgn as ra
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CMA_KERNELS = {True: "vaeq::awgn_cma_kernel<true>", False: "vaeq::awgn_cma_kernel<false>"}
VAL_KERNELS = {True: "vaeq::awgn_cma_validate_kernel<true>", False: "vaeq::awgn_cma_validate_kernel<false>"}
# relerr(kernel, float64 model) = max |a - b| / max |b| per group: four times the maximum measured on one MI355X (the measured value
# beside each bound), rounded down to three digits.
BOUND = {
    "cma lr0 out": 1.08e-6,         # 2.717e-07
    "cma lr0 e": 1.94e-5,           # 4.871e-06 (e = R - |out|^2 is a difference of O(1) terms, relative to the largest |e| of the frame)
    "cma train out": 5.40e-6,       # 1.351e-06
    "cma train e": 2.67e-5,         # 6.685e-06
    "cma train h": 2.74e-6,         # 6.873e-07
    "cma train loss": 1.30e-5,      # 3.267e-06
    "validate cpe lds": 1.58e-6,    # 3.962e-07
    "validate cpe global": 1.10e-6,  # 2.757e-07
    "lmmse out": 4.64e-7,           # 1.161e-07
    "dfe ff": 9.86e-7,              # 2.465e-07
}
STATS = {}


def _note(key, value):
    STATS[key] = max(STATS.get(key, 0.0), float(value))
    return float(value) <= BOUND[key]


def _hold(ok, *tag):
    """Asserted once per test, after every figure of it went into STATS, so that a run reports the whole maximum."""
    assert all(ok), (tag, {k: (STATS[k], BOUND[k]) for k in STATS if STATS[k] > BOUND[k]})


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(STATS):
        print(f"  measured max {k}: {STATS[k]:.4g} (bound {BOUND[k]:.3g})")


def crel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_cma(frames, lr, sps, update, Rc=1.0, want_out=True, want_e=True):
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import awgn_cma
    rx, h = t(np.stack([f[0] for f in frames])), t(np.stack([f[1] for f in frames]))
    lr_t = torch.tensor(np.broadcast_to(np.asarray(lr, np.float32), (len(frames),)).copy(), device=DEV)
    loss, out, e = awgn_cma(rx, h, lr_t, sps, update, Rc, want_out=want_out, want_e=want_e)
    torch.cuda.synchronize()
    name = nat.last_kernel()
    return loss.cpu().numpy(), None if out is None else out.cpu().numpy(), None if e is None else e.cpu().numpy(), h.cpu().numpy(), name


# ------------------------------------------------------------------ vaeq_awgn_cma: FIR and index map
@pytest.mark.parametrize("update", [1, 0])
def test_cma_fir_and_index_over_the_grid(update):
    """lr = 0 with the update on (the rank-1 update runs with a zero step: an added 0 * NaN would show) and update = 0, over the whole
    (M, sps, K) grid with 1 to 5 distinct runs per call: h comes back bit for bit, out and e land where the model puts them."""
    seen, ok = set(), []
    for i, (M, sps, K) in enumerate(ra.cma_grid()):
        frames = [ra.cma_frame(7000 + 10 * i + r, K * sps, sps, M) for r in range(1 + i % 5)]
        loss, out, e, h, name = run_cma(frames, 0.0 if update else 1e-2, sps, update)
        seen.add(name)
        assert name == CMA_KERNELS[M <= 31]
        for r, (rx, h0) in enumerate(frames):
            ro, rh, re_, rl = ra.awgn_cma(rx, h0, 0.0, sps, False)
            assert np.array_equal(h[r], h0), (M, sps, K, r)
            ok += [_note("cma lr0 out", relerr(out[r], ro)), _note("cma lr0 e", relerr(e[r], re_))]
            # a float32 running sum of K terms: K 2^-24 relative at worst, on top of the error of the terms
            assert abs(loss[r] - rl) <= (K * 2.0 ** -24 + BOUND["cma lr0 e"]) * max(rl, np.max(np.abs(re_))), (M, sps, K, r, loss[r], rl)
    _hold(ok, "lr0 grid")
    assert seen == set(CMA_KERNELS.values())


TRAIN = [  # M, sps, K, R_mod, lr
    (31, 1, 1000, 1.0, 4e-4), (29, 2, 2000, 1.32, 3e-4), (3, 3, 777, 1.0, 1e-3), (1, 2, 500, 1.32, 1e-3),
    (33, 1, 1000, 1.32, 3e-4), (33, 2, 2000, 1.0, 3e-4), (63, 3, 1500, 1.0, 2e-4), (61, 2, 129, 1.32, 3e-4),
]


@pytest.mark.parametrize("M,sps,K,Rc,lr", TRAIN)
def test_cma_training_against_float64(M, sps, K, Rc, lr):
    """Three runs with their own frames, taps and step sizes in one call; each instantiation at 1, 2 and 3 samples per symbol."""
    frames = [ra.cma_frame(100 * M + sps + r, K * sps, sps, M, n_lev=2 + 2 * (r % 2)) for r in range(3)]
    lrs = [lr * (1 + 0.5 * r) for r in range(3)]
    loss, out, e, h, name = run_cma(frames, lrs, sps, 1, Rc)
    assert name == CMA_KERNELS[M <= 31]
    for r, (rx, h0) in enumerate(frames):
        ro, rh, re_, rl = ra.awgn_cma(rx, h0, lrs[r], sps, True, Rc)
        assert np.abs(rh - h0).max() > 1e-3 and np.all(np.isfinite(rh)) and np.abs(rh).max() < 3
        _hold([_note("cma train out", relerr(out[r], ro)), _note("cma train e", relerr(e[r], re_)), _note("cma train h", relerr(h[r], rh)),
               _note("cma train loss", abs(loss[r] - rl) / rl)], M, sps, K, r)


@pytest.mark.parametrize("M,sps,K", [(31, 2, 300), (33, 3, 129), (63, 1, 65)])
def test_cma_null_outputs_and_batch_independence(M, sps, K):
    frames = [ra.cma_frame(300 + r, K * sps, sps, M) for r in range(5)]
    lrs = [2e-4 * (1 + r) for r in range(5)]
    loss, out, e, h, _ = run_cma(frames, lrs, sps, 1)
    l1, o1, e1, h1, _ = run_cma(frames, lrs, sps, 1, want_out=False)
    l2, o2, e2, h2, _ = run_cma(frames, lrs, sps, 1, want_e=False)
    assert o1 is None and np.array_equal(e1, e) and np.array_equal(h1, h) and np.array_equal(l1, loss)
    assert e2 is None and np.array_equal(o2, out) and np.array_equal(h2, h) and np.array_equal(l2, loss)
    for r in (0, 3, 4):
        ls, os_, es, hs, _ = run_cma([frames[r]], lrs[r], sps, 1)
        assert np.array_equal(os_[0], out[r]) and np.array_equal(es[0], e[r]) and np.array_equal(hs[0], h[r]) and ls[0] == loss[r]


# ------------------------------------------------------------------ vaeq_awgn_cma_validate
def run_validate(rx, h, data, lev, sps, n_shift):
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import awgn_cma_validate
    ser, shift, cpe = awgn_cma_validate(t(rx), t(h), t(data), t(lev), sps, n_shift, want_cpe=True)
    torch.cuda.synchronize()
    return ser.cpu().numpy(), shift.cpu().numpy(), cpe.cpu().numpy(), nat.last_kernel()


def _track_err(got, rx, h0, sps):
    """relerr of a phase-corrected track [2,K] against the model's, the four quarter turns accepted at the symbols the model flags (at most
    0.5 % of them) -> (error, model track, model CMA output)."""
    out, _, _, _ = ra.awgn_cma(rx, h0, 0.0, sps, False)
    y, mod, dist = ra.cpe(out)
    flag = ra.cpe_flags(mod, dist)
    assert flag.sum() <= 0.005 * y.shape[1]
    yc, gc = y[0] + 1j * y[1], got[0].astype(np.float64) + 1j * got[1]
    err = np.abs(gc - yc)
    err[flag] = np.min([np.abs(gc[flag] - yc[flag] * 1j ** q) for q in range(4)], axis=0)
    return err.max() / np.abs(yc).max(), y, out


TRACKS = [  # K, sps, M, n_shift: the chunk rule ((K + 1023) / 1024) | 1 gives 1, 1, 3, 3, 3, 3, 5, 17, 19 (global), 27
    (1021, 2, 31, 21), (1024, 1, 63, 21), (1025, 3, 1, 23), (2047, 2, 33, 1), (2048, 3, 31, 21), (2049, 1, 33, 23), (5000, 2, 63, 21),
    (17408, 1, 31, 21), (17409, 1, 33, 21), (26000, 2, 1, 21),
]


@pytest.mark.parametrize("K,sps,M,n_shift", TRACKS)
def test_validate_track_against_float64(K, sps, M, n_shift):
    """The phase-corrected track of two runs (one with a carrier drift of 2.5 rad across the frame: the correction jumps by pi/2, not
    unwrapped) against the model.  Where the model flags the averaged phasor as within 1e-3 rad of the cut of atan2 (or as cancelled), the
    kernel may have taken either side: the model value times 1, j, -1 or -j is accepted there."""
    rng = np.random.default_rng(K + M)
    frames = [ra.cma_frame(K + r, K * sps, sps, M, n_lev=4, drift=2.5 * r, noise=0.03) for r in range(2)]
    for rx, h0 in frames:
        h0 += (0.03 * rng.standard_normal(h0.shape)).astype(np.float32)
    lev = ra.qam_levels(4)
    data = lev[rng.integers(0, 4, (2, 2, K))].astype(np.float16)
    ser, shift, cpe, name = run_validate(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), data, lev, sps, n_shift)
    assert name == VAL_KERNELS[K <= 17408]
    key = "validate cpe lds" if K <= 17408 else "validate cpe global"
    for r, (rx, h0) in enumerate(frames):
        err, y, out = _track_err(cpe[r], rx, h0, sps)
        if r == 1:
            phi = np.angle((y[0] + 1j * y[1]) * (out[0] - 1j * out[1]))
            assert np.abs(np.diff(phi)).max() > 1.0                            # the correction did jump by pi/2
        _hold([_note(key, err)], K, sps, M, r)
    assert np.all((ser >= 0) & (ser <= 1)) and np.all(np.abs(shift) <= n_shift // 2)


@pytest.mark.parametrize("K,p", [(2000, 778), (17500, 319)])
def test_validate_chunk_rule_restarts_the_window_sum(K, p):
    """The chunk length ((K + 1023) / 1024) | 1, the one thing that shows which symbols open a chunk: a thread sums the 501-symbol window of
    its chunk's first symbol afresh and slides it along the chunk.  One sample of modulus 300 at p has a 4th power of 8e9, whose float32 ulp
    (512) swallows the other 500 terms of a window, so a window sum that the outlier LEAVES by the sliding subtraction is void, while one
    summed afresh behind it is as good as any.  The outlier leaves the window in front of symbol p + 251, and p is chosen so that p + 251 is
    a multiple of the chunk length (3 at K = 2000 in LDS, 19 at K = 17 500 in the global workspace) and of no shorter one: every window is then
    either summed afresh or still holds the outlier, and the whole track keeps the bound of its group.  With any other chunk length
    (2 or 18 without the `| 1`) symbol p + 251 gets a void phase."""
    chunk = ((K + 1023) // 1024) | 1
    assert (p + 251) % chunk == 0 and (p + 251) % (chunk - 1) != 0
    rx, h0 = ra.cma_frame(K + p, K, 1, 1, n_lev=2)
    rx[:, p] = 300 * np.cos(np.pi / 8), 300 * np.sin(np.pi / 8)                # 4th power 8.1e9 j: a quarter turn away from the cut of atan2
    lev = ra.qam_levels(2)
    data = lev[np.random.default_rng(p).integers(0, 2, (1, 2, K))].astype(np.float16)
    ser, shift, cpe, name = run_validate(rx[None], h0[None], data, lev, 1, 21)
    assert name == VAL_KERNELS[K <= 17408]
    err, y, out = _track_err(cpe[0], rx, h0, 1)
    _hold([_note("validate cpe lds" if K <= 17408 else "validate cpe global", err)], K, p)


def test_validate_shift_and_error_counts_on_conditioned_frames():
    """Every lag of n_shift = 21 and 23 (but -11), n_shift = 1, the four relabelings as winners, the I-rail, Q-rail and "I kept" branches of
    the shift search (K = 26 000: 0.02 K is above any 990-symbol correlation), n_lev 2 / 4 / 8: shifts and error COUNTS exactly.  The kernel
    reports neither the winning relabeling nor the branch: those two sets come from the float64 model, whose shift and count the kernel must
    equal (tests/test_ref_awgn_host.py: the runner-up relabeling has over ten times the errors, and every branch decides by 2 % or more)."""
    winners, branches, kernels = set(), set(), set()
    for b in ra.validator_cases():
        frames = ra.build_validator_batch(b)
        ser, shift, cpe, name = run_validate(np.stack([f["rx"] for f in frames]), np.stack([f["h"] for f in frames]),
                                             np.stack([f["data"] for f in frames]), frames[0]["levels"], b["sps"], b["n_shift"])
        kernels.add(name)
        for r, fr in enumerate(frames):
            v = fr["model"]
            assert shift[r] == v["shift"] == b["runs"][r]["lag"], (b["K"], r, shift[r], v["shift"])
            cnt = float(ser[r]) * v["L"]
            assert abs(cnt - round(cnt)) < 1e-2 and round(cnt) == v["counts"].min() > 0, (b["K"], r, cnt, v["counts"])
            winners.add(v["winner"])
            branches.add(v["branch"])
    assert winners == {0, 1, 2, 3} and branches == {"I", "Q", "I kept"} and kernels == set(VAL_KERNELS.values())


# ------------------------------------------------------------------ vaeq_awgn_lmmse_eval
def run_lmmse(frames, n_shift, n_cut, want_out):
    from vae_equalizer_amd.engine import awgn_lmmse_eval
    ser, shift, dec, out = awgn_lmmse_eval(t(np.stack([f["rx"] for f in frames])), torch.from_numpy(np.stack([f["taps"] for f in frames])),
                                           t(np.stack([f["data"] for f in frames])), frames[0]["levels"], n_shift, n_cut, want_out=want_out)
    torch.cuda.synchronize()
    return ser.cpu().numpy(), shift.cpu().numpy(), dec.cpu().numpy(), None if out is None else out.cpu().numpy()


@pytest.mark.parametrize("case", ra.lmmse_cases())
def test_lmmse_against_float64(case):
    """Three frames with their own taps, rotation and lag per call: the output, the decisions of out[1:], the shift and the error count."""
    K, N, n_cut, n_shift, n_lev = case
    frames = [ra.build_lmmse_case(case, r)[0] for r in range(3)]
    ser, shift, dec, out = run_lmmse(frames, n_shift, n_cut, True)
    ser2, shift2, dec2, out2 = run_lmmse(frames, n_shift, n_cut, False)
    assert out2 is None and np.array_equal(ser, ser2) and np.array_equal(shift, shift2) and np.array_equal(dec, dec2)
    for r, fr in enumerate(frames):
        v = ra.lmmse(fr["rx"], fr["taps"], fr["data"], fr["levels"], n_shift, n_cut)
        _hold([_note("lmmse out", crel(out[r], v["out"]))], case, r)
        assert np.array_equal(dec[r].astype(np.int64), v["dec"]), (case, r)
        assert shift[r] == v["shift"], (case, r, shift[r], v["shift"])
        cnt = float(ser[r]) * v["L"]
        assert abs(cnt - round(cnt)) < 1e-2 and round(cnt) == v["counts"].min() == 4 + r, (case, r, cnt, v["counts"])


def test_lmmse_scale_takes_the_one_longer_slice():
    """One decided sample sits 1 % of a level spacing inside a boundary with the rescale over L + 1 track samples and 3 % outside with the
    rescale over L: 3 errors with the reference's rule, 4 without the extra sample."""
    fr = ra.longer_slice_frame()
    ser, shift, dec, out = run_lmmse([fr], 21, 20, True)
    v = ra.lmmse(fr["rx"], fr["taps"], fr["data"], fr["levels"], 21, 20)
    assert shift[0] == v["shift"] == 3 and v["counts"].min() == 3
    assert abs(float(ser[0]) * v["L"] - 3) < 1e-2, float(ser[0]) * v["L"]


# ------------------------------------------------------------------ vaeq_awgn_dfe
def run_dfe(ff, fb, init, lev, C, W, data=None, n_shift=24, n_cut=20, ff_taps=None, want_ff=False):
    """ff complex [R,N] goes in as rx through a one-tap identity feed-forward filter (exact), unless ff_taps is given."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import awgn_dfe
    rx = t(np.stack([ff.real, ff.imag], 1).astype(np.float32))
    taps = torch.tensor([1.0 + 0j]) if ff_taps is None else torch.from_numpy(ff_taps)
    r = awgn_dfe(rx, taps, torch.from_numpy(fb), t(init), lev, None if data is None else t(data), n_shift, n_cut, C=C, W=W, want_ff=want_ff)
    torch.cuda.synchronize()
    # the recursion's instantiation: <n_lev, 4> up to four feedback taps, <n_lev, 10> above
    assert nat.last_kernel() == f"vaeq::dfe_repair_kernel<{len(lev)}, {4 if fb.shape[1] <= 4 else 10}>", (nat.last_kernel(), len(lev), fb.shape)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


@pytest.mark.parametrize("K1", [1, 2, 11, 63, 64])
def test_dfe_feed_forward_against_float64(K1):
    """N = 1100 and 3001: the last 256-thread block is ragged; three runs with their own taps."""
    rng = np.random.default_rng(K1)
    for N in (1100, 3001):
        x = (rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N))).astype(np.complex64)
        taps = ((rng.standard_normal((3, K1)) + 1j * rng.standard_normal((3, K1))) / np.sqrt(K1)).astype(np.complex64)
        fb = np.full((3, 1), 0.1 + 0.1j, np.complex64)
        r = run_dfe(x, fb, np.zeros((3, N), np.int8), ra.qam_levels(4), 1, 0, ff_taps=taps, want_ff=True)
        for q in range(3):
            _hold([_note("dfe ff", crel(r["ff"][q], ra.compl_conv(x[q], taps[q])[:N]))], K1, N, q)


@pytest.mark.parametrize("case", ra.dfe_cases(), ids=lambda c: f"nl{c[0]}-k{c[1]}-n{c[2]}")
def test_dfe_recursion_is_exact(case):
    """Every decision equals the model's, for every chunking and warm-up of the case, with the runs of one call on their own fb taps; run_dfe
    holds the <NL, K2M> instantiation of every call.  No repair at C = 1; with seven chunks and no warm-up every chunk starts from the random
    init decisions, so the repair walk must have run."""
    n_lev, K2, N, outliers, chunkings = case
    frames = [ra.conditioned_dfe_frame(s, N, n_lev, K2, outliers) for s in ra.dfe_run_seeds(n_lev, K2, N)]
    want = np.stack([ra.dfe(f["ff"], f["fb"], f["init"], f["levels"])[0] for f in frames])
    assert np.array_equal(want, np.stack([f["expected"] for f in frames]))
    ff, fb, init = np.stack([f["ff"] for f in frames]), np.stack([f["fb"] for f in frames]), np.stack([f["init"] for f in frames])
    for C, W in chunkings:
        r = run_dfe(ff, fb, init, frames[0]["levels"], C, W)
        bad = np.argwhere(r["dec"].astype(np.int64) != want)
        assert len(bad) == 0, (case[:3], C, W, len(bad), bad[:5])
        assert np.all(r["repairs"] >= 0) and np.all(r["repairs"] <= N - K2), (C, W, r["repairs"])
        if C == 1:
            assert not r["repairs"].any()
        if (C, W) == (7, 0):
            assert np.all(r["repairs"] > 0), r["repairs"]


@pytest.mark.parametrize("n_lev,K2", [(n, k) for n in (2, 4, 8) for k in (1, 4, 5, 10)])
def test_dfe_shift_and_error_counts(n_lev, K2):
    fr = ra.conditioned_dfe_frame(100 * n_lev + K2, 1200, n_lev, K2, 7)
    base = run_dfe(fr["ff"][None], fr["fb"][None], fr["init"][None], fr["levels"], 5, 3)
    assert base["ser"] is None and np.array_equal(base["dec"][0].astype(np.int64), fr["expected"])
    for n_shift, n_cut, lag in ((1, 0, 0), (1, 20, 0), (24, 20, -12), (24, 20, 11), (24, 20, 5)):
        data = ra.shifted_data(fr["data"], lag, K2)
        ev = ra.dfe_eval(fr["expected"], data, fr["levels"], n_shift, n_cut)
        r = run_dfe(fr["ff"][None], fr["fb"][None], fr["init"][None], fr["levels"], 5, 3, data[None], n_shift, n_cut)
        assert np.array_equal(r["dec"], base["dec"])
        assert r["shift"][0] == ev["shift"] == lag
        cnt = float(r["ser"][0]) * ev["L"]
        assert abs(cnt - round(cnt)) < 1e-2 and round(cnt) == ev["counts"].min() > 0, (n_shift, n_cut, lag, cnt, ev["counts"])

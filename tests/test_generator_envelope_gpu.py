"""The channel generators (csrc/vaeq_gen.hip, csrc/vaeq_gen_fused.h) sample by sample against the float64 model tests/_ref_generator.py, over
their envelope: every kernel form (one-pass <2> / <4>, two-pass, clean frame, generic sps, staged hipFFT chain exact / padded, fused three-pass
rows N1 = 4 .. 20, 1 / 2 / 4 runs per wavefront, two stream blocks) at the tile boundaries, odd lengths, longest pulses and ragged groups.

Every case makes three assertions per checked run:
  data       (fp16) == float16(amps32[model levels]) exactly;
  sigma_out  within SIGMA_RTOL of the model's sigma (exactly sigma_fixed where that is given);
  |rx - (clean64 + sigma_dev noise64)| <= a max|clean64| + b sigma_dev at EVERY returned sample (no edge trimmed, no percentile), sigma_dev
             being the kernel's own sigma_out, so that an error of sigma shows in the second assertion only.

a, b per path (TOL): four times the largest residual measured once on an MI355X against this model -- a from the noise-free runs of the suite
(sigma_fixed = 0, SNR = 200 dB) as max residual / max|clean|, b from the noisy runs as max residual / sigma_dev (which still contains the clean
part, so b is generous by that much) -- and never above A_MAX = 1e-4, B_MAX = 1e-3: a wrong noise word, index or polarisation leaves a
residual of order sigma, a shifted sample or a missing tap one of order the amplitude, and either fails bounds that tight."""
import numpy as np
import pytest
import torch

import _ref_generator as M
from vae_equalizer_amd import _native as nat
from vae_equalizer_amd import channel as ch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIB = dict(symb_rate=90e9, tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000), phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64))
A_MAX, B_MAX, SIGMA_RTOL = 1e-4, 1e-3, 1e-4
# path: (a, b) = 4 x the measured maxima in the trailing comments (one MI355X), see the module docstring
TOL = {
    "awgn_fused": (8.4e-7, 3.2e-5),      # one-pass <2> / <4>, two-pass, clean frame:        a 2.078e-07, b 7.895e-06
    "awgn_generic": (1.6e-6, 4.7e-5),    # sps = 3 and sps = 1 (DFE), one thread per sample:  a 3.940e-07, b 1.172e-05
    "dp_exact": (2.1e-6, 1.13e-4),       # hipFFT chain on the exact length Ls:                a 5.091e-07, b 2.815e-05
    "dp_staged": (1.52e-6, 4.4e-5),      # hipFFT chain on a padded row:                       a 3.784e-07, b 1.082e-05
    "dp_fused": (1.45e-6, 8.4e-5),       # three-pass split FFT, N1 = 4 .. 20, rpw 1 / 2 / 4:  a 3.607e-07, b 2.091e-05
}
assert all(a <= A_MAX and b <= B_MAX for a, b in TOL.values())


# ------------------------------------------------------------------ inputs
def _amps(n_lev):
    a = np.arange(-(n_lev - 1), n_lev, 2, dtype=np.float64)
    return (a / np.sqrt(2 * np.mean(a * a))).astype(np.float32)                # unit mean power of the complex symbol


def _p_rows(n_lev, R):
    """Per-run pmfs: uniform, heavily shaped, one level of probability zero, repeating."""
    a = np.arange(-(n_lev - 1), n_lev, 2, dtype=np.float64)
    uni = np.full(n_lev, 1.0 / n_lev)
    shaped = np.array([0.85, 0.15]) if n_lev == 2 else np.exp(-0.9 * a * a / n_lev)
    zero = uni.copy()
    zero[1 if n_lev == 2 else n_lev // 2 - 1] = 0.0
    rows = [uni, shaped / shaped.sum(), zero / zero.sum()]
    return np.stack([rows[r % 3] for r in range(R)])


def _channel(n, seed=3):
    if n == 1:
        return np.ones(1, np.complex64)
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.8 ** np.arange(n)
    return (h / np.linalg.norm(h)).astype(np.complex64)


def _cplx(t):
    """[..., 2 (I, Q), S] device tensor -> complex128 numpy [..., S]."""
    x = t.cpu().numpy().astype(np.float64)
    return x[..., 0, :] + 1j * x[..., 1, :]


# ------------------------------------------------------------------ the three assertions
def _check_samples(path, tag, got, clean, nz, sig_dev):
    a, b = TOL[path]
    res = np.abs(got - (clean + sig_dev * nz)).max()
    peak = np.abs(clean).max()
    print(f"ENV {path} {tag} res/peak={res / peak:.3e} res/sigma={res / sig_dev if sig_dev > 0 else float('nan'):.3e} sigma/peak={sig_dev / peak:.3e}")
    assert res <= a * peak + b * sig_dev, (path, tag, res, peak, sig_dev)


def _check_sigma(tag, sig_dev, sig_model, fixed=None):
    if fixed is not None:
        assert sig_dev == float(np.float32(fixed)), (tag, sig_dev, fixed)
        return
    print(f"ENV sigma {tag} rel={abs(sig_dev / sig_model - 1):.3e}")
    assert abs(sig_dev / sig_model - 1) < SIGMA_RTOL, (tag, sig_dev, sig_model)


def _check_awgn(path, tag, out, geo, sps, N, amps, P, snr, seed, frame, fixed=None, runs=None):
    rx, data, sig = out
    R = rx.shape[0]
    assert rx.shape == (R, 2, sps * N) and data.shape == (R, 2, N) and data.dtype == torch.float16
    got, data, sig = _cplx(rx), data.cpu().numpy(), sig.cpu().numpy().astype(np.float64)
    cdf, lo, key = M.cdf_table(P), geo["ref_offset"], M.mix_seed(seed, 0)
    for r in range(R) if runs is None else runs:
        lev, clean, nz = M.awgn_run(key, frame, r, amps, cdf[r], geo["g"], sps, N, geo["N_conv"], lo)
        assert len(clean) == geo["Ls"]
        assert np.array_equal(data[r], amps[lev][:, lo:lo + N].astype(np.float16)), (tag, r)
        _check_sigma(f"{tag} r={r}", sig[r], M.sigma(clean, geo["Ls"], sps, snr[r]), None if fixed is None else fixed[r])
        _check_samples(path, f"{tag} r={r}", got[r], clean[:sps * N], nz, sig[r])


def _check_dp(path, tag, out, geo, sps, N, amps, P, snr, theta, seed, frame, Lrow, runs):
    rx, data, sig = out
    R = rx.shape[0]
    assert rx.shape == (R, 2, 2, sps * N) and data.shape == (R, 2, 2, N) and data.dtype == torch.float16
    cdf, lo = M.cdf_table(P), geo["ref_offset"]
    sig = sig.cpu().numpy().astype(np.float64)
    for r in runs:
        key, run = M.block_key_and_run(seed, r)
        lev, clean, pre, nz = M.dp_run(key, frame, run, amps, cdf[r], geo["g"], sps, N, geo["N_conv"], FIB["symb_rate"], FIB["tau_cd"],
                                       FIB["tau_pmd"], FIB["phiIQ"], theta[r], Lrow)
        assert pre.shape[1] == geo["Ls"]
        assert np.array_equal(data[r].cpu().numpy(), amps[lev][:, :, lo:lo + N].astype(np.float16)), (tag, r)
        _check_sigma(f"{tag} r={r}", sig[r], M.sigma(pre, geo["Ls"], sps, snr[r]))
        _check_samples(path, f"{tag} r={r}", _cplx(rx[r]), clean, nz, sig[r])


# ------------------------------------------------------------------ AWGN / ISI, sps = 2: Ls = 2 N + len(h) + 33
# (Ls, channel taps, n_lev): 1 tile | 1 | 2 | 2 (Lg = 96) | 3 | 4 | 4 | 5 tiles of 2048 -> onepass<2>, onepass<4>, two-pass; channels of 1 tap (a Dirac),
# with ref_offset odd (3, 4 taps) and even (1, 2, 6, 65 taps); 2082: Lout = 2048 ends on a tile boundary; Lout = 2012 (Ls = 2047), 3998 (4096), ...
# end in the middle of a thread's 8 samples
AWGN_CASES = [(2047, 2, 8), (2048, 1, 4), (2049, 4, 2), (2082, 1, 8), (4096, 65, 8), (4097, 2, 4), (8191, 4, 8), (8192, 3, 2), (8193, 6, 4)]


@pytest.mark.parametrize("twopass", [False, True], ids=["dispatched", "twopass"])
@pytest.mark.parametrize("Ls,Lh,n_lev", AWGN_CASES)
def test_awgn_sps2_frame(Ls, Lh, n_lev, twopass, monkeypatch):
    sps, R = 2, 5
    hc = _channel(Lh, seed=Ls)
    N = (Ls - Lh - 33) // 2
    geo = ch.awgn_frame_geometry(N, hc, sps)
    assert geo["Ls"] == Ls and geo["Lg"] == Lh + 31 <= 96 and sps * N <= Ls
    amps, P = _amps(n_lev), _p_rows(n_lev, R)
    snr = np.linspace(8.0, 20.0, R).astype(np.float32)
    fixed = np.array([0.05, 0.0, 0.3, 0.11, 0.2], np.float32)                # run 1: no noise at all, the clean bound alone
    seed, frame = 1000 + Ls, Lh
    if twopass:
        monkeypatch.setenv("VAEQ_AWGN_TWOPASS", "1")
    else:
        monkeypatch.delenv("VAEQ_AWGN_TWOPASS", raising=False)
    for sf in (None, fixed):
        out = ch.generate_awgn_batch_hip(R, N, amps, P, snr, hc, sps, DEV, seed, frame, return_sigma=True, sigma_fixed=sf)
        _check_awgn("awgn_fused", f"Ls={Ls} two={int(twopass)} fixed={int(sf is not None)}", out, geo, sps, N, amps, P, snr, seed, frame, sf)


def test_awgn_case_list_covers_the_dispatch():
    tiles = sorted({(Ls + 2047) // 2048 for Ls, _, _ in AWGN_CASES})
    assert tiles == [1, 2, 3, 4, 5]
    louts = [Ls - Lh - 33 for Ls, Lh, _ in AWGN_CASES]
    assert any(L % 2048 == 0 for L in louts) and any(L % 8 != 0 for L in louts)
    offs = {ch.awgn_frame_geometry(100, _channel(Lh), 2)["ref_offset"] % 2 for _, Lh, _ in AWGN_CASES}
    assert offs == {0, 1} and {n for _, _, n in AWGN_CASES} == {2, 4, 8} and any(Lh == 1 for _, Lh, _ in AWGN_CASES)


def test_awgn_pulse_longer_than_96_taps_is_refused():
    hc = _channel(66)
    assert ch.awgn_frame_geometry(500, hc, 2)["Lg"] == 97
    with pytest.raises(nat.VaeqError, match=r"unsupported sizes \(code -2\)"):
        ch.generate_awgn_batch_hip(2, 500, _amps(8), _p_rows(8, 2), 15.0, hc, 2, DEV, 1, 0)
    with pytest.raises(nat.VaeqError, match=r"unsupported sizes \(code -2\)"):
        ch.generate_awgn_clean_batch_hip(2, 500, _amps(8), _p_rows(8, 2), 15.0, hc, 2, DEV, 1, 0)


@pytest.mark.parametrize("Ls,Lh", [(2049, 4), (8193, 6)])
def test_awgn_clean_frame(Ls, Lh):
    """gen_tx_kernel<3>: the clean samples (staged through LDS), the tile power sums and the TX reference."""
    sps, R, n_lev = 2, 3, 8
    hc = _channel(Lh, seed=Ls)
    N = (Ls - Lh - 33) // 2
    geo = ch.awgn_frame_geometry(N, hc, sps)
    assert geo["Ls"] == Ls
    amps, P = _amps(n_lev), _p_rows(n_lev, R)
    seed, frame = 77, 4
    fr = ch.generate_awgn_clean_batch_hip(R, N, amps, P, 15.0, hc, sps, DEV, seed, frame)
    assert fr.sig.shape == (R, Ls, 2) and fr.power.shape == (R, (Ls + 2047) // 2048)
    sig = fr.sig.cpu().numpy().astype(np.float64)
    parts, data = fr.power.cpu().numpy(), fr.data.cpu().numpy()
    cdf, lo = M.cdf_table(P), geo["ref_offset"]
    for r in range(R):
        lev, clean, _ = M.awgn_run(M.mix_seed(seed, 0), frame, r, amps, cdf[r], geo["g"], sps, N, geo["N_conv"], lo)
        assert np.array_equal(data[r], amps[lev][:, lo:lo + N].astype(np.float16))
        _check_samples("awgn_fused", f"clean Ls={Ls} r={r}", sig[r, :, 0] + 1j * sig[r, :, 1], clean, np.zeros(Ls), 0.0)
        pw = 0.0
        for t in range(parts.shape[1]):                                        # in tile order
            pw += float(parts[r, t])
        want = float(np.sum(np.abs(clean) ** 2))
        print(f"ENV power clean Ls={Ls} r={r} rel={abs(pw / want - 1):.3e}")
        assert abs(pw / want - 1) < 1e-5
        # and tile by tile: the sums belong to their own 2048 samples
        for t in range(parts.shape[1]):
            wt = float(np.sum(np.abs(clean[2048 * t:2048 * (t + 1)]) ** 2))
            assert abs(float(parts[r, t]) - wt) < 1e-5 * want


# ------------------------------------------------------------------ generic kernels (one thread per sample)
@pytest.mark.parametrize("N,R", [(333, 4), (16387, 2)], ids=["small", "gridstride"])
def test_awgn_generic_sps3(N, R):
    """sps = 3, 16-QAM, N odd (Lout odd: the i + 1 < Lout tail).  N = 16387: Ls > 3 N > 32768 samples, N > 16384 reference symbols and more than
    16384 noise pairs, so the 64-block grid-stride loops of gen_tx_generic_kernel, gen_ref_kernel and gen_finish_kernel all go round again."""
    sps, n_lev = 3, 4
    hc = _channel(5, seed=N)
    geo = ch.awgn_frame_geometry(N, hc, sps)
    assert N % 2 == 1 and (N < 1000 or (N > 64 * 256 and (sps * N + 1) // 2 > 64 * 256))
    amps, P = _amps(n_lev), _p_rows(n_lev, R)
    snr = np.linspace(8.0, 20.0, R).astype(np.float32)
    fixed = np.array([0.0, 0.2, 0.07, 0.13][:R], np.float32)
    for sf in (None, fixed):
        out = ch.generate_awgn_batch_hip(R, N, amps, P, snr, hc, sps, DEV, 31, 6, return_sigma=True, sigma_fixed=sf)
        _check_awgn("awgn_generic", f"sps3 N={N} fixed={int(sf is not None)}", out, geo, sps, N, amps, P, snr, 31, 6, sf)


def test_dfe_generic_sps1():
    """sps = 1 with the raised-cosine (DFE) geometry, N odd: Lout odd."""
    N, R, n_lev = 1501, 4, 8
    hc = _channel(5, seed=8)
    geo = ch.dfe_frame_geometry(N, hc, 1)
    amps, P = _amps(n_lev), _p_rows(n_lev, R)
    snr = np.linspace(8.0, 20.0, R).astype(np.float32)
    fixed = np.array([0.1, 0.0, 0.25, 0.02], np.float32)
    for sf in (None, fixed):
        out = ch.generate_dfe_batch_hip(R, N, amps, P, snr, hc, DEV, 13, 2, sigma_fixed=sf, return_sigma=True)
        _check_awgn("awgn_generic", f"dfe N={N} fixed={int(sf is not None)}", out, geo, 1, N, amps, P, snr, 13, 2, sf)
        rx2, data2 = ch.generate_dfe_batch_hip(R, N, amps, P, snr, hc, DEV, 13, 2, sigma_fixed=sf)
        assert torch.equal(rx2, out[0]) and torch.equal(data2, out[1])


# ------------------------------------------------------------------ DP
def _dp_inputs(R, n_lev=8, seed=0):
    """Per-run P, theta and SNR (as the float32 values the kernel is given); the last of a short batch is noise-free (200 dB): it pins a."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(-np.pi, np.pi, R).astype(np.float32)
    snr = rng.uniform(10.0, 30.0, R).astype(np.float32)
    if R <= 8:
        snr[-1] = 200.0
    return _amps(n_lev), _p_rows(n_lev, R), snr, theta


def _dp_generate(R, N, amps, P, snr, theta, hc, sps, seed, frame, fft):
    return ch.generate_batch_hip(R, N, amps, P, snr, hc, FIB["symb_rate"], sps, FIB["tau_cd"], FIB["tau_pmd"], FIB["phiIQ"], theta, DEV, seed,
                                 frame, return_sigma=True, fft=fft)


def _longest_N(row, hc, sps=2):
    return (row - 64 - ch.dp_frame_geometry(100, hc, sps)["Ls"] + sps * 100) // sps


@pytest.mark.parametrize("inside", [False, True], ids=["longest", "inside"])
@pytest.mark.parametrize("n1", [4, 5, 8, 10, 16, 20])
def test_dp_fused_rows(n1, inside, monkeypatch):
    """The default frame (three-pass split FFT), every row length, the whole frame including the edges of the padded row."""
    sps, R, hc = 2, 3, _channel(3, seed=n1)
    N = _longest_N(1024 * n1, hc) - (300 if inside else 0)
    geo = ch.dp_frame_geometry(N, hc, sps)
    assert ch.padded_row_len(geo["Ls"] + 64) == 1024 * n1 and (inside or geo["Ls"] + 64 >= 1024 * n1 - 1)
    amps, P, snr, theta = _dp_inputs(R, seed=n1)
    monkeypatch.delenv("VAEQ_GEN_STAGED", raising=False)
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, 40 + n1, 3, "padded")
    _check_dp("dp_fused", f"n1={n1} N={N}", out, geo, sps, N, amps, P, snr, theta, 40 + n1, 3, 1024 * n1, range(R))


def test_dp_fused_long_pulse():
    """A combined pulse longer than 64 taps: symbols past Lrow / 2 exist and belong to the last stripe's halo."""
    sps, R = 2, 3
    hc = np.concatenate([_channel(3), 0.05 * np.exp(1j * np.arange(50))]).astype(np.complex64)
    N = _longest_N(4096, hc)
    geo = ch.dp_frame_geometry(N, hc, sps)
    assert geo["Lg"] > 64 and ch.padded_row_len(geo["Ls"] + 64) == 4096
    amps, P, snr, theta = _dp_inputs(R, n_lev=4, seed=1)
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, 9, 1, "padded")
    _check_dp("dp_fused", f"long pulse Lg={geo['Lg']}", out, geo, sps, N, amps, P, snr, theta, 9, 1, 4096, range(R))


@pytest.mark.parametrize("fft,N,Lc,odd", [("padded", None, 3, 0), ("exact", 600, 3, 0), ("exact", 601, 4, 1)], ids=["padded", "exact-even", "exact-odd"])
def test_dp_staged_chain(fft, N, Lc, odd, monkeypatch):
    """The five-pass hipFFT chain: on the padded row N1 = 4 (what VAEQ_GEN_STAGED=1 selects) and on the exact sequence length, even and odd."""
    sps, R, hc = 2, 3, _channel(Lc, seed=5)
    N = _longest_N(4096, hc) if N is None else N
    geo = ch.dp_frame_geometry(N, hc, sps)
    Lrow = 4096 if fft == "padded" else geo["Ls"]
    assert geo["Ls"] == 2 * N + Lc + 33 and geo["Ls"] % 2 == odd
    amps, P, snr, theta = _dp_inputs(R, seed=N)
    monkeypatch.setenv("VAEQ_GEN_STAGED", "1")
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, 7, 2, fft)
    _check_dp("dp_staged" if fft == "padded" else "dp_exact", f"staged {fft} Ls={geo['Ls']}", out, geo, sps, N, amps, P, snr, theta, 7, 2, Lrow, range(R))


@pytest.mark.parametrize("fft", ["exact", "padded"])
def test_dp_generic_sps3(fft, monkeypatch):
    """sps = 3: generic stage 1, hipFFT, gen_power_kernel."""
    sps, R, N, hc = 3, 3, 201, _channel(2, seed=6)
    geo = ch.dp_frame_geometry(N, hc, sps)
    Lrow = geo["Ls"] if fft == "exact" else ch.padded_row_len(geo["Ls"] + 64)
    amps, P, snr, theta = _dp_inputs(R, n_lev=4, seed=2)
    monkeypatch.delenv("VAEQ_GEN_STAGED", raising=False)
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, 3, 0, fft)
    _check_dp("dp_exact" if fft == "exact" else "dp_staged", f"sps3 {fft}", out, geo, sps, N, amps, P, snr, theta, 3, 0, Lrow, range(R))


@pytest.mark.parametrize("R", [1027, 4099], ids=["rpw2", "rpw4"])
def test_dp_fused_runs_per_wavefront(R, monkeypatch):
    """genf_fft_kernel takes 2 runs per wavefront from R = 1024 and 4 from R = 4096: both, each with a ragged last group."""
    sps, N, hc = 2, 1000, _channel(3, seed=2)
    geo = ch.dp_frame_geometry(N, hc, sps)
    assert ch.padded_row_len(geo["Ls"] + 64) == 4096
    amps, P, snr, theta = _dp_inputs(R, seed=R)
    monkeypatch.delenv("VAEQ_GEN_STAGED", raising=False)
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, 19, 1, "padded")
    runs = [0, 1, R // 2] + list(range(R - 5, R))
    _check_dp("dp_fused", f"R={R}", out, geo, sps, N, amps, P, snr, theta, 19, 1, 4096, runs)


def test_dp_stream_blocks():
    """Runs past STREAM_BLOCK draw with the key of their block and the run counter r % STREAM_BLOCK."""
    sps, N, R, seed, frame = 2, 64, ch.STREAM_BLOCK + 3, 23, 5
    hc = _channel(31, seed=4)                                                  # Ls = 2 N + 31 + 33 = 192
    geo = ch.dp_frame_geometry(N, hc, sps)
    amps, P, snr, theta = _dp_inputs(R, seed=3)
    B = ch.STREAM_BLOCK
    P[B:B + 3], snr[B:B + 3], theta[B:B + 3] = P[:3], snr[:3], theta[:3]      # the two triples differ in their streams only
    out = _dp_generate(R, N, amps, P, snr, theta, hc, sps, seed, frame, "exact")
    _check_dp("dp_exact", "blocks", out, geo, sps, N, amps, P, snr, theta, seed, frame, geo["Ls"], [0, 1, 2, B - 1, B, B + 1, B + 2])
    rx, data, sig = out
    cdf, lo = M.cdf_table(P), geo["ref_offset"]
    for i in range(3):                                                         # spelled out: key _mix_seed(seed, 8192) with counters 0 .. 2, key _mix_seed(seed, 0)
        for r, key in ((i, M.mix_seed(seed, 0)), (B + i, M.mix_seed(seed, B))):
            lev = np.stack([M.symbols(key, frame, i, p, np.arange(geo["N_conv"]), cdf[r]) for p in range(2)])
            assert np.array_equal(data[r].cpu().numpy(), amps[lev][:, :, lo:lo + N].astype(np.float16))
        assert not torch.equal(data[i], data[B + i]) and not torch.equal(rx[i], rx[B + i])

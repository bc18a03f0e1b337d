"""Drop-in for AWGN_channel/DFE_MQAM_shaping.py: the known-channel ("genie") LMMSE and DFE reference curves of the AWGN channel.

Same module constants and functions (positional names as in the reference); the frame work runs on HIP: the generator (vaeq_gen_awgn at
1 sps with the raised-cosine geometry, or the reference-faithful numpy restatement when seeded), the LMMSE evaluation in one launch for all
frames (vaeq_awgn_lmmse_eval) and the DFE as an exact speculate-and-repair recursion (vaeq_awgn_dfe).  The filter design stays on the host
in torch cfloat, as in the reference.

The one intended difference: importing this module runs nothing.  The reference runs its sweep and a plot at import; here the sweep is
``main()`` (or ``python -m vae_equalizer_amd.DFE_MQAM_shaping``) and returns (SER_mmse, SER_dfe).  Plotting is out of scope.

``info_metrics = True`` adds what a shaping sweep is read in -- GMI, NGMI, achievable rate and pre-FEC BER of both curves -- over exactly the
symbols each SER keeps (engine.awgn_track_info; the DFE's soft sequence is its slicer input, engine.awgn_dfe_soft).
"""
import numpy as np
import torch

from . import channel as ch
from .func_CMA_MQAM_shaping import find_shift_symb  # noqa: F401  (:137-150: the same text as in func_CMA_MQAM_shaping.py)

# ------------------------------------------------------------------ the reference's module constants (:17-56, :246-262)
CHANNELS = {
    "proakis_a": np.array([0.04, -0.05, 0.07, -0.21, -0.5, 0.72, 0.36, 0, 0.21, 0.03, 0.07]),
    "proakis_b": np.array([0.407, 0.815, 0.407]),
    "proakis_c": np.array([0.227, 0.460, 0.688, 0.460, 0.227]),
    "h1": np.array([0.0545 + 1j * 0.05, 0.2823 - 1j * 0.11971, -0.7676 + 1j * 0.2788, -0.0641 - 1j * 0.0576,
                    0.0466 - 1j * 0.02275]).astype(np.complex64),
    "h2": np.array([0.0545 + 1j * 0.0165, -1.3449 - 1j * 0.4523, 1.0067 + 1j * 1.1524, 0.3476 + 1j * 0.3153]).astype(np.complex64),
}
h_channel_orig = CHANNELS["h1"]                        # Caciularu h_1 (:23)
mod = '64-QAM'
M = len(h_channel_orig)
sps = 1                                                # the reference implements 1 sps only


def channel_taps(h_orig, sps=1):
    """Zero-stuffed, unit-norm channel (:33-37)."""
    h = np.zeros(sps * (np.asarray(h_orig).shape[-1] - 1) + 1, dtype=np.complex64)
    h[0::sps] = h_orig
    h /= np.linalg.norm(h)
    return h


def qam_constants(mod):
    """constellation (I-major: index = iI * n + iQ), const_torch, amp_levels, num_lev, const_mean of :39-51."""
    n = {'4-QAM': 2, '16-QAM': 4, '64-QAM': 8}[mod]
    lev = np.arange(-(n - 1), n, 2)
    pts = (np.repeat(lev, n) + 1j * np.tile(lev, n)).astype(np.complex128)
    constellation = pts / np.sqrt(np.mean(np.abs(pts) ** 2))
    amp = torch.tensor(constellation.real[::n], dtype=torch.float32)
    return dict(constellation=constellation, const_torch=torch.tensor(constellation, dtype=torch.cfloat), amp_levels=amp, num_lev=n,
                const_mean=torch.tensor(np.mean(np.abs(constellation)), dtype=torch.float32))


h_channel = channel_taps(h_channel_orig, sps)
h_tensor = torch.tensor(h_channel, dtype=torch.cfloat)
_q = qam_constants(mod)
constellation, const_torch, amp_levels, num_lev, const_mean = (_q[k] for k in ("constellation", "const_torch", "amp_levels", "num_lev",
                                                                               "const_mean"))

SNR_vec = np.arange(15, 23, 1)
nu = 0.0270955
N_valid = 128000
N_cut = 20
lmmse_filter_order = 20
M_dfe = 11
num_epochs = 5
n1 = (lmmse_filter_order - 1) // 2 + 1
N_SHIFT_LMMSE, N_SHIFT_DFE = 21, 24                    # find_shift_symb lags (:280, :292)

info_metrics = False    # True: main() also returns the info dicts of both curves (AIR, GMI, NGMI, BER, kept, sym_err, bit_err, hyp)
fec_metrics = None      # dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75, depth=None, quant=None, outer=None; quant=dict(bits=5) decodes in fixed point and takes no alpha; outer=dict(code=fec.BchCode, ...) puts fec.bch_outer behind it, and the .mat also gains BER_outer and FER_outer; code=fec.ScLdpcCode takes window, iters and test in place of max_iter, depth and quant and decodes with fec.ldpc_sc_decode): main() also returns fec.ldpc_decode's figures of both curves' LLRs
base_seed = None        # int -> reproducible frames (the reference's stream under the same seed); None = like the reference
generator = None        # None: "hip" (on-device generator vaeq_gen_awgn) for unseeded sweeps, "numpy" (reference-faithful host simulator) when base_seed is set

rcfir, rrcfir = ch.rcfir, ch.rrcfir


def generate_data_shaping(N, amp_levels, SNR, h_channel, nu, *, rng=None, noise=None, device="cpu"):
    """:77-105 (host restatement, the reference's random-number consumption; rng / noise as in channel.SeededStreams)
    -> (rx[2,N] f32, data[2,N] f16, P f32)."""
    amps = torch.as_tensor(amp_levels).detach().cpu().numpy()
    rx, data, P = ch.generate_data_rc(N, amps, SNR, h_channel, nu, sps, rng=rng, noise=noise)
    return (torch.from_numpy(rx).to(device, torch.float32), torch.from_numpy(data).to(device, torch.float16),
            torch.tensor(P, device=device, dtype=torch.float32))


def SER_func(rx, tx, amp_levels=None, num_lev=None):
    """:107-135 (batched over leading dims): rescales rx IN PLACE by mean|tx| / mean|rx| -- over ALL of rx's samples, which may be more
    than tx's (the LMMSE slice is one longer) --, per-axis decisions on the first tx.shape[-1] samples, minimum SER over the 0 / pi / pi/4 /
    3pi/4 relabelings.  amp_levels / num_lev default to the module's."""
    lev = (globals()["amp_levels"] if amp_levels is None else torch.as_tensor(amp_levels)).to(rx.device, torch.float32).reshape(-1, 1)
    n = lev.shape[0] if num_lev is None else num_lev
    N = tx.shape[-1]
    scale = (n - 1) / 2
    t = tx.float()
    data = torch.round(scale * t + scale)
    rx *= (torch.mean(torch.sqrt(t[..., 0, :] ** 2 + t[..., 1, :] ** 2), -1) /
           torch.mean(torch.sqrt(rx[..., 0, :] ** 2 + rx[..., 1, :] ** 2), -1))[..., None, None]
    dec = torch.stack([torch.argmin(torch.abs(rx[..., 0, :N].unsqueeze(-2) - lev), -2),
                       torch.argmin(torch.abs(rx[..., 1, :N].unsqueeze(-2) - lev), -2)], -2).float()
    dec_pi = -(dec - scale * 2)
    dec_pi4 = torch.stack([-(dec[..., 1, :] - scale * 2), dec[..., 0, :]], -2)
    dec_3pi4 = -(dec_pi4 - scale * 2)
    return torch.stack([((data - d) != 0).any(-2).float().mean(-1) for d in (dec, dec_pi, dec_pi4, dec_3pi4)], -1).min(-1).values


def compute_lmmse(channel, SNR, order, n1):
    """:154-168: the LMMSE taps (length ``order``) from the channel and the SNR; H @ H.T without conjugation, result flipped."""
    h = torch.as_tensor(channel).to("cpu", torch.cfloat)
    L = h.numel() - 1
    sigma_w = 1 / 2 / 10 ** (SNR / 10)
    H = torch.zeros((order, order + L), dtype=torch.cfloat)
    hr = torch.flip(h, dims=[0])
    for i in range(order):
        H[i, i:i + L + 1] = hr
    A = sigma_w * torch.eye(order) + torch.matmul(H, H.T)
    return torch.flip(torch.matmul(torch.linalg.inv(A), H[:, -(n1 + 1)]), dims=[0])


def compute_feedforward(channel, SNR, order):
    """:170-184: the DFE's feed-forward taps (a causal MMSE filter of ``order`` taps)."""
    h = torch.as_tensor(channel).to("cpu", torch.cfloat)
    L = h.numel() - 1
    sigma_w = 1 / 2 / 10 ** (SNR / 10)
    H = torch.zeros([order, order], dtype=torch.cfloat)
    for i in range(order - L):
        H[i, i:i + L + 1] = h
    for i in range(L):
        H[order - L + i, order - L + i:] = h[:L - i]
    rhs = torch.cat((torch.zeros(order - L - 1, dtype=torch.cfloat), torch.flip(h, dims=[0])))
    return torch.matmul(torch.linalg.inv(sigma_w * torch.eye(order, dtype=torch.cfloat) + torch.matmul(H, H.T)), rhs)


def compute_feedback_filter(channel, feedforward):
    """:186-198: fb[k] = -sum ff[-(L-k):] * flip(channel[k+1:]) (no conjugation), L = len(channel) - 1 taps."""
    h = torch.as_tensor(channel).to("cpu", torch.cfloat)
    f = torch.as_tensor(feedforward).to("cpu", torch.cfloat)
    L = h.numel() - 1
    fb = torch.zeros(L, dtype=torch.cfloat)
    for k in range(L):
        fb[k] = -torch.dot(f[-(L - k):], torch.flip(h[k + 1:], dims=[0]))
    return fb


def compl_conv(rx, h):
    """:236-241: complex convolution from four real conv1d with the flipped taps and padding K // 2 (torch restatement)."""
    K = h.shape[-1]
    x = rx.reshape(1, 1, rx.shape[-1])
    k = torch.flip(h, dims=[-1]).reshape(1, 1, K).to(x.device)
    cv = lambda a, b: torch.nn.functional.conv1d(a, b, padding=K // 2)  # noqa: E731
    out = (cv(x.real, k.real) - cv(x.imag, k.imag)) + 1j * (cv(x.imag, k.real) + cv(x.real, k.imag))
    return out.squeeze()


def nearest_neighbor(rx_syms, const=None):
    """:224-234: index of the nearest constellation point (complex distance over all points, first index on ties)."""
    c = (const_torch if const is None else const).to(rx_syms.device)
    return torch.argmin(torch.abs(c.reshape(-1, 1) - rx_syms.reshape(1, -1)), dim=0)


def dfe(feedforward_output, feedforward_filter, feedback_filter, init_decisions_idxs, amp_levels=None):
    """:200-222 on the HIP recursion (vaeq_awgn_dfe): the first K2 decisions are init_decisions_idxs[:K2], then the feedback recursion on
    the feed-forward output.  Returns the decision indices as a float32 tensor (the reference's state_idxs)."""
    from .dp_runs import default_device
    from .engine import awgn_dfe
    dev = feedforward_output.device if feedforward_output.is_cuda else default_device()
    y = torch.as_tensor(feedforward_output).to(dev, torch.cfloat).reshape(1, -1)
    x = torch.stack([y.real, y.imag], 1).contiguous()                      # the feed-forward output itself, through a one-tap identity FIR
    one = torch.tensor([1.0 + 0.0j], dtype=torch.cfloat)
    lev = globals()["amp_levels"] if amp_levels is None else amp_levels
    init = torch.as_tensor(init_decisions_idxs).to(dev).long().to(torch.int8).reshape(1, -1)
    r = awgn_dfe(x, one, torch.as_tensor(feedback_filter).to(torch.cfloat), init, lev)
    return r["dec"][0].float().to(feedforward_output.device)


def _filters(h, SNR):
    """Per SNR (:264-269): LMMSE taps, feed-forward and feedback filters."""
    ht = torch.tensor(h, dtype=torch.cfloat)
    lm = compute_lmmse(ht, SNR, lmmse_filter_order, lmmse_filter_order // 2 + 1)
    ff = compute_feedforward(ht, SNR, M_dfe)
    return lm, ff, compute_feedback_filter(ht, ff)


def run_dfe_batch(SNRs, num_epochs, N_valid, mod="64-QAM", h_orig=None, nu=0.0270955, *, seed=None, generator=None, device=None,
                  verbose=False, C=None, W=None, want_info=False, want_llr=False, fec=None):
    """The script's loop nest (:264-296) for a channel (h_orig: symbol-spaced taps, default h_1) and a modulation, all frames at once:
    R = len(SNRs) * num_epochs frames, one generator call, ONE LMMSE evaluation launch and ONE DFE launch.

    seed / generator: as in Eval_run_shaping_cma.py -- with a seed the frames come from the reference-faithful numpy generator in the
    reference's loop order (SNR-major; those of the reference under the same seed), without one from the device generator.
    Returns dict(SER_mmse [num_snr, num_epochs], SER_dfe (CPU float32), shift_mmse, shift_dfe, repairs (numpy), C, W); with want_info also
    info_mmse and info_dfe, each dict(AIR, GMI, NGMI, BER f32; kept, sym_err, bit_err, hyp int64) of [num_snr, num_epochs] CPU tensors:
    engine.awgn_track_info at edge N_cut + 11 on the LMMSE output (one sample longer than the data) at shift_mmse and on the DFE's slicer input
    (engine.awgn_dfe_soft) at shift_dfe, demapped at var = 10^(-SNR/10), the VAE-LE's of the same SNR (func_VAELE_MQAM_shaping.py:272).
    With want_llr also llr_mmse and llr_dfe, each dict(llr[num_snr, num_epochs, 2b, N_valid] f32, bits[num_snr, num_epochs, 2b, N_valid] int8,
    hyp[num_snr, num_epochs]) ON THE DEVICE: engine.awgn_track_llr on the same two tracks, shifts, edge and var under the hypothesis of
    awgn_track_info on them (want_info's call, when that is on), and fec.label_bits of the TX data.  All frames go through one launch, so
    all of them are returned; the two dicts share one bits tensor: num_snr x num_epochs x 2b x N_valid x (2 x 4 + 1) bytes (64-QAM, 15 SNRs x
    10 epochs x 10 000 symbols: 81 MB).
    Every other output is the same with and without it.
    With fec = dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75, depth=None) also fec_mmse and fec_dfe ON THE DEVICE: fec.ldpc_decode's
    figures of those LLRs (computed for it; llr_* itself is returned only with want_llr), all num_snr x num_epochs frames as the run axis of one
    call per curve: the counters [num_snr, num_epochs, C], the rates [num_snr, num_epochs].  A quant=dict(bits, scale=None, app_bits=None, num=6, beta=0) in fec decodes in
    fixed point (vaeq_ldpc_decode_q; no alpha then).  A bad fec dict is a ValueError before anything is allocated or launched."""
    from .dp_runs import default_device, fresh_seed, resolve_generator
    from .engine import awgn_dfe, awgn_dfe_soft, awgn_lmmse_eval, awgn_track_info, awgn_track_llr
    from .fec import check_fec, fec_figures, label_bits
    check_fec(fec)
    need_llr = want_llr or fec is not None
    device = default_device() if device is None else torch.device(device)
    h = channel_taps(CHANNELS["h1"] if h_orig is None else np.asarray(h_orig), sps)
    q = qam_constants(mod)
    amps = q["amp_levels"].numpy()
    SNRs = [float(s) if not float(s).is_integer() else int(s) for s in np.asarray(SNRs).reshape(-1)]
    S, E = len(SNRs), int(num_epochs)
    R = S * E
    filt = [_filters(h, s) for s in SNRs]
    per = lambda k: torch.stack([filt[r // E][k] for r in range(R)])  # noqa: E731
    lm, ff, fb = per(0), per(1), per(2)
    generator = resolve_generator(generator, seed is not None)
    if generator == "numpy":
        st = ch.SeededStreams(seed) if seed is not None else None
        frames = [ch.generate_data_rc(N_valid, amps, SNRs[r // E], h, nu, sps, rng=st.next_rng() if st else None, noise=st.noise if st else None)
                  for r in range(R)]
        rx = torch.from_numpy(np.stack([f[0] for f in frames])).to(device)
        data = torch.from_numpy(np.stack([f[1] for f in frames])).to(device)
    elif generator == "hip":
        P = ch.pcs_probabilities(amps, nu)
        rx, data = ch.generate_dfe_batch_hip(R, N_valid, amps, P, np.repeat(np.asarray(SNRs, np.float32), E), h, device,
                                             fresh_seed() if seed is None else seed, 0)
    else:
        raise ValueError(f"unknown generator {generator!r}")
    ser_m, sh_m, dec_m, out_m = awgn_lmmse_eval(rx, lm, data, amps, N_SHIFT_LMMSE, N_cut, want_out=want_info or need_llr)
    r = awgn_dfe(rx, ff, fb, dec_m, amps, data, N_SHIFT_DFE, N_cut, C=C, W=W, want_ff=want_info or need_llr)
    info = {}
    if want_info or need_llr:
        P = ch.pcs_probabilities(amps, nu)
        var = [10 ** (-SNRs[k // E] / 10) for k in range(R)]
        on_grid = lambda d: {k: v.cpu().reshape(S, E) for k, v in d.items()}  # noqa: E731
        bits = label_bits(data, len(amps)).reshape(S, E, -1, data.shape[-1]) if need_llr else None

        def on_se(v):                                                           # fec_figures' [R, ...] tensors on the (SNR, epoch) grid; "outer" is a dict of them, "quant" the resolved dict
            if torch.is_tensor(v):
                return v.reshape(S, E, *v.shape[1:])
            return {k: on_se(x) for k, x in v.items()} if isinstance(v, dict) else v

        for key, z, sh in (("mmse", out_m, sh_m), ("dfe", awgn_dfe_soft(r["ff"], fb, r["dec"], amps), r["shift"])):
            fig = awgn_track_info(z, data, amps, P, var, sh, N_cut + 11)
            if want_info:
                info["info_" + key] = on_grid(fig)
            if need_llr:                                                        # the same track, shift, edge and var as fig, under its hypothesis
                llr = awgn_track_llr(z, data, amps, var, sh, fig["hyp"], N_cut + 11)
                if want_llr:
                    info["llr_" + key] = dict(llr=llr.reshape(S, E, *llr.shape[1:]), bits=bits, hyp=fig["hyp"].reshape(S, E))
                if fec is not None:
                    info["fec_" + key] = on_se(fec_figures(dict(llr=llr, bits=bits.reshape(R, *bits.shape[2:])), fec))
    out = dict(SER_mmse=ser_m.cpu().reshape(S, E), SER_dfe=r["ser"].cpu().reshape(S, E), shift_mmse=sh_m.cpu().numpy().reshape(S, E),
               shift_dfe=r["shift"].cpu().numpy().reshape(S, E), repairs=r["repairs"].cpu().numpy().reshape(S, E), C=r["C"], W=r["W"])
    out.update(info)
    if verbose:
        for s in range(S):
            for e in range(E):
                print(e, SNRs[s], '\t\t\t\t\t\t\tSER_mmse = ', out["SER_mmse"][s, e].item(), '\t\t\t SER_dfe = ', out["SER_dfe"][s, e].item())
    return out


def main():
    """The reference's sweep (:264-296) with the module's constants -> (SER_mmse, SER_dfe), each [num_snr, num_epochs] (CPU float32); with
    info_metrics (SER_mmse, SER_dfe, info_mmse, info_dfe), the two dicts as run_dfe_batch's; with fec_metrics additionally fec_mmse and fec_dfe,
    run_dfe_batch's (on the device), at the end."""
    from .dp_runs import default_device
    device = default_device()
    print("We are using the following device for learning:", device)
    r = run_dfe_batch(SNR_vec, num_epochs, N_valid, mod, h_channel_orig, nu, seed=base_seed, generator=generator, device=device,
                      verbose=True, want_info=info_metrics, fec=fec_metrics)
    out = (r["SER_mmse"], r["SER_dfe"], r["info_mmse"], r["info_dfe"]) if info_metrics else (r["SER_mmse"], r["SER_dfe"])
    return out if fec_metrics is None else out + (r["fec_mmse"], r["fec_dfe"])


if __name__ == "__main__":
    main()

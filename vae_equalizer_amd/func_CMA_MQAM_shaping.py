"""Drop-in for AWGN_channel/func_CMA_MQAM_shaping.py: same ``processing`` signature (:201) and return value (:256), with the per-symbol
training loop on one HIP wave per run (vaeq_awgn_cma) and each evaluated epoch -- CMA(..., eval=False), CPE, find_shift_symb, SER_CMA
(:225-232) -- in one HIP launch for all runs (vaeq_awgn_cma_validate).

The mirrors CPE / find_shift_symb / SER_CMA / SER_symb keep the reference's call surface as batched torch restatements on the device; they
are also the cross-check of the fused validation kernel (cma_validate_torch)."""
import torch

from . import channel as ch
from .awgn_runs import check_generator, first_run, run_awgn_epochs
from .dp_runs import default_device, resolve_generator
from .engine import awgn_cma, awgn_cma_validate, awgn_track_info, awgn_track_llr
from .fec import check_fec, label_bits
from .func_VAELE_MQAM_shaping import SER_symb, awgn_batch_tables, awgn_tables  # noqa: F401  (SER_symb: identical text in both reference modules)

rcfir, rrcfir = ch.rcfir, ch.rrcfir
generate_data = ch.generate_data                       # (:39-61) host restatement, reference signature + optional rng / noise streams
M_MA = 501                                             # CPE moving-average length (:172)
N_SHIFT = 21                                           # find_shift_symb lags (:230)


def CMA(Rx, R, h, lr, sps, eval):
    """:142-168 on the HIP kernel: Rx[2,N], h[2,M] (updated IN PLACE when ``eval``) -> (out[2,N//sps], h, e[N//sps]) at the reference's
    wrapped indices (symbol j lands at j - (mh - mh // sps))."""
    if h.dtype != torch.float32 or not h.is_contiguous():
        raise ValueError("h must be a contiguous float32 tensor [2, M]")
    _, out, e = awgn_cma(Rx.reshape(1, 2, -1).float(), h.detach().unsqueeze(0), lr, sps, bool(eval), float(R), want_out=True, want_e=True)
    return out[0], h, e[0]


def CPE(y):
    """:170-198, batched over leading dims: y[..., 2, K] -> de-rotated y (4th power, zero-padded 501-tap moving average, atan2 / 4;
    no unwrapping)."""
    a, b = y[..., 0, :], y[..., 1, :]
    a2, b2 = a ** 2, b ** 2
    p4 = torch.stack([a2 ** 2 - 6 * a2 * b2 + b2 ** 2, 4 * (a2 * a * b - a * b2 * b)], -2)
    lead = p4.shape[:-2]
    k = torch.full((1, 1, M_MA), 1 / M_MA, device=y.device, dtype=torch.float32)
    ma = torch.nn.functional.conv1d(p4.reshape(-1, 1, p4.shape[-1]).float(), k, padding=M_MA // 2).reshape(*lead, 2, -1)
    phi = torch.atan2(ma[..., 1, :], -ma[..., 0, :]) / 4
    c, s = torch.cos(phi), torch.sin(phi)
    return torch.stack([a * c - b * s, b * c + a * s], -2)


def find_shift_symb(rx, tx, N_shift):
    """:127-140, batched over leading dims: correlation of tx[.., 0, N_shift//2:1000] with the I rail of rx at N_shift lags (tx's Q rail as
    the fallback when the I peak is below 0.02 * K) -> argmax - N_shift // 2 (first index on ties)."""
    half = N_shift // 2
    n = 1000 - half
    mat = torch.stack([rx[..., 0, i:n + i] for i in range(N_shift)], -1)                    # [..., n, N_shift]
    corr = (tx[..., 0, half:1000].float().unsqueeze(-2) @ mat).squeeze(-2).abs()
    corr_IQ = (tx[..., 1, half:1000].float().unsqueeze(-2) @ mat).squeeze(-2).abs()
    mI, aI = corr.max(-1)
    mQ, aQ = corr_IQ.max(-1)
    use_q = (mI < 0.02 * rx.shape[-1]) & (mQ >= mI)
    return torch.where(use_q, aQ, aI) - half


def SER_CMA(rx, tx, sps, amp_levels, num_lev, device=None):
    """:63-94: rescales rx IN PLACE by mean|tx| / mean|rx| (tx = the fp16 TX symbols), nearest-level decisions per axis, minimum SER over the
    0 / pi / pi/4 / 3pi/4 relabelings.  Batched over leading dims (returns one SER per leading index)."""
    N = tx.shape[-1]
    scale = (num_lev - 1) / 2
    t = tx.float()
    data = torch.round(scale * t + scale)
    rx *= (torch.mean(torch.sqrt(t[..., 0, :] ** 2 + t[..., 1, :] ** 2), -1) /
           torch.mean(torch.sqrt(rx[..., 0, :] ** 2 + rx[..., 1, :] ** 2), -1))[..., None, None]
    lev = amp_levels.reshape(-1, 1)
    dec = torch.stack([torch.argmin(torch.abs(rx[..., 0, :N].unsqueeze(-2) - lev), -2),
                       torch.argmin(torch.abs(rx[..., 1, :N].unsqueeze(-2) - lev), -2)], -2).float()
    dec_pi = -(dec - scale * 2)
    dec_pi4 = torch.stack([-(dec[..., 1, :] - scale * 2), dec[..., 0, :]], -2)
    dec_3pi4 = -(dec_pi4 - scale * 2)
    return torch.stack([((data - d) != 0).any(-2).float().mean(-1) for d in (dec, dec_pi, dec_pi4, dec_3pi4)], -1).min(-1).values


def cma_validate_torch(rx, h, data, amp_levels, sps=2, n_shift=N_SHIFT):
    """The evaluated epoch composed from the mirrors (:227-232): CMA(..., False) on the HIP kernel, then CPE, find_shift_symb and SER_CMA in
    torch, for R runs: rx[R,2,N], h[R,2,M], data[R,2,K] -> (SER[R], shift[R], CPE output [R,2,K]).  The cross-check of the fused kernel."""
    h = h.contiguous().clone()
    _, out, _ = awgn_cma(rx, h, 0.0, sps, update=False, want_out=True)
    y = CPE(out)
    shift = find_shift_symb(y, data, n_shift)
    amp = torch.as_tensor(amp_levels, dtype=torch.float32, device=rx.device).reshape(-1)
    num_lev = amp.numel()
    K = y.shape[-1]
    ser = torch.stack([SER_CMA(y[r, :, 11 + int(s):K - 11].clone(), data[r, :, 11:K - 11 - int(s)], sps, amp, num_lev)
                       for r, s in enumerate(shift.tolist())])
    return ser, shift, y


def run_awgn_cma_batch(runs, mod, sps, M_est, N_valid, N_train, num_epochs, epe, channel, device=None, verbose=False, generator=None,
                       seed=None, want_info=False, want_llr=False, fec=None):
    """R AWGN constant-modulus runs at once: ``runs`` = list of dict(SNR, nu, lr_optim, seed).  Per epoch ONE training launch (every run's
    per-symbol chain on its own wave) and, on evaluated epochs, ONE fused validation launch (:213-232).

    generator: None    = "hip" when no run carries a seed (the reference seeds nothing), else "numpy" (dp_runs.resolve_generator);
               "numpy" = the reference-faithful host channel model per run (seeded like tools/capture_golden.py when the run has a seed);
               "hip"   = the on-device generator (vaeq_gen_awgn), Philox streams keyed by ``seed``, the draw counter and the run index.
    Returns SER_valid[R, num_epochs // epe] (CPU float32); with want_info (SER_valid, info), info = dict(AIR, GMI, NGMI, BER f32; kept, sym_err,
    bit_err, hyp int64), each [R, num_epochs // epe] on the CPU: engine.awgn_track_info on the CPE output and the shift of every validation launch,
    demapped at var = 10^(-SNR/10), the VAE-LE's of the same sweep point (func_VAELE_MQAM_shaping.py:272).
    want_llr / fec: (SER_valid, info or None, extras), for the LAST evaluated validation only and on the device: with want_llr extras["llr"] =
    dict(llr[R,2b,N_valid] f32 = engine.awgn_track_llr on that validation's CPE output and shift, at the var and edge 11 of the info call and
    under its hyp, bits int8 = fec.label_bits of its TX data, hyp[R]); with fec = dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75,
    depth=None) extras["fec"] = fec.ldpc_decode's figures of those LLRs. A quant=dict(bits, ...) in fec decodes in fixed point (vaeq_ldpc_decode_q).  Both off: no output changes."""
    device = default_device() if device is None else torch.device(device)
    check_fec(fec)
    R = len(runs)
    generator = check_generator(resolve_generator(generator, any(r.get("seed") is not None for r in runs)))
    tabs, gen_args, host, seeded = awgn_batch_tables(runs, mod, sps, channel)
    amp = torch.tensor(gen_args[0], dtype=torch.float32, device=device)
    var = [t["var"] for t in tabs]
    h = torch.zeros(R, 2, M_est, dtype=torch.float32, device=device)
    h[:, 0, M_est // 2] = 1.0                                                    # :245-246
    lr = torch.tensor([r["lr_optim"] for r in runs], dtype=torch.float32, device=device)

    def validate(draw, N, soft=False):                                           # :222-232
        rxv, datav = draw(N)
        ser, sh, yv = awgn_cma_validate(rxv, h, datav, amp, sps, N_SHIFT, want_cpe=want_info or soft)
        if not soft:
            return ser, sh, awgn_track_info(yv, datav, amp, gen_args[1], var, sh, 11) if want_info else None
        info = awgn_track_info(yv, datav, amp, gen_args[1], var, sh, 11)
        return ser, sh, info, dict(llr=awgn_track_llr(yv, datav, amp, var, sh, info["hyp"], 11), bits=label_bits(datav, amp.numel()), hyp=info["hyp"])

    return run_awgn_epochs(R, device, num_epochs, epe, N_train, N_valid, lambda rx: awgn_cma(rx, h, lr, sps, update=True)[0], validate,   # :218-220
                           generator, seed, gen_args, host, seeded, verbose, want_info, want_llr, fec)


def processing(mod, sps, SNR, nu, M_est, lr_optim, N_valid, N_train, num_epochs, epe, channel, *, seed=None, device=None, verbose=True,
               generator=None, **options):
    """One AWGN constant-modulus run -> SER_valid[num_epochs//epe] (CPU float32); with want_info=True (SER_valid, info), info as
    run_awgn_cma_batch's per run.  The named keyword-only parameters are the pinned call surface of this drop-in (tests/test_awgn_cma_host.py);
    what the reference has no word for arrives through ``options``: want_info (default False), keyword-only like them, anything else a TypeError.
    NB no ``batch_len``: the positional order differs from
    func_VAELE_MQAM_shaping.processing (:201)."""
    want_info = bool(options.pop("want_info", False))
    if options:
        raise TypeError(f"processing() got an unexpected keyword argument {sorted(options)[0]!r}")
    device = default_device() if device is None else torch.device(device)
    if verbose:
        print("We are using the following device for learning:", device)
    out = run_awgn_cma_batch([dict(SNR=SNR, nu=nu, lr_optim=lr_optim, seed=seed)], mod, sps, M_est, N_valid, N_train, num_epochs, epe,
                             channel, device=device, verbose=verbose, generator=generator, want_info=want_info)
    return first_run(out, want_info)

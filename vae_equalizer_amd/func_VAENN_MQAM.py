"""Drop-in for AWGN_channel/func_VAENN_MQAM.py: same ``processing`` signature (:215) and return value (:304); the
training loop and the validation pass run on the HIP kernels (engine.NNEngine: vaeq_nn_train, vaeq_nn_validate).

Both topologies of the reference are implemented: ``net_type='Net'`` and ``'Net_BN'`` (BatchNorm1d between the ELU and fc2).

``Net`` and ``Net_BN`` (:170-211) are torch modules with the reference's constructor, submodule names and ``state_dict``; their forward and
backward passes are the HIP encoder kernels (autograd_ops.nn_encode: vaeq_nn_enc_forward / vaeq_nn_enc_backward), so the reference's loop
``net(minibatch) -> loss_function -> loss.backward() -> optimizer.step()`` runs unchanged.  ``processing`` does not use them: it trains with the
fused kernel.  ``net_to_theta`` / ``theta_to_net`` convert between a module plus h_est and the engine's flat vectors."""
import numpy as np
import torch
from torch import nn

from . import channel as ch
from .awgn_runs import check_generator, first_run, run_awgn_epochs
from .dp_runs import default_device
from .engine import NNEngine
from .fec import check_fec, label_bits
from .func_VAELE_MQAM_shaping import SER_q, SER_symb, find_shift  # noqa: F401  (identical helpers in both reference files)
from .shared_funcs import _CHANNELS, _LEVELS


def vaenn_tables(mod, channel, sps):
    """Constants processing() derives before the loop (:219-237): unit-power square QAM, its ASK levels, the upsampled unit-norm
    channel impulse response."""
    if channel not in ("h1", "h2"):
        raise UnboundLocalError(f"unknown channel {channel!r} (the reference leaves h_channel_orig unbound, :219-222)")
    ir = np.array(_CHANNELS[channel]).astype(np.complex64)
    h_channel = np.zeros(sps * (ir.shape[-1] - 1) + 1, dtype=np.complex64)
    h_channel[0::sps] = ir
    h_channel /= np.linalg.norm(h_channel)
    n = _LEVELS[mod]
    ask = np.arange(-(n - 1), n, 2).astype(np.float64)
    constellation = (ask[:, None] + 1j * ask[None, :]).reshape(-1)
    constellation = constellation / np.sqrt(np.mean(np.abs(constellation) ** 2))
    return dict(constellation=constellation, amps=constellation.real[::n], h_channel=h_channel, M_channel=len(ir), n=n)


def generate_data(N, M, constellation, SNR, h_channel, sps, device, rng=None):
    """Host restatement of generate_data (:39-61): uniform symbols, RRC + channel, AWGN of FIXED variance 1/(2 SNR).
    rng: a ``np.random.RandomState`` (the reference uses the global legacy stream for symbols and noise alike)."""
    rng = np.random if rng is None else rng
    T = ch.PULSE_SPAN
    N_conv = N + len(h_channel) + 4 * T
    data = rng.randint(len(constellation), size=N_conv)
    tx_sig = constellation[data]
    tx_up = np.zeros(sps * (N_conv - 1) + 1, dtype=np.complex64)
    tx_up[::sps] = tx_sig
    sig = np.convolve(np.convolve(tx_up, ch.rrcfir(T, sps, ch.ROLL_OFF), mode="valid"), h_channel, mode="valid")
    sigma_n = np.sqrt(1 / 2) / 10 ** (SNR / 20)
    sig = sig + sigma_n * (rng.randn(*sig.shape) + 1j * rng.randn(*sig.shape))
    lo = T + M - 1
    rx = np.stack([sig[:sps * N].real, sig[:sps * N].imag])
    ref = np.stack([tx_sig[lo:lo + N].real, tx_sig[lo:lo + N].imag])
    return (torch.from_numpy(np.ascontiguousarray(rx)).to(device, torch.float32),
            torch.from_numpy(np.ascontiguousarray(ref)).to(device, torch.float16))


def loss_function(q, rx, h, device, amp_levels):
    """ELBO of one minibatch (:63-95): q[2n,B], rx[2,B*sps], h[2,M] (HIP: vaeq_awgn_loss with the entropy term; differentiable in q, h and rx)."""
    if torch.is_grad_enabled() and (q.requires_grad or h.requires_grad or rx.requires_grad):
        from .autograd_ops import awgn_elbo_loss
        return awgn_elbo_loss(q, rx, h, amp_levels, None)
    from .engine import awgn_loss
    return awgn_loss(q, rx, h.detach(), amp_levels, None)


class _Encoder(nn.Module):
    """fc1 = Conv1d(2, C, k1, pad k1 // 2) -> ELU [-> batch1 = BatchNorm1d(C)] -> fc2 = Conv1d(C, C, k2, pad k2 // 2, stride sps) -> softmax per
    axis, C = 2 num_lev.  The submodules only hold the parameters and buffers (so that state_dict() has the reference's keys and shapes and
    checkpoints interchange in both directions); the arithmetic is the HIP kernels'.  The reference's residual x_res (:183-185) is the same
    for every level of an axis and cancels in the softmax: it is not computed."""
    _batch_norm = False

    def __init__(self, kernel_1, kernel_2, num_lev, sps):
        super().__init__()
        C_ = 2 * num_lev
        self.fc1 = nn.Conv1d(2, C_, kernel_1, bias=True, padding=kernel_1 // 2)
        self.fc2 = nn.Conv1d(C_, C_, kernel_2, bias=True, padding=kernel_2 // 2, stride=sps)
        if self._batch_norm:
            self.batch1 = nn.BatchNorm1d(C_)
            nn.init.kaiming_uniform_(self.fc1.weight)
        else:
            nn.init.xavier_uniform_(self.fc1.weight, gain=1)
        nn.init.xavier_uniform_(self.fc2.weight, gain=1)

    def _params(self):
        p = [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]
        return p + [self.batch1.weight, self.batch1.bias] if self._batch_norm else p

    def forward(self, x):
        """x[1,2,L] -> netout[1,2 num_lev,ceil(L/sps)] float32.  With autograd on and a parameter or x requiring a gradient the result carries the
        HIP-backed graph (x then receives its gradient too: vaeq_nn_enc_backward_x); self.training selects the BatchNorm mode, and a training-mode forward moves the running statistics (also under
        no_grad, as PyTorch does).  CPU tensors are refused."""
        from .autograd_ops import nn_encode
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[1] != 2:
            raise ValueError(f"x must be [1, 2, L], got {tuple(x.shape)}")
        if not self._batch_norm:
            return nn_encode(x, self._params(), self.fc2.stride[0])
        b = self.batch1
        q = nn_encode(x, self._params(), self.fc2.stride[0], True, self.training, b.running_mean, b.running_var)
        if self.training:
            b.num_batches_tracked += 1
        return q


class Net(_Encoder):
    """Net (:170-188): xavier_uniform_ on both convolution weights."""


class Net_BN(_Encoder):
    """Net_BN (:190-211): BatchNorm1d between the ELU and fc2, kaiming_uniform_ on fc1.weight."""
    _batch_norm = True


def net_to_theta(net, h_est):
    """(module, h_est[2,M]) -> (theta[NP] in NNEngine.offsets() order, bn[2C] = running_mean | running_var, or None for Net)."""
    parts = [p.detach().reshape(-1) for p in net._params()] + [h_est.detach().reshape(-1)]
    theta = torch.cat([p.to(torch.float32) for p in parts])
    bn = torch.cat([net.batch1.running_mean, net.batch1.running_var]).to(torch.float32) if net._batch_norm else None
    return theta, bn


def theta_to_net(theta, net, bn=None):
    """Load one run's flat engine vector theta[NP] (and bn[2C] for Net_BN) into the module, in place -> h_est[2,M] (a new tensor)."""
    theta = torch.as_tensor(theta).detach().reshape(-1)
    params = net._params()
    sizes = [p.numel() for p in params]
    n_net = sum(sizes)
    if theta.numel() <= n_net or (theta.numel() - n_net) % 2:
        raise ValueError(f"theta has {theta.numel()} entries; the network alone takes {n_net}, h_est an even number more")
    with torch.no_grad():
        for p, v in zip(params, torch.split(theta[:n_net], sizes)):
            p.copy_(v.reshape(p.shape))
        if net._batch_norm and bn is not None:
            bn = torch.as_tensor(bn).detach().reshape(2, -1)
            net.batch1.running_mean.copy_(bn[0])
            net.batch1.running_var.copy_(bn[1])
    return theta[n_net:].reshape(2, -1).to(torch.float32).clone()


def run_vaenn_batch(runs, mod, sps, M_est, kernel_1, kernel_2, batch_len, N_valid, N_train, num_epochs, epe, channel, device=None,
                    verbose=False, generator="hip", seed=0, theta0=None, net_type="Net", want_info=False, want_llr=False, fec=None):
    """R VAE-NN runs at once: ``runs`` = list of dict(SNR, lr_optim, seed).  Per epoch one generator call, ONE training launch
    (N_train // batch_len minibatches) and, on evaluated epochs, one fused validation launch for all runs (:266-301).

    generator: "hip" = on-device channel model (vaeq_gen_awgn with the script's fixed noise level), Philox streams keyed by ``seed``;
               "numpy" = the host restatement per run, seeded per run when the run has a seed.
    theta0: optional [R, NP] initial parameters (default: Xavier / PyTorch-default initialisation drawn on the device).
    Returns SER_valid[R, num_epochs // epe] (CPU float32); with want_info (SER_valid, info), info = dict(AIR, GMI, NGMI, BER f32; kept, sym_err,
    bit_err, hyp int64), each [R, num_epochs // epe] on the CPU: NNEngine.info (eval forward, then engine.awgn_info in q-mode, uniform pmf) on the
    frame and the shift of every validation launch.
    want_llr / fec: (SER_valid, info or None, extras), for the LAST evaluated validation only and on the device: with want_llr extras["llr"] =
    dict(llr[R,2b,N_valid] f32 = NNEngine.llr on that validation's frame and shift under the hyp of NNEngine.info on them, bits int8 =
    fec.label_bits of its TX data, hyp[R]); with fec = dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75, depth=None) extras["fec"] =
    fec.ldpc_decode's figures of those LLRs. A quant=dict(bits, ...) in fec decodes in fixed point (vaeq_ldpc_decode_q).  Both off: no output changes."""
    device = default_device() if device is None else torch.device(device)
    R = len(runs)
    t = vaenn_tables(mod, channel, sps)
    if net_type not in ("Net", "Net_BN"):
        raise UnboundLocalError(f"unknown net_type {net_type!r} (the reference leaves `net` unbound, :239-243)")
    check_generator(generator)
    check_fec(fec)
    eng = NNEngine(R, M_est, kernel_1, kernel_2, t["amps"], device, sps, batch_norm=(net_type == "Net_BN"))
    if theta0 is None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed) + 12345)
        eng.init_parameters(gen)
    else:
        eng.init_parameters()
        eng.theta.copy_(torch.as_tensor(theta0, dtype=torch.float32, device=device).expand(R, -1))
    lr = np.array([r["lr_optim"] for r in runs], dtype=np.float32)
    snr = np.array([r["SNR"] for r in runs], dtype=np.float32)
    rngs = [np.random.RandomState(r["seed"]) if r.get("seed") is not None else None for r in runs]
    steps = N_train // batch_len

    def validate(draw, N, soft=False):
        rxv, datav = draw(N)
        ser, sh = eng.validate(rxv, datav, 21)
        if not soft:
            return ser, sh, eng.info(rxv, datav, sh) if want_info else None
        info = eng.info(rxv, datav, sh)
        return ser, sh, info, dict(llr=eng.llr(rxv, sh, info["hyp"]), bits=label_bits(datav, t["n"]), hyp=info["hyp"])

    return run_awgn_epochs(R, device, num_epochs, epe, N_train, N_valid, lambda rx: eng.train(rx, batch_len, steps, lr)["loss"][:, -1], validate,
                           generator, seed, (t["amps"], np.full(t["n"], 1.0 / t["n"]), snr, t["h_channel"], sps),
                           lambda N, i: generate_data(N, t["M_channel"], t["constellation"], runs[i]["SNR"], t["h_channel"], sps, "cpu", rngs[i]),
                           all(g is not None for g in rngs), verbose, want_info, want_llr, fec, sigma_fixed=np.sqrt(0.5) / 10 ** (snr / 20))


def processing(mod, sps, SNR, M_est, kernel_1, kernel_2, lr_optim, batch_len, N_valid, N_train, num_epochs, epe, channel, net_type, *,
               seed=None, device=None, verbose=True, generator="numpy", theta0=None, want_info=False):
    """One VAE-NN run -> SER_valid[num_epochs//epe] (CPU float32), the reference's positional signature (:215); with want_info
    (SER_valid, info), info as run_vaenn_batch's per run."""
    device = default_device() if device is None else torch.device(device)
    if verbose:
        print("We are using the following device for learning:", device)
    out = run_vaenn_batch([dict(SNR=SNR, lr_optim=lr_optim, seed=seed)], mod, sps, M_est, kernel_1, kernel_2, batch_len, N_valid, N_train,
                          num_epochs, epe, channel, device=device, verbose=verbose, generator=generator, seed=seed or 0, theta0=theta0,
                          net_type=net_type, want_info=want_info)
    return first_run(out, want_info)

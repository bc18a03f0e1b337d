"""Batched run engines: device-resident state of R independent equalizer runs + launches of the HIP training loop.

This is the host side of the C ABI (include/vaeq.h).  It mirrors what one call of the reference's
``processing()`` keeps alive between minibatches -- the ``twoXtwoFIR`` weight, ``h_est`` and the two
``optim.Adam`` parameter groups (optical_DP_channel/func_VAELE_DP_MQAM_shaping.py:26-31) -- for R runs at
once, because on an MI355X the sweep (Eval_run_DP.py:68-86), not the single run, is the unit of parallelism.
"""
import ctypes as C
import math

import torch

from . import _native as nat
from .fec import (  # noqa: F401  (the FEC host layer lives in fec.py; its public names stay importable from here)
    FEC_BLOCK_ONLY, FEC_KEYS, FEC_SC_ONLY, FEC_STAIRCASE_KEYS, FEC_TPC_KEYS, INNER_KEYS, OUTER_KEYS, OUTER_POST_BYTES, QUANT_KEYS, TPC_ALPHA, TPC_BETA,
    TPC_CLIP, BchCode, EbchCode, HammingCode, LdpcCode, ProductCode, ScLdpcCode, StaircaseCode, array_code, bch_outer, chase_decode, check_fec,
    ebch_code, fec_figures, hamming_code, label_bits, ldpc_decode, ldpc_sc_decode, resolve_inner, resolve_outer, resolve_quant, resolve_tpc,
    sc_array_code, staircase_decode, tpc_decode)


INFO_FLOAT, INFO_INT = ("AIR", "GMI", "NGMI", "BER"), ("kept", "sym_err", "bit_err", "hyp")   # the keys of the info dicts: float32 figures, int64 counts


def _f32(x, device):
    return torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()


def _per_run(x, R, shape, device):
    """One value per run: x of ``shape`` (shared by the R runs) or [R, *shape] -> contiguous float32 [R, *shape]."""
    t = _f32(x, device)
    if t.dim() == len(shape):
        t = t.expand(R, *shape)
    if tuple(t.shape) != (R, *shape):
        raise ValueError(f"expected shape {(R, *shape)} or {shape}, got {tuple(t.shape)}")
    return t.contiguous()


def _amp(amp_levels, dev):
    return _f32(amp_levels, dev).reshape(-1)


def _pmf(P, R, n, dev):                                  # the per-axis pmf [n] or [R,n] -> [R,n]
    return _f32(P, dev).reshape(-1, n).expand(R, n).contiguous()


def _var_nu(var, nu_sc, R, dev):                         # the soft demapper's constants: var [2] or [R,2] -> [R,2], nu_sc scalar or [R] -> [R]
    return _f32(var, dev).expand(R, 2).contiguous(), _f32(nu_sc, dev).expand(R).contiguous()


def _i32(t, shape, dev):
    return torch.as_tensor(t, device=dev).to(torch.int32).reshape(shape).contiguous()


def _f16(data):
    return data.to(torch.float16).contiguous()


def _posterior_source(who, q, y, amp_levels, lead, data):
    """What the information-rate and LLR functions of a DP frame (lead = (2,)) and of an AWGN validation frame (lead = ()) take: exactly one of
    q[R,*lead,2n,N] and y[R,*lead,2,N], and data[R,*lead,2,N] where the function reads it (None otherwise) ->
    (dev, R, N, n, amp[n], q or None, y or None, data fp16 or None), contiguous."""
    if (q is None) == (y is None):
        raise ValueError(f"{who} takes exactly one of q and y")
    src = q if y is None else y
    dev, R, N = src.device, src.shape[0], src.shape[-1]
    amp = _amp(amp_levels, dev)
    n = amp.numel()
    if tuple(src.shape) != (R, *lead, 2 * n if y is None else 2, N) or (data is not None and tuple(data.shape) != (R, *lead, 2, N)):
        raise ValueError(f"expected q{[R, *lead, 2 * n, N]} or y{[R, *lead, 2, N]} and data{[R, *lead, 2, N]}, got {tuple(src.shape)}"
                         + ("" if data is None else f", {tuple(data.shape)}"))
    src = src.contiguous()
    return dev, R, N, n, amp, (src if y is None else None), (src if y is not None else None), None if data is None else _f16(data)


def _dp_frame(who, q, y, data, amp_levels, nu_sc, var, shift, r):
    """The arguments dp_epilogue_info and dp_epilogue_llr share -> (dev, R, N, n, amp, q, y, data, var[R,2], nu_sc[R] (None in q-mode),
    shift[R,2] i32, r[R] i32)."""
    dev, R, N, n, amp, q, y, data = _posterior_source(who, q, y, amp_levels, (2,), data)
    var_t, nu_t = (None, None) if y is None else _var_nu(var, nu_sc, R, dev)
    return dev, R, N, n, amp, q, y, data, var_t, nu_t, _i32(shift, (R, 2), dev), _i32(r, R, dev)


def _awgn_frame(who, q, y, data, amp_levels, amp_mean, var, shift):
    """The arguments awgn_info and awgn_llr share -> (dev, R, N, n, amp, q, y, data, amp_mean[R], var[R] (None in q-mode), shift[R] i32)."""
    dev, R, N, n, amp, q, y, data = _posterior_source(who, q, y, amp_levels, (), data)
    am_t, var_t = (None, None) if y is None else (_f32(amp_mean, dev).expand(R).contiguous(), _f32(var, dev).expand(R).contiguous())
    return dev, R, N, n, amp, q, y, data, am_t, var_t, _i32(shift, R, dev)


def _cma_frame(y, data, amp_levels, nu_sc, var, shift_c, r_c, shift_q, r_q):
    """The arguments cma_epilogue_info and cma_epilogue_llr share -> (dev, R, N, n, amp, y, data fp16, var[R,2], nu_sc[R], and the four alignment
    outputs as int32: shift_c[R,2], r_c[R], shift_q[R,2], r_q[R])."""
    dev, R, N = y.device, y.shape[0], y.shape[-1]
    amp = _amp(amp_levels, dev)
    if tuple(y.shape) != (R, 2, 2, N) or tuple(data.shape) != (R, 2, 2, N):
        raise ValueError(f"expected y[R,2,2,N] and data[R,2,2,N], got {tuple(y.shape)}, {tuple(data.shape)}")
    var_t, nu_t = _var_nu(var, nu_sc, R, dev)
    return (dev, R, N, amp.numel(), amp, y.contiguous(), _f16(data), var_t, nu_t,
            _i32(shift_c, (R, 2), dev), _i32(r_c, R, dev), _i32(shift_q, (R, 2), dev), _i32(r_q, R, dev))


def _track(z, data, amp_levels, var, shift):
    """The arguments awgn_track_info and awgn_track_llr share: z float [R,2,Nz] (planar) or complex [R,Nz] (interleaved: the layout follows from
    the dtype), data[R,2,Nd] -> (dev, R, Nz, Nd, n, interleaved, amp, z float32, data fp16, var[R], shift[R] i32)."""
    dev, R = z.device, z.shape[0]
    amp = _amp(amp_levels, dev)
    interleaved = z.is_complex()
    if interleaved:
        z = torch.view_as_real(z.to(torch.complex64).contiguous())
    Nz, Nd = (z.shape[1] if interleaved else z.shape[-1]), data.shape[-1]
    if tuple(z.shape) != ((R, Nz, 2) if interleaved else (R, 2, Nz)) or tuple(data.shape) != (R, 2, Nd):
        raise ValueError(f"expected z[R,2,Nz] float or z[R,Nz] complex and data[R,2,Nd], got {tuple(z.shape)}, {tuple(data.shape)}")
    return (dev, R, Nz, Nd, amp.numel(), interleaved, amp, z.float().contiguous(), _f16(data), _f32(var, dev).expand(R).contiguous(),
            _i32(shift, R, dev))


def _alignment_out(R, dev):
    """What an epilogue launch writes: SER[R,4] f32, shift[R,2,2] i32 and the exchange flags [R,2] i32 (stage q, then stage c)."""
    e = lambda *s, dtype=torch.int32: torch.empty(R, *s, dtype=dtype, device=dev)
    return e(4, dtype=torch.float32), e(2, 2), e(2)


def _alignment_dict(ser, shift, rflag):
    return dict(SER=ser, shift_q=shift[:, 0].long(), r_q=rflag[:, 0].long(), shift_c=shift[:, 1].long(), r_c=rflag[:, 1].long())


def _info_dict(info, counts, P):
    """An info kernel's info[..., 3] = (AIR, GMI, BER) and counts[..., 4] -> the dict of INFO_FLOAT + INFO_INT, with NGMI = 1 - (2 H - GMI) / (2 log2 n)
    formed here in float32 from the entropy H of P[R,n]."""
    H = -(P * torch.where(P > 0, torch.log2(P.clamp_min(torch.finfo(torch.float32).tiny)), torch.zeros_like(P))).sum(1, keepdim=info.dim() == 3)
    gmi = info[..., 1]
    return dict(AIR=info[..., 0], GMI=gmi, NGMI=1.0 - (2.0 * H - gmi) / (2.0 * math.log2(P.shape[1])), BER=info[..., 2],
                kept=counts[..., 0].long(), sym_err=counts[..., 1].long(), bit_err=counts[..., 2].long(), hyp=counts[..., 3].long())


class DPEngine:
    """R dual-polarisation runs (VAE-LE or VAEflex) sharing modulation, M_est and sps; P/var/nu_sc/lr per run."""

    def __init__(self, R, M_est, amp_levels, P, var, nu_sc, device="cuda:0", sps=2, threads=0):
        if M_est % 2 == 0:
            # even M_est: FIR yields B+1 outputs and the loss indexes M_est+1 taps in the reference (SURVEY note N3)
            raise ValueError("M_est must be odd")
        self.device = torch.device(device)
        self.R, self.M, self.sps, self.threads = int(R), int(M_est), int(sps), int(threads)
        self.amp = _amp(amp_levels, self.device)
        self.n_lev = self.amp.numel()
        self.P = _per_run(P, self.R, (self.n_lev,), self.device)
        self.var = _per_run(var, self.R, (2,), self.device)
        self.nu_sc = _per_run(nu_sc, self.R, (), self.device)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
        self.W, self.h = z(R, 2, 4, self.M), z(R, 2, 2, 2, self.M)
        self.mW, self.vW, self.mh, self.vh = z(R, 2, 4, self.M), z(R, 2, 4, self.M), z(R, 2, 2, 2, self.M), z(R, 2, 2, 2, self.M)
        self.step = torch.zeros(R, dtype=torch.int32, device=self.device)
        self.reset()

    def reset(self):
        """Dirac initialisation of W (shared_funcs.py:495) and h_est (:585); Adam state zeroed."""
        for t in (self.W, self.h, self.mW, self.vW, self.mh, self.vh):
            t.zero_()
        self.step.zero_()
        c = self.M // 2
        self.W[:, 0, 0, c] = 1.0
        self.W[:, 1, 1, c] = 1.0
        self.h[:, 0, 0, 0, c] = 1.0
        self.h[:, 1, 1, 0, c] = 1.0

    def set_state(self, W=None, h=None):
        if W is not None:
            self.W.copy_(_f32(W, self.device).expand_as(self.W))
        if h is not None:
            self.h.copy_(_f32(h, self.device).expand_as(self.h))

    _STATE = ("W", "h", "mW", "vW", "mh", "vh", "step")

    def state_dict(self):
        """Everything a run carries from one minibatch to the next (taps, channel estimate, both Adam groups' moments, step counts), on the
        CPU: a sweep can be checkpointed between frames and resumed bit-identically (the reference persists nothing mid-run)."""
        return {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}

    def load_state_dict(self, sd):
        for k in self._STATE:
            t = getattr(self, k)
            if tuple(sd[k].shape) != tuple(t.shape) or sd[k].dtype != t.dtype:
                raise ValueError(f"state {k!r}: expected {tuple(t.shape)} {t.dtype}, got {tuple(sd[k].shape)} {sd[k].dtype}")
            t.copy_(sd[k].to(self.device))

    def train(self, rx, B, steps, lr_W, lr_h=None, stride=None, keep_off=0, keep_len=None, want_q=True, want_y=True,
              want_loss=True, debug_grads=False, no_update=False, want_compact=False):
        """Run ``steps`` minibatch steps per frame on rx[R, n_frames, 2, 2, S] (or [R, 2, 2, S]).

        VAE-LE: defaults (stride = keep_len = B).  VAEflex: stride = keep_len = flex_step, keep_off = (B-flex_step)//2.
        Returns dict of device tensors: q [R,F,2,2n,steps*keep_len], y [R,F,2,2,...], loss [R,F,steps], var_est [R,F,2,steps].
        want_compact adds eq [R,F,2,No] (E_q[x_I] per polarisation) and dec [R,F,2,2,No] int8 (argmax of q per axis): everything the
        per-frame epilogue reads of q, so a sweep can run with want_q=False (dp_epilogue_compact).
        """
        if rx.dim() == 4:
            rx = rx.unsqueeze(1)
        R, F, S = rx.shape[0], rx.shape[1], rx.shape[-1]
        if R != self.R or tuple(rx.shape[2:4]) != (2, 2):
            raise ValueError(f"rx must be [R={self.R}, F, 2, 2, S], got {tuple(rx.shape)}")
        stride = B if stride is None else stride
        keep_len = B if keep_len is None else keep_len
        lr_h = lr_W if lr_h is None else lr_h
        lrW, lrH = _per_run(lr_W, R, (), self.device), _per_run(lr_h, R, (), self.device)
        No = steps * keep_len
        dev = self.device
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = {
            "q": e(R, F, 2, 2 * self.n_lev, No) if want_q else None,
            "y": e(R, F, 2, 2, No) if want_y else None,
            "loss": e(R, F, steps) if want_loss else None,
            "var_est": e(R, F, 2, steps) if want_loss else None,
            "gW": e(R, 2, 4, self.M) if debug_grads else None,
            "gh": e(R, 2, 2, 2, self.M) if debug_grads else None,
            "eq": e(R, F, 2, No) if want_compact else None,
            "dec": torch.empty(R, F, 2, 2, No, dtype=torch.int8, device=dev) if want_compact else None,
        }
        a = nat.DPArgs(R=R, n_frames=F, steps=steps, B=B, sps=self.sps, M=self.M, n_lev=self.n_lev, stride_sym=stride,
                       keep_off=keep_off, keep_len=keep_len, S=S, rx=nat.ptr(rx), W=nat.ptr(self.W), h=nat.ptr(self.h),
                       adam_mW=nat.ptr(self.mW), adam_vW=nat.ptr(self.vW), adam_mh=nat.ptr(self.mh), adam_vh=nat.ptr(self.vh),
                       step=nat.ptr(self.step, torch.int32), amp=nat.ptr(self.amp), P=nat.ptr(self.P), var=nat.ptr(self.var),
                       nu_sc=nat.ptr(self.nu_sc), lr_W=nat.ptr(lrW), lr_h=nat.ptr(lrH), q_out=nat.ptr(out["q"]),
                       y_out=nat.ptr(out["y"]), loss=nat.ptr(out["loss"]), var_est=nat.ptr(out["var_est"]),
                       eq_out=nat.ptr(out["eq"]), dec_out=nat.ptr(out["dec"], torch.int8),
                       dbg_gW=nat.ptr(out["gW"]), dbg_gh=nat.ptr(out["gh"]), threads=self.threads, no_update=int(no_update))
        with torch.cuda.device(dev):
            nat.check(nat.lib().vaeq_dp_train(C.byref(a), nat.current_stream(dev)), "vaeq_dp_train")
        out["_keepalive"] = (lrW, lrH, rx)
        return out


def pad_to_symbols(x, sps):
    """Zero-pad the last axis of x to ceil(L / sps) * sps samples.  The reference's Conv1d(padding=M//2, stride=sps) yields ceil(L / sps)
    outputs and reads zeros past the end, so the padded block gives exactly its outputs; the FIR kernels take whole symbols."""
    r = x.shape[-1] % sps
    return x if r == 0 else torch.nn.functional.pad(x, (0, sps - r))


def soft_demap(y, amp_levels, var, nu_sc):
    """soft_dec on device: y[R,2,2,N] (or [2,2,N]) -> q[R,2,2n,N]."""
    squeeze = y.dim() == 3
    if squeeze:
        y = y.unsqueeze(0)
    dev, R, N = y.device, y.shape[0], y.shape[-1]
    amp = _amp(amp_levels, dev)
    n = amp.numel()
    var, nu = _var_nu(var, nu_sc, R, dev)
    y = y.contiguous()
    q = torch.empty(R, 2, 2 * n, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_soft_demap(R, N, n, nat.ptr(y), nat.ptr(amp), nat.ptr(var), nat.ptr(nu), nat.ptr(q),
                                            nat.current_stream(dev)), "vaeq_soft_demap")
    return q[0] if squeeze else q


def dp_forward(x, W, amp_levels, var, nu_sc, sps=2, want_q=True):
    """twoXtwoFIR.forward (eval) on device: x[R,2,2,L], W[R,2,4,M] -> (q[R,2,2n,N] or None, y[R,2,2,N]), N = ceil(L / sps)."""
    squeeze = x.dim() == 3
    if squeeze:
        x, W = x.unsqueeze(0), W.unsqueeze(0)
    x = pad_to_symbols(x, sps)
    dev, R = x.device, x.shape[0]
    N, M = x.shape[-1] // sps, W.shape[-1]
    amp = _amp(amp_levels, dev)
    n = amp.numel()
    var, nu = _var_nu(var, nu_sc, R, dev)
    x, W = x.contiguous(), W.contiguous()
    q = torch.empty(R, 2, 2 * n, N, dtype=torch.float32, device=dev) if want_q else None
    y = torch.empty(R, 2, 2, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_forward(R, N, sps, M, n, nat.ptr(x), nat.ptr(W), nat.ptr(amp), nat.ptr(var), nat.ptr(nu),
                                            nat.ptr(q), nat.ptr(y), nat.current_stream(dev)), "vaeq_dp_forward")
    if squeeze:
        return (q[0] if want_q else None), y[0]
    return q, y


def dp_loss(q, rx, h, amp_levels, P):
    """loss_function_shaping values on device: q[R,2,2n,B], rx[R,2,2,B*sps], h[R,2,2,2,M] (or unbatched) -> (loss, var_est)."""
    squeeze = q.dim() == 3
    if squeeze:
        q, rx, h = q.unsqueeze(0), rx.unsqueeze(0), h.unsqueeze(0)
    dev, R, B = q.device, q.shape[0], q.shape[-1]
    sps, M = rx.shape[-1] // B, h.shape[-1]
    amp = _amp(amp_levels, dev)
    n = amp.numel()
    Pt = _f32(P, dev)
    Pt = (Pt.expand(R, n) if Pt.dim() == 1 else Pt).contiguous()
    q, rx, h = q.contiguous(), rx.contiguous(), h.contiguous()
    loss = torch.empty(R, dtype=torch.float32, device=dev)
    ve = torch.empty(R, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_loss(R, B, sps, M, n, nat.ptr(q), nat.ptr(rx), nat.ptr(h), nat.ptr(amp), nat.ptr(Pt),
                                         nat.ptr(loss), nat.ptr(ve), nat.current_stream(dev)), "vaeq_dp_loss")
    return (loss[0], ve[0]) if squeeze else (loss, ve)


class AWGNEngine:
    """R single-polarisation VAE-LE runs (AWGN_channel/func_VAELE_MQAM_shaping.py:275-286): twoFIR weight, h_est and the
    two Adam(amsgrad=True) groups, device-resident."""

    def __init__(self, R, M_est, amp_levels, P, amp_mean, var, device="cuda:0", sps=2, threads=0):
        if M_est % 2 == 0:
            raise ValueError("M_est must be odd")
        self.device = torch.device(device)
        self.R, self.M, self.sps, self.threads = int(R), int(M_est), int(sps), int(threads)
        self.amp = _amp(amp_levels, self.device)
        self.n_lev = self.amp.numel()
        pr = lambda x, shape: _per_run(x, self.R, shape, self.device)
        self.P, self.amp_mean, self.var = pr(P, (self.n_lev,)), pr(amp_mean, ()), pr(var, ())
        z = lambda: torch.zeros(R, 2, self.M, dtype=torch.float32, device=self.device)
        self.W, self.h = z(), z()
        self.mW, self.vW, self.xW, self.mh, self.vh, self.xh = z(), z(), z(), z(), z(), z()
        self.step = torch.zeros(R, dtype=torch.int32, device=self.device)
        self.W[:, 0, self.M // 2] = 1.0   # nn.init.dirac_ (:210)
        self.h[:, 0, self.M // 2] = 1.0   # (:279)

    def set_state(self, W=None, h=None):
        if W is not None:
            self.W.copy_(_f32(W, self.device).reshape(-1, 2, self.M).expand_as(self.W))
        if h is not None:
            self.h.copy_(_f32(h, self.device).expand_as(self.h))

    def train(self, rx, B, steps, lr, want_q=False, want_y=False, debug_grads=False, no_update=False):
        """rx[R,2,S] -> dict(loss[R,steps], q[R,2n,steps*B]?, y[R,2,steps*B]?, gW?, gh?)."""
        R, S = rx.shape[0], rx.shape[-1]
        if R != self.R or rx.shape[1] != 2:
            raise ValueError(f"rx must be [R={self.R}, 2, S], got {tuple(rx.shape)}")
        lr_t = _per_run(lr, R, (), self.device)
        dev = self.device
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = {"loss": e(R, steps), "q": e(R, 2 * self.n_lev, steps * B) if want_q else None,
               "y": e(R, 2, steps * B) if want_y else None, "gW": e(R, 2, self.M) if debug_grads else None,
               "gh": e(R, 2, self.M) if debug_grads else None}
        a = nat.AWGNArgs(R=R, steps=steps, B=B, sps=self.sps, M=self.M, n_lev=self.n_lev, S=S, rx=nat.ptr(rx), W=nat.ptr(self.W),
                         h=nat.ptr(self.h), adam_mW=nat.ptr(self.mW), adam_vW=nat.ptr(self.vW), adam_xW=nat.ptr(self.xW),
                         adam_mh=nat.ptr(self.mh), adam_vh=nat.ptr(self.vh), adam_xh=nat.ptr(self.xh),
                         step=nat.ptr(self.step, torch.int32), amp=nat.ptr(self.amp), P=nat.ptr(self.P),
                         amp_mean=nat.ptr(self.amp_mean), var=nat.ptr(self.var), lr=nat.ptr(lr_t), q_out=nat.ptr(out["q"]),
                         y_out=nat.ptr(out["y"]), loss=nat.ptr(out["loss"]), dbg_gW=nat.ptr(out["gW"]), dbg_gh=nat.ptr(out["gh"]),
                         threads=self.threads, no_update=int(no_update))
        with torch.cuda.device(dev):
            nat.check(nat.lib().vaeq_awgn_train(C.byref(a), nat.current_stream(dev)), "vaeq_awgn_train")
        out["_keepalive"] = (lr_t, rx)
        return out

    def forward(self, x, want_q=True):
        """Validation pass (:313): x[R,2,L] -> (q[R,2n,N] or None, y[R,2,N]), N = ceil(L / sps) like the reference's Conv1d."""
        x = pad_to_symbols(x, self.sps).contiguous()
        R, N = x.shape[0], x.shape[-1] // self.sps
        q = torch.empty(R, 2 * self.n_lev, N, dtype=torch.float32, device=self.device) if want_q else None
        y = torch.empty(R, 2, N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().vaeq_awgn_forward(R, N, self.sps, self.M, self.n_lev, nat.ptr(x), nat.ptr(self.W), nat.ptr(self.amp),
                                                  nat.ptr(self.amp_mean), nat.ptr(self.var), nat.ptr(q), nat.ptr(y),
                                                  nat.current_stream(self.device)), "vaeq_awgn_forward")
        return q, y

    def validate(self, x, data, n_shift=21):
        """Fused validation pass (:308-318) -> (SER[R] f32, shift[R] i32, y[R,2,N]): forward, find_shift and SER_q in one
        kernel (vaeq_awgn_validate; rows of 23 + n_shift // 2 <= N < 64 symbols: vaeq_awgn_validate_short, the same kernel);
        x[R,2,N*sps] f32, data[R,2,N] f16."""
        R, N = x.shape[0], x.shape[-1] // self.sps
        if tuple(data.shape) != (R, 2, N):
            raise ValueError(f"data must be [R={R}, 2, N={N}], got {tuple(data.shape)}")
        x, data = x.contiguous(), data.contiguous()
        ser = torch.empty(R, dtype=torch.float32, device=self.device)
        shift = torch.empty(R, dtype=torch.int32, device=self.device)
        y = torch.empty(R, 2, N, dtype=torch.float32, device=self.device)
        short = 23 + int(n_shift) // 2 <= N < 64
        fn, what = (nat.lib().vaeq_awgn_validate_short, "vaeq_awgn_validate_short") if short else (nat.lib().vaeq_awgn_validate, "vaeq_awgn_validate")
        with torch.cuda.device(self.device):
            nat.check(fn(R, N, self.sps, self.M, self.n_lev, int(n_shift), nat.ptr(x), nat.ptr(self.W), nat.ptr(self.amp), nat.ptr(self.amp_mean),
                         nat.ptr(self.var), nat.ptr(data, torch.float16), nat.ptr(y), nat.ptr(ser), nat.ptr(shift, torch.int32),
                         nat.current_stream(self.device)), what)
        return ser, shift, y

    def validate_clean(self, frame, n_shift=21, return_sigma=False):
        """validate() on a channel.CleanAwgnFrame: the noise of the frame's (seed, frame index) is added while the samples are staged
        (vaeq_awgn_validate_gen) -- bit for bit validate(*generate_awgn_batch_hip(...)) without the noisy frame's round trip through HBM."""
        R, N = frame.R, frame.N
        if R != self.R or frame.sps != self.sps:
            raise ValueError(f"frame of {R} runs at {frame.sps} sps for an engine of {self.R} runs at {self.sps} sps")
        ser = torch.empty(R, dtype=torch.float32, device=self.device)
        shift = torch.empty(R, dtype=torch.int32, device=self.device)
        y = torch.empty(R, 2, N, dtype=torch.float32, device=self.device)
        sigma = torch.empty(R, dtype=torch.float32, device=self.device) if return_sigma else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().vaeq_awgn_validate_gen(R, N, self.sps, self.M, self.n_lev, int(n_shift), nat.ptr(frame.sig), frame.Ls,
                                                       nat.ptr(frame.power), nat.ptr(frame.snr),
                                                       None if frame.sigma_fixed is None else nat.ptr(frame.sigma_fixed),
                                                       C.c_uint64(frame.seed), C.c_uint32(frame.frame), nat.ptr(self.W), nat.ptr(self.amp),
                                                       nat.ptr(self.amp_mean), nat.ptr(self.var), nat.ptr(frame.data, torch.float16), nat.ptr(y),
                                                       nat.ptr(ser), nat.ptr(shift, torch.int32), None if sigma is None else nat.ptr(sigma),
                                                       nat.current_stream(self.device)), "vaeq_awgn_validate_gen")
        return (ser, shift, y, sigma) if return_sigma else (ser, shift, y)

    def info(self, y, data, shift):
        """GMI, NGMI, achievable rate and pre-FEC BER of a validation frame (awgn_info, y-mode) from what validate / validate_clean return:
        y[R,2,N], data[R,2,N] f16 and shift[R], demapped with the engine's P, amp_mean and var."""
        return awgn_info(y=y, data=data, amp_levels=self.amp, P=self.P, amp_mean=self.amp_mean, var=self.var, shift=shift)

    def llr(self, y, shift, hyp):
        """Per-bit LLRs of a validation frame (awgn_llr, y-mode) [R,2b,N]: y[R,2,N] and shift[R] from validate / validate_clean, hyp[R] from info on
        them, demapped with the engine's amp_mean and var -- the posteriors whose GMI info reports."""
        return awgn_llr(y=y, amp_levels=self.amp, amp_mean=self.amp_mean, var=self.var, shift=shift, hyp=hyp)


class NNEngine:
    """R independent AWGN VAE-NN runs (AWGN_channel/func_VAENN_MQAM.py): flat per-run parameter vectors
    theta = [fc1.weight | fc1.bias | fc2.weight | fc2.bias | h_est] and their AMSGrad state on the device."""

    def __init__(self, R, M_est, kernel_1, kernel_2, amp_levels, device="cuda:0", sps=2, batch_norm=False):
        self.device = torch.device(device)
        self.amp = _f32(amp_levels, self.device).reshape(-1).contiguous()
        self.R, self.M, self.k1, self.k2, self.sps, self.n_lev = int(R), int(M_est), int(kernel_1), int(kernel_2), int(sps), self.amp.numel()
        self.batch_norm = bool(batch_norm)                      # Net_BN (:190-211): theta gains [gamma | beta], bn = running statistics
        C_ = 2 * self.n_lev
        self.bn = torch.cat([torch.zeros(self.R, C_), torch.ones(self.R, C_)], 1).to(self.device).contiguous() if self.batch_norm else None
        NP = int(nat.lib().vaeq_nn_param_count(self.M, self.n_lev, self.k1, self.k2, int(self.batch_norm)))
        if NP < 0:
            raise ValueError(f"unsupported VAE-NN shape M={M_est} k1={kernel_1} k2={kernel_2} n_lev={self.n_lev}: "
                             + nat.lib().vaeq_strerror(NP).decode())
        self.NP = NP
        z = lambda: torch.zeros(self.R, NP, dtype=torch.float32, device=self.device)
        self.theta, self.m, self.v, self.vmax = z(), z(), z(), z()
        self.step = torch.zeros(self.R, dtype=torch.int32, device=self.device)

    def offsets(self):
        C_ = 2 * self.n_lev
        o = [0, C_ * 2 * self.k1]
        o += [o[-1] + C_, o[-1] + C_ + C_ * C_ * self.k2]
        o += [o[-1] + C_]
        if self.batch_norm:
            o += [o[-1] + C_, o[-1] + 2 * C_]
        o += [o[-1] + 2 * self.M]
        return o

    def init_parameters(self, generator=None):
        """nn.init.xavier_uniform_ on both conv weights, PyTorch's default uniform(+-1/sqrt(fan_in)) on the biases (:172-176), Dirac
        h_est (:244-246), independently per run."""
        C_, o = 2 * self.n_lev, self.offsets()
        u = lambda n, bound: (torch.rand(self.R, n, generator=generator, device=self.device) * 2 - 1) * bound
        # Net: xavier_uniform_ on fc1 (fan_in 2 k1, fan_out C k1, :173); Net_BN: kaiming_uniform_ (a = 0: bound sqrt(6 / fan_in), :195)
        self.theta[:, o[0]:o[1]] = u(o[1] - o[0], (6.0 / (2 * self.k1)) ** 0.5 if self.batch_norm else (6.0 / (2 * self.k1 + C_ * self.k1)) ** 0.5)
        self.theta[:, o[1]:o[2]] = u(C_, (2 * self.k1) ** -0.5)
        self.theta[:, o[2]:o[3]] = u(o[3] - o[2], (6.0 / (2 * C_ * self.k2)) ** 0.5)
        self.theta[:, o[3]:o[4]] = u(C_, (C_ * self.k2) ** -0.5)
        if self.batch_norm:
            self.theta[:, o[4]:o[5]] = 1                        # BatchNorm weight
            self.theta[:, o[5]:o[6]] = 0                        # BatchNorm bias
            self.bn[:, :C_] = 0
            self.bn[:, C_:] = 1
        oh = o[-2]
        self.theta[:, oh:] = 0
        self.theta[:, oh + self.M // 2] = 1
        for t in (self.m, self.v, self.vmax):
            t.zero_()
        self.step.zero_()

    def train(self, rx, B, steps, lr, want_q=False, debug_grads=False, no_update=False):
        """rx[R,2,S] -> dict(loss[R,steps], q[R,2n,steps*B]?, g[R,NP]?)."""
        R, S = rx.shape[0], rx.shape[-1]
        if R != self.R or rx.dim() != 3 or rx.shape[1] != 2:
            raise ValueError(f"rx must be [R={self.R}, 2, S], got {tuple(rx.shape)}")
        rx = rx.contiguous()
        dev = self.device
        lr_t = _f32(lr, dev).expand(R).contiguous()
        out = {"loss": torch.empty(R, steps, dtype=torch.float32, device=dev),
               "q": torch.empty(R, 2 * self.n_lev, steps * B, dtype=torch.float32, device=dev) if want_q else None,
               "g": torch.empty(R, self.NP, dtype=torch.float32, device=dev) if debug_grads else None}
        a = nat.NNArgs(R=R, steps=steps, B=B, sps=self.sps, M=self.M, n_lev=self.n_lev, k1=self.k1, k2=self.k2, S=S, rx=nat.ptr(rx),
                       theta=nat.ptr(self.theta), adam_m=nat.ptr(self.m), adam_v=nat.ptr(self.v), adam_x=nat.ptr(self.vmax),
                       step=nat.ptr(self.step, torch.int32), amp=nat.ptr(self.amp), lr=nat.ptr(lr_t), loss=nat.ptr(out["loss"]),
                       q_out=nat.ptr(out["q"]), dbg_g=nat.ptr(out["g"]), no_update=int(no_update), batch_norm=int(self.batch_norm),
                       bn_running=nat.ptr(self.bn))
        with torch.cuda.device(dev):
            nat.check(nat.lib().vaeq_nn_train(C.byref(a), nat.current_stream(dev)), "vaeq_nn_train")
        out["_keepalive"] = (lr_t, rx)
        return out

    def forward(self, x):
        """Validation pass (:293-295): x[R,2,N*sps] -> q[R,2n,N]."""
        R, N = x.shape[0], x.shape[-1] // self.sps
        x = x.contiguous()
        q = torch.empty(R, 2 * self.n_lev, N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().vaeq_nn_forward(R, N, self.sps, self.M, self.n_lev, self.k1, self.k2, nat.ptr(x), nat.ptr(self.theta),
                                                nat.ptr(self.bn), nat.ptr(q), nat.current_stream(self.device)), "vaeq_nn_forward")
        return q

    def validate(self, x, data, n_shift=21):
        """Fused validation pass (:287-301) -> (SER[R] f32, shift[R] i32): eval forward, find_shift and SER_q in one kernel
        (vaeq_nn_validate); x[R,2,N*sps] f32, data[R,2,N] f16."""
        R, N = x.shape[0], x.shape[-1] // self.sps
        if tuple(data.shape) != (R, 2, N):
            raise ValueError(f"data must be [R={R}, 2, N={N}], got {tuple(data.shape)}")
        x, data = x.contiguous(), data.contiguous()
        ser = torch.empty(R, dtype=torch.float32, device=self.device)
        shift = torch.empty(R, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().vaeq_nn_validate(R, N, self.sps, self.M, self.n_lev, self.k1, self.k2, int(n_shift), nat.ptr(x),
                                                 nat.ptr(self.theta), nat.ptr(self.bn), nat.ptr(self.amp), nat.ptr(data, torch.float16), nat.ptr(ser),
                                                 nat.ptr(shift, torch.int32), nat.current_stream(self.device)), "vaeq_nn_validate")
        return ser, shift

    def info(self, x, data, shift, P=None):
        """GMI, NGMI, achievable rate and pre-FEC BER of a validation frame (awgn_info, q-mode on the eval forward's posteriors): x[R,2,N*sps],
        data[R,2,N] f16, shift[R] = validate's; P[R,n] / [n] the per-axis pmf (default uniform: the VAE-NN script's model).  The posteriors are
        formed and consumed in chunks of runs of at most 1 GiB each."""
        R, N = x.shape[0], x.shape[-1] // self.sps
        if R != self.R or tuple(data.shape) != (R, 2, N):
            raise ValueError(f"x must be [R={self.R}, 2, N*sps] and data [R, 2, N={N}], got {tuple(x.shape)}, {tuple(data.shape)}")
        n = self.n_lev
        P = _pmf([1.0 / n] * n if P is None else P, R, n, self.device)
        x, data = x.contiguous(), _f16(data)
        shift = _i32(shift, R, self.device)
        chunk = max(1, (1 << 30) // (2 * n * N * 4))
        parts = []
        for s in range(0, R, chunk):
            e = min(R, s + chunk)
            q = torch.empty(e - s, 2 * n, N, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                nat.check(nat.lib().vaeq_nn_forward(e - s, N, self.sps, self.M, n, self.k1, self.k2, nat.ptr(x[s:e]), nat.ptr(self.theta[s:e]),
                                                    None if self.bn is None else nat.ptr(self.bn[s:e]), nat.ptr(q),
                                                    nat.current_stream(self.device)), "vaeq_nn_forward")
            parts.append(awgn_info(q=q, data=data[s:e], amp_levels=self.amp, P=P[s:e], shift=shift[s:e]))
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

    def llr(self, x, shift, hyp):
        """Per-bit LLRs of a validation frame (awgn_llr, q-mode on the eval forward's posteriors) [R,2b,N]: x[R,2,N*sps], shift[R] = validate's,
        hyp[R] = info's.  The posteriors are formed and consumed in chunks of runs of at most 1 GiB each, as in info."""
        R, N = x.shape[0], x.shape[-1] // self.sps
        if R != self.R or x.dim() != 3 or x.shape[1] != 2:
            raise ValueError(f"x must be [R={self.R}, 2, N*sps], got {tuple(x.shape)}")
        n = self.n_lev
        x = x.contiguous()
        shift, hyp = _i32(shift, R, self.device), _i32(hyp, R, self.device)
        chunk = max(1, (1 << 30) // (2 * n * N * 4))
        parts = []
        for s in range(0, R, chunk):
            e = min(R, s + chunk)
            q = torch.empty(e - s, 2 * n, N, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                nat.check(nat.lib().vaeq_nn_forward(e - s, N, self.sps, self.M, n, self.k1, self.k2, nat.ptr(x[s:e]), nat.ptr(self.theta[s:e]),
                                                    None if self.bn is None else nat.ptr(self.bn[s:e]), nat.ptr(q),
                                                    nat.current_stream(self.device)), "vaeq_nn_forward")
            parts.append(awgn_llr(q=q, amp_levels=self.amp, shift=shift[s:e], hyp=hyp[s:e]))
        return torch.cat(parts)


def dp_epilogue(q, y, data, amp_levels, nu_sc, var, batch_len=None):
    """Per-frame epilogue on the device (vaeq_dp_epilogue): q[R,2,2n,N], y[R,2,2,N], data[R,2,2,N] fp16 ->
    dict(SER[R,4], shift_q[R,2], r_q[R], shift_c[R,2], r_c[R]).  batch_len None = VAEflex (no per-minibatch cut)."""
    dev, R, N = q.device, q.shape[0], q.shape[-1]
    amp = _amp(amp_levels, dev)
    n = amp.numel()
    var, nu = _var_nu(var, nu_sc, R, dev)
    q, y = q.contiguous(), y.contiguous()
    data = _f16(data)
    ser, shift, rflag = _alignment_out(R, dev)
    ws = torch.empty(int(nat.lib().vaeq_dp_epilogue_ws_bytes(R, N)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_epilogue(R, N, n, int(batch_len or 0), nat.ptr(q), nat.ptr(y), nat.ptr(data, torch.float16),
                                             nat.ptr(amp), nat.ptr(var), nat.ptr(nu), nat.ptr(ser), nat.ptr(shift, torch.int32),
                                             nat.ptr(rflag, torch.int32), nat.ptr(ws, torch.uint8), nat.current_stream(dev)),
                  "vaeq_dp_epilogue")
    return _alignment_dict(ser, shift, rflag)


def dp_epilogue_compact(eq, dec, y, data, amp_levels, nu_sc, var, batch_len=None):
    """dp_epilogue fed by the training kernel's compact outputs of one frame (vaeq_dp_epilogue_compact): eq[R,2,N] f32,
    dec[R,2,2,N] int8, y[R,2,2,N], data[R,2,2,N] fp16 -> the same dict; bit-identical to dp_epilogue on that call's q."""
    dev, R, N = y.device, y.shape[0], y.shape[-1]
    amp = _amp(amp_levels, dev)
    var, nu = _var_nu(var, nu_sc, R, dev)
    eq, dec, y = eq.contiguous(), dec.contiguous(), y.contiguous()
    data = _f16(data)
    ser, shift, rflag = _alignment_out(R, dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_epilogue_compact(R, N, amp.numel(), int(batch_len or 0), nat.ptr(eq), nat.ptr(dec, torch.int8), nat.ptr(y),
                                                     nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(var), nat.ptr(nu), nat.ptr(ser),
                                                     nat.ptr(shift, torch.int32), nat.ptr(rflag, torch.int32), nat.current_stream(dev)),
                  "vaeq_dp_epilogue_compact")
    return _alignment_dict(ser, shift, rflag)


def dp_epilogue_info(q=None, y=None, data=None, amp_levels=None, P=None, nu_sc=None, var=None, shift=None, r=None, batch_len=None):
    """Information-rate figures of one frame on the device (vaeq_dp_epilogue_info), over exactly the symbols dp_epilogue's soft-demapper SER keeps:
    exactly one of q[R,2,2n,N] and y[R,2,2,N] (y: the posteriors are recomputed by the soft demapper from var / nu_sc, in the log domain),
    data[R,2,2,N] fp16, P[R,n] (or [n]) the per-axis pmf, shift[R,2] / r[R] = dp_epilogue's shift_q / r_q ->
    dict(AIR[R,2], GMI[R,2], NGMI[R,2], BER[R,2] f32 (NaN where nothing is kept); kept, sym_err, bit_err, hyp [R,2] int64).
    AIR and GMI in bit per 2-D symbol; NGMI = 1 - (2 H - GMI) / (2 log2 n)."""
    dev, R, N, n, amp, q, y, data, var_t, nu_t, shift, r = _dp_frame("dp_epilogue_info", q, y, data, amp_levels, nu_sc, var, shift, r)
    P = _pmf(P, R, n, dev)
    info = torch.empty(R, 2, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(R, 2, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_epilogue_info(R, N, n, int(batch_len or 0), nat.ptr(q), nat.ptr(y),
                                                  nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(P), nat.ptr(var_t), nat.ptr(nu_t),
                                                  nat.ptr(shift, torch.int32), nat.ptr(r, torch.int32), nat.ptr(info), nat.ptr(counts, torch.int32),
                                                  nat.current_stream(dev)), "vaeq_dp_epilogue_info")
    return _info_dict(info, counts, P)


def awgn_info(q=None, y=None, data=None, amp_levels=None, P=None, amp_mean=None, var=None, shift=None):
    """Information-rate figures of an AWGN validation frame on the device (vaeq_awgn_info), over exactly the symbols the validation's SER_q keeps
    (q[:, 11+sh : -11] against data[:, 11 : -11-sh], sh = shift[r]): exactly one of q[R,2n,N] (stored posteriors) and y[R,2,N] (the validation's
    un-normalised output; the VAE-LE demapper's posteriors are recomputed from amp_mean[R] / var[R] in the log domain), data[R,2,N] fp16,
    P[R,n] (or [n]) the per-axis pmf, shift[R] ->
    dict(AIR[R], GMI[R], NGMI[R], BER[R] f32 (NaN where nothing is kept); kept, sym_err, bit_err, hyp [R] int64).
    AIR and GMI in bit per 2-D symbol; NGMI = 1 - (2 H - GMI) / (2 log2 n)."""
    dev, R, N, n, amp, q, y, data, am_t, var_t, shift = _awgn_frame("awgn_info", q, y, data, amp_levels, amp_mean, var, shift)
    P = _pmf(P, R, n, dev)
    info = torch.empty(R, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(R, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_info(R, N, n, nat.ptr(q), nat.ptr(y),
                                           nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(P), nat.ptr(am_t), nat.ptr(var_t),
                                           nat.ptr(shift, torch.int32), nat.ptr(info), nat.ptr(counts, torch.int32), nat.current_stream(dev)),
                  "vaeq_awgn_info")
    return _info_dict(info, counts, P)


def dp_epilogue_llr(q=None, y=None, amp_levels=None, nu_sc=None, var=None, shift=None, r=None, hyp=None, batch_len=None):
    """Per-bit a-posteriori LLRs of one frame on the device (vaeq_dp_epilogue_llr), the input of a bit-wise decoder: exactly one of q[R,2,2n,N] and
    y[R,2,2,N] (y: the soft demapper's posteriors are recomputed from var / nu_sc, in the log domain), shift[R,2] / r[R] = dp_epilogue's shift_q /
    r_q, hyp[R,2] = dp_epilogue_info's hyp on the same alignment -> llr[R,2,2b,N] f32 in nats, positive = bit 0, b = log2 n: plane a b + k of
    polarisation p at TX index n is bit k (b-1 = the top bit of the Gray label i ^ (i >> 1)) of TX axis a (0 = I, 1 = Q), aligned with
    label_bits(data, n); the symbols dp_epilogue_info does not keep are erasures, +0.0."""
    dev, R, N, n, amp, q, y, _, var_t, nu_t, shift, r = _dp_frame("dp_epilogue_llr", q, y, None, amp_levels, nu_sc, var, shift, r)
    hyp = _i32(hyp, (R, 2), dev)
    llr = torch.empty(R, 2, 2 * (n.bit_length() - 1), N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_epilogue_llr(R, N, n, int(batch_len or 0), nat.ptr(q), nat.ptr(y),
                                                 nat.ptr(amp), nat.ptr(var_t), nat.ptr(nu_t), nat.ptr(shift, torch.int32), nat.ptr(r, torch.int32),
                                                 nat.ptr(hyp, torch.int32), nat.ptr(llr), nat.current_stream(dev)), "vaeq_dp_epilogue_llr")
    return llr


def awgn_llr(q=None, y=None, amp_levels=None, amp_mean=None, var=None, shift=None, hyp=None):
    """Per-bit a-posteriori LLRs of an AWGN validation frame on the device (vaeq_awgn_llr): exactly one of q[R,2n,N] (stored posteriors) and
    y[R,2,N] (the validation's un-normalised output; the VAE-LE demapper's posteriors are recomputed from amp_mean[R] / var[R] as awgn_info
    does), shift[R], hyp[R] = awgn_info's hyp on the same shift -> llr[R,2b,N] f32 in nats, positive = bit 0: plane a b + k at TX index n is bit
    k of TX axis a, aligned with label_bits(data, n); everything outside TX indices [11, N - 11 - shift) is an erasure, +0.0."""
    dev, R, N, n, amp, q, y, _, am_t, var_t, shift = _awgn_frame("awgn_llr", q, y, None, amp_levels, amp_mean, var, shift)
    hyp = _i32(hyp, R, dev)
    llr = torch.empty(R, 2 * (n.bit_length() - 1), N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_llr(R, N, n, nat.ptr(q), nat.ptr(y), nat.ptr(amp),
                                          nat.ptr(am_t), nat.ptr(var_t), nat.ptr(shift, torch.int32), nat.ptr(hyp, torch.int32), nat.ptr(llr),
                                          nat.current_stream(dev)), "vaeq_awgn_llr")
    return llr


def cma_epilogue(y, data, amp_levels, nu_sc, var):
    """The constant-modulus baselines' two-stage epilogue of one frame in one launch (vaeq_cma_epilogue): y[R,2,2,N] = phase-corrected output cut
    to [10:-10], data[R,2,2,N] fp16 cut likewise -> dict(SER[R,4] (constellation rows, then soft-demapper rows), shift_c, r_c, shift_q, r_q)."""
    dev, R, N = y.device, y.shape[0], y.shape[-1]
    amp = _amp(amp_levels, dev)
    var, nu = _var_nu(var, nu_sc, R, dev)
    y = y.contiguous()
    data = _f16(data)
    ser, shift, rflag = _alignment_out(R, dev)
    L = nat.lib()
    ws = torch.empty(int(L.vaeq_dp_epilogue_ws_bytes(R, N)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.vaeq_cma_epilogue(R, N, amp.numel(), nat.ptr(y), nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(var), nat.ptr(nu), nat.ptr(ser),
                                      nat.ptr(shift, torch.int32), nat.ptr(rflag, torch.int32), nat.ptr(ws, torch.uint8), nat.current_stream(dev)),
                  "vaeq_cma_epilogue")
    return _alignment_dict(ser, shift, rflag)


def cma_epilogue_info(y, data, amp_levels, P, nu_sc, var, shift_c, r_c, shift_q, r_q):
    """Information-rate figures of one frame of the constant-modulus baselines on the device (vaeq_cma_epilogue_info), over exactly the symbols
    cma_epilogue's soft-demapper SER keeps: y[R,2,2,N], data[R,2,2,N] fp16, nu_sc, var as cma_epilogue got them, P[R,n] (or [n]) the per-axis pmf,
    shift_c[R,2] / r_c[R] / shift_q[R,2] / r_q[R] = that call's alignment.  The posteriors are the soft demapper's on the stage-c aligned output
    whose kept window carries the mean-radius normalisation, recomputed in the log domain (neither that sequence nor q exists in memory) ->
    dict(AIR[R,2], GMI[R,2], NGMI[R,2], BER[R,2] f32 (NaN for a run without a normalisation); kept, sym_err, bit_err, hyp [R,2] int64).
    AIR and GMI in bit per 2-D symbol; NGMI = 1 - (2 H - GMI) / (2 log2 n)."""
    dev, R, N, n, amp, y, data, var_t, nu_t, sc, rc, sq, rq = _cma_frame(y, data, amp_levels, nu_sc, var, shift_c, r_c, shift_q, r_q)
    P = _pmf(P, R, n, dev)
    info = torch.empty(R, 2, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(R, 2, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_cma_epilogue_info(R, N, n, nat.ptr(y), nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(P), nat.ptr(var_t),
                                                   nat.ptr(nu_t), nat.ptr(sc, torch.int32), nat.ptr(rc, torch.int32), nat.ptr(sq, torch.int32),
                                                   nat.ptr(rq, torch.int32), nat.ptr(info), nat.ptr(counts, torch.int32), nat.current_stream(dev)),
                  "vaeq_cma_epilogue_info")
    return _info_dict(info, counts, P)


def cma_epilogue_llr(y, data, amp_levels, nu_sc, var, shift_c, r_c, shift_q, r_q, hyp):
    """Per-bit a-posteriori LLRs of one frame of the constant-modulus baselines on the device (vaeq_cma_epilogue_llr), the input of a bit-wise
    decoder: y[R,2,2,N], data[R,2,2,N] fp16 (needed for the mean-radius factor only), nu_sc, var and the four alignment outputs as
    cma_epilogue_info got them, hyp[R,2] = that call's hyp -> llr[R,2,2b,N] f32 in nats, positive = bit 0, b = log2 n: plane a b + k of output
    polarisation p at TX index n is bit k of TX axis a, aligned with label_bits(data, n).  The posteriors are cma_epilogue_info's; the symbols
    it does not keep are erasures, +0.0, and a run without a normalisation is all zeros."""
    dev, R, N, n, amp, y, data, var_t, nu_t, sc, rc, sq, rq = _cma_frame(y, data, amp_levels, nu_sc, var, shift_c, r_c, shift_q, r_q)
    hyp = _i32(hyp, (R, 2), dev)
    llr = torch.empty(R, 2, 2 * (n.bit_length() - 1), N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_cma_epilogue_llr(R, N, n, nat.ptr(y), nat.ptr(data, torch.float16), nat.ptr(amp), nat.ptr(var_t), nat.ptr(nu_t),
                                                  nat.ptr(sc, torch.int32), nat.ptr(rc, torch.int32), nat.ptr(sq, torch.int32),
                                                  nat.ptr(rq, torch.int32), nat.ptr(hyp, torch.int32), nat.ptr(llr), nat.current_stream(dev)),
                  "vaeq_cma_epilogue_llr")
    return llr


def awgn_loss(q, x, h, amp_levels, P=None):
    """ELBO of the single-polarisation variants for a given q (vaeq_awgn_loss): q[R,2n,B] (or [2n,B]), x[R,2,B*sps], h[R,2,M];
    P[R,n] / [n] -> the VAE-LE form (KL to the prior), P None -> the VAE-NN form (entropy).  Returns loss[R] (or a 0-dim tensor)."""
    single = q.dim() == 2
    if single:
        q, x, h = q.unsqueeze(0), x.unsqueeze(0), h.unsqueeze(0)
    dev, R, B = q.device, q.shape[0], q.shape[-1]
    amp = _amp(amp_levels, dev).contiguous()
    n = amp.numel()
    q, x, h = q.contiguous().float(), x.contiguous().float(), h.contiguous().float()
    Pt = None if P is None else _f32(P, dev).expand(R, n).contiguous()
    loss = torch.empty(R, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_loss(R, B, x.shape[-1] // B, h.shape[-1], n, nat.ptr(q), nat.ptr(x), nat.ptr(h), nat.ptr(amp),
                                           nat.ptr(Pt), nat.ptr(loss), nat.current_stream(dev)), "vaeq_awgn_loss")
    return loss[0] if single else loss


def cma(rx, h, lr, sps=2, mode="CMA", batch_len=100, symb_step=10, R_mod=1.0, want_e=True):
    """CMA / CMAbatch / CMAflex (shared_funcs.py:341-488, vaeq_cma) for R runs: rx[R,2,2,N], h[R,2,2,2,M] (updated IN PLACE),
    lr scalar or [R] -> (out[R,2,2,N//sps], e[R,N//sps,2] or None)."""
    dev, R, N = rx.device, rx.shape[0], rx.shape[-1]
    if tuple(rx.shape[1:3]) != (2, 2) or tuple(h.shape[:4]) != (R, 2, 2, 2) or not h.is_contiguous():
        raise ValueError(f"rx must be [R,2,2,N] and h a contiguous [R,2,2,2,M], got {tuple(rx.shape)}, {tuple(h.shape)}")
    m = {"CMA": 0, "CMAbatch": 1, "CMAflex": 1}[mode]
    step = batch_len if mode == "CMAbatch" else symb_step
    rx = rx.contiguous()
    lr_t = _f32(lr, dev).expand(R).contiguous()
    K = N // sps
    out = torch.empty(R, 2, 2, K, dtype=torch.float32, device=dev)
    e = torch.empty(R, K, 2, dtype=torch.float32, device=dev) if want_e else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_cma(R, N, sps, h.shape[-1], m, int(batch_len), int(step), nat.ptr(rx), float(R_mod), nat.ptr(h),
                                     nat.ptr(lr_t), nat.ptr(out), nat.ptr(e), nat.current_stream(dev)), "vaeq_cma")
    return out, e


def cpe(y, M_ma=501):
    """Viterbi-Viterbi carrier phase estimation (shared_funcs.py:139-186, vaeq_cpe): y[R,2,2,N] (or [2,2,N]) -> corrected y."""
    squeeze = y.dim() == 3
    if squeeze:
        y = y.unsqueeze(0)
    y = y.contiguous().float()
    out = torch.empty_like(y)
    with torch.cuda.device(y.device):
        nat.check(nat.lib().vaeq_cpe(y.shape[0], y.shape[-1], int(M_ma), nat.ptr(y), nat.ptr(out), nat.current_stream(y.device)), "vaeq_cpe")
    return out[0] if squeeze else out


def awgn_cma(rx, h, lr, sps=2, update=True, R_mod=1.0, want_out=False, want_e=False):
    """The AWGN scripts' constant-modulus training pass (AWGN_channel/func_CMA_MQAM_shaping.py:142-168, vaeq_awgn_cma) for R runs:
    rx[R,2,N], h[R,2,M] (updated IN PLACE when ``update``; untouched otherwise = CMA(..., eval=False)), lr scalar or [R]
    -> (loss[R] = mean|e|, out[R,2,N//sps] or None, e[R,N//sps] or None)."""
    dev, R, N = rx.device, rx.shape[0], rx.shape[-1]
    if rx.dim() != 3 or rx.shape[1] != 2 or h.dim() != 3 or tuple(h.shape[:2]) != (R, 2) or not h.is_contiguous():
        raise ValueError(f"rx must be [R,2,N] and h a contiguous [R,2,M], got {tuple(rx.shape)}, {tuple(h.shape)}")
    rx = rx.contiguous()
    lr_t = _f32(lr, dev).expand(R).contiguous()
    K = N // sps
    loss = torch.empty(R, dtype=torch.float32, device=dev)
    out = torch.empty(R, 2, K, dtype=torch.float32, device=dev) if want_out else None
    e = torch.empty(R, K, dtype=torch.float32, device=dev) if want_e else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_cma(R, N, int(sps), h.shape[-1], int(bool(update)), nat.ptr(rx), float(R_mod), nat.ptr(h), nat.ptr(lr_t),
                                          nat.ptr(loss), nat.ptr(out), nat.ptr(e), nat.current_stream(dev)), "vaeq_awgn_cma")
    return loss, out, e


def awgn_cma_validate(rx, h, data, amp_levels, sps=2, n_shift=21, want_cpe=False):
    """One evaluated epoch of the AWGN constant-modulus script in one launch (func_CMA_MQAM_shaping.py:225-232, vaeq_awgn_cma_validate):
    CMA(..., eval=False) with the taps h[R,2,M], CPE, find_shift_symb and SER_CMA on rx[R,2,N] against data[R,2,N//sps] (fp16)
    -> (SER[R] f32, shift[R] i32, CPE output [R,2,N//sps] or None)."""
    dev, R, N = rx.device, rx.shape[0], rx.shape[-1]
    K = N // sps
    if tuple(data.shape) != (R, 2, K) or tuple(h.shape[:2]) != (R, 2):
        raise ValueError(f"data must be [R={R}, 2, {K}] and h [R, 2, M], got {tuple(data.shape)}, {tuple(h.shape)}")
    rx, h = rx.contiguous(), h.contiguous()
    data = _f16(data)
    amp = _amp(amp_levels, dev)
    L = nat.lib()
    wsb = int(L.vaeq_awgn_cma_validate_ws_bytes(R, N, int(sps)))
    nat.check(min(wsb, 0), "vaeq_awgn_cma_validate_ws_bytes")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev) if wsb > 0 else None
    ser = torch.empty(R, dtype=torch.float32, device=dev)
    shift = torch.empty(R, dtype=torch.int32, device=dev)
    cpe_out = torch.empty(R, 2, K, dtype=torch.float32, device=dev) if want_cpe else None
    with torch.cuda.device(dev):
        nat.check(L.vaeq_awgn_cma_validate(R, N, int(sps), h.shape[-1], amp.numel(), int(n_shift), nat.ptr(rx), nat.ptr(h), nat.ptr(amp),
                                           nat.ptr(data, torch.float16), nat.ptr(ws), nat.ptr(ser), nat.ptr(shift, torch.int32), nat.ptr(cpe_out),
                                           nat.current_stream(dev)), "vaeq_awgn_cma_validate")
    return ser, shift, cpe_out


def _taps2(taps, R, dev):
    """Complex taps [K] or [R,K] (complex tensor / array) or [R,2,K] float -> contiguous float32 [R,2,K] (re, im) on ``dev``."""
    t = torch.as_tensor(taps)
    if t.is_complex():
        t = t.to(dev).reshape(-1, t.shape[-1]).expand(R, -1)
        t = torch.stack([t.real, t.imag], 1)
    elif t.dim() == 2 and t.shape[0] == 2:
        t = t.to(dev).unsqueeze(0).expand(R, -1, -1)
    return t.to(dev, torch.float32).contiguous()


def awgn_lmmse_eval(rx, taps, data, amp_levels, n_shift=21, n_cut=20, want_out=False):
    """The LMMSE evaluation of AWGN_channel/DFE_MQAM_shaping.py (:274-281, vaeq_awgn_lmmse_eval) for R frames at sps = 1 in one launch:
    rx[R,2,N], taps (complex [K] / [R,K], or [R,2,K] re/im; K even), data[R,2,N] (fp16) -> (SER[R] f32, shift[R] i32, decisions[R,N] int8
    (iI * n + iQ of out[1:]), LMMSE output [R,N+1] complex64 or None)."""
    dev, R, N = rx.device, rx.shape[0], rx.shape[-1]
    if rx.dim() != 3 or rx.shape[1] != 2 or tuple(data.shape) != (R, 2, N):
        raise ValueError(f"rx and data must be [R,2,N], got {tuple(rx.shape)}, {tuple(data.shape)}")
    rx = rx.contiguous()
    h = _taps2(taps, R, dev)
    K = h.shape[-1]
    data = _f16(data)
    amp = _amp(amp_levels, dev)
    L = nat.lib()
    wsb = int(L.vaeq_awgn_lmmse_eval_ws_bytes(R, N, K))
    nat.check(min(wsb, 0), "vaeq_awgn_lmmse_eval_ws_bytes")
    No = N + 2 * (K // 2) - K + 1
    out = torch.empty(R, No, 2, dtype=torch.float32, device=dev) if want_out else None
    ws = None if want_out else torch.empty(max(wsb // 4, 1), dtype=torch.float32, device=dev)
    ser = torch.empty(R, dtype=torch.float32, device=dev)
    shift = torch.empty(R, dtype=torch.int32, device=dev)
    dec = torch.empty(R, N, dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.vaeq_awgn_lmmse_eval(R, N, 1, amp.numel(), K, int(n_shift), int(n_cut), nat.ptr(rx), nat.ptr(h), nat.ptr(amp),
                                         nat.ptr(data, torch.float16), nat.ptr(ws), nat.ptr(ser), nat.ptr(shift, torch.int32),
                                         nat.ptr(dec, torch.int8), nat.ptr(out), nat.current_stream(dev)), "vaeq_awgn_lmmse_eval")
    return ser, shift, dec, (torch.view_as_complex(out) if want_out else None)


def dfe_chunks(R, N, K2):
    """The speculate-and-repair split the host picks: C chunks of about 128 symbols each, at most 64 Ki lanes in all (R * C), and W = 32
    symbols of warm-up."""
    C = max(1, min(max(1, 65536 // max(R, 1)), (N - K2) // 128, 8192))
    return C, 32


def awgn_dfe(rx, ff_taps, fb_taps, init_dec, amp_levels, data=None, n_shift=24, n_cut=20, C=None, W=None, want_ff=False):
    """The DFE of AWGN_channel/DFE_MQAM_shaping.py (:283-293, vaeq_awgn_dfe) for R frames at sps = 1: feed-forward FIR, the decision
    recursion seeded by the LMMSE decisions init_dec[R,N] (int8), and -- when ``data`` [R,2,N] is given -- find_shift_symb and SER_func on
    the hard decisions.  C / W: chunks and warm-up of the speculate-and-repair recursion (default: dfe_chunks; the decisions do not depend
    on them).  -> dict(dec[R,N] int8, ser[R] / shift[R] (None without data), repairs[R] i32, ff [R,N] complex64 or None, C, W)."""
    dev, R, N = rx.device, rx.shape[0], rx.shape[-1]
    if rx.dim() != 3 or rx.shape[1] != 2 or tuple(init_dec.shape) != (R, N):
        raise ValueError(f"rx must be [R,2,N] and init_dec [R,N], got {tuple(rx.shape)}, {tuple(init_dec.shape)}")
    rx = rx.contiguous()
    ff_t, fb_t = _taps2(ff_taps, R, dev), _taps2(fb_taps, R, dev)
    K1, K2 = ff_t.shape[-1], fb_t.shape[-1]
    c0, w0 = dfe_chunks(R, N, K2)
    C = c0 if C is None else int(C)
    W = w0 if W is None else int(W)
    init_dec = init_dec.to(dev, torch.int8).contiguous()
    amp = _amp(amp_levels, dev)
    L = nat.lib()
    wsb = int(L.vaeq_awgn_dfe_ws_bytes(R, N, C))
    nat.check(min(wsb, 0), "vaeq_awgn_dfe_ws_bytes")
    ws = torch.empty(max(wsb, 1), dtype=torch.int8, device=dev)
    dec = torch.empty(R, N, dtype=torch.int8, device=dev)
    repairs = torch.empty(R, dtype=torch.int32, device=dev)
    ff = torch.empty(R, N, 2, dtype=torch.float32, device=dev) if want_ff else None
    ser = shift = None
    if data is not None:
        if tuple(data.shape) != (R, 2, N):
            raise ValueError(f"data must be [R={R}, 2, {N}], got {tuple(data.shape)}")
        data = _f16(data)
        ser = torch.empty(R, dtype=torch.float32, device=dev)
        shift = torch.empty(R, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(L.vaeq_awgn_dfe(R, N, 1, amp.numel(), K1, K2, C, W, int(n_shift), int(n_cut), nat.ptr(rx), nat.ptr(ff_t), nat.ptr(fb_t),
                                  nat.ptr(amp), nat.ptr(init_dec, torch.int8), nat.ptr(data, torch.float16), nat.ptr(ws, torch.int8),
                                  nat.ptr(dec, torch.int8), nat.ptr(ser), nat.ptr(shift, torch.int32), nat.ptr(repairs, torch.int32),
                                  nat.ptr(ff), nat.current_stream(dev)), "vaeq_awgn_dfe")
    return dict(dec=dec, ser=ser, shift=shift, repairs=repairs, ff=torch.view_as_complex(ff) if want_ff else None, C=C, W=W)


def awgn_track_info(z, data, amp_levels, P, var, shift, edge=11):
    """Information-rate figures of an AWGN baseline's soft sequence on the device (vaeq_awgn_track_info), over exactly the symbols its validator's
    SER keeps (z[:, e+sh : -e] against data[:, e : -e-sh], sh = shift[r], e = edge: 11 for awgn_cma_validate, N_cut + 11 for the LMMSE and the DFE).
    z: float [R,2,Nz] (planar: the CPE output of awgn_cma_validate) or complex [R,Nz] (the LMMSE output, Nz = Nd + 1, or awgn_dfe_soft's); the
    layout follows from the dtype.  data[R,2,Nd] fp16, P[R,n] (or [n]) the per-axis pmf, var[R] (or a scalar) the demapper's variance
    (10^(-SNR/10) in the host layers), shift[R] the validator's ->
    dict(AIR[R], GMI[R], NGMI[R], BER[R] f32 (NaN where nothing is kept or z is zero); kept, sym_err, bit_err, hyp [R] int64).
    AIR and GMI in bit per 2-D symbol; NGMI = 1 - (2 H - GMI) / (2 log2 n)."""
    dev, R, Nz, Nd, n, interleaved, amp, z, data, var_t, shift = _track(z, data, amp_levels, var, shift)
    P = _pmf(P, R, n, dev)
    info = torch.empty(R, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(R, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_track_info(R, Nz, Nd, n, int(edge), int(interleaved), nat.ptr(z), nat.ptr(data, torch.float16), nat.ptr(amp),
                                                 nat.ptr(P), nat.ptr(var_t), nat.ptr(shift, torch.int32), nat.ptr(info),
                                                 nat.ptr(counts, torch.int32), nat.current_stream(dev)), "vaeq_awgn_track_info")
    return _info_dict(info, counts, P)


def awgn_track_llr(z, data, amp_levels, var, shift, hyp, edge=11):
    """Per-bit a-posteriori LLRs of an AWGN baseline's soft sequence on the device (vaeq_awgn_track_llr), the input of a bit-wise decoder: z, data,
    var, shift and edge as awgn_track_info got them (z float [R,2,Nz] planar or complex [R,Nz]; the layout follows from the dtype; data is needed
    for the normalisation only), hyp[R] = that call's hyp -> llr[R,2b,Nd] f32 in nats, positive = bit 0: plane a b + k at TX index edge + j,
    j < Nd - 2 edge - shift, is bit k of TX axis a of sample edge + shift + j, aligned with label_bits(data, n); everything else is an erasure,
    +0.0, and a run whose window is empty or whose slice is zero is all zeros."""
    dev, R, Nz, Nd, n, interleaved, amp, z, data, var_t, shift = _track(z, data, amp_levels, var, shift)
    hyp = _i32(hyp, R, dev)
    llr = torch.empty(R, 2 * (n.bit_length() - 1), Nd, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_track_llr(R, Nz, Nd, n, int(edge), int(interleaved), nat.ptr(z), nat.ptr(data, torch.float16), nat.ptr(amp),
                                                nat.ptr(var_t), nat.ptr(shift, torch.int32), nat.ptr(hyp, torch.int32), nat.ptr(llr),
                                                nat.current_stream(dev)), "vaeq_awgn_track_llr")
    return llr


def awgn_dfe_soft(ff, fb_taps, dec, amp_levels):
    """The DFE's soft sequence (vaeq_awgn_dfe_soft): the slicer input of the reference's dfe() (DFE_MQAM_shaping.py:215-221), which keeps only the
    hard decisions, rebuilt from awgn_dfe's ff[R,N] complex64 (want_ff) and dec[R,N] int8 and the feedback taps (as awgn_dfe takes them):
    z[p] = ff[p] + sum_j fb[j] c(dec[p-1-j]) for p >= K2, c(dec[p]) in front -> z[R,N] complex64."""
    dev, R, N = ff.device, ff.shape[0], ff.shape[-1]
    if not ff.is_complex() or ff.dim() != 2 or tuple(dec.shape) != (R, N):
        raise ValueError(f"ff must be complex [R,N] and dec [R,N], got {tuple(ff.shape)} {ff.dtype}, {tuple(dec.shape)}")
    ff = torch.view_as_real(ff.to(torch.complex64).contiguous())
    fb = _taps2(fb_taps, R, dev)
    dec = dec.to(dev, torch.int8).contiguous()
    amp = _amp(amp_levels, dev)
    z = torch.empty(R, N, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_awgn_dfe_soft(R, N, amp.numel(), fb.shape[-1], nat.ptr(ff), nat.ptr(fb), nat.ptr(dec, torch.int8), nat.ptr(amp),
                                               nat.ptr(z), nat.current_stream(dev)), "vaeq_awgn_dfe_soft")
    return torch.view_as_complex(z)

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


def label_bits(data, n_lev):
    """The transmitted label bits in the plane order of dp_epilogue_llr / awgn_llr: data[..., 2, N] (the TX reference, axis 0 = I, 1 = Q) ->
    int8[..., 2b, N], plane a b + k = bit k of the Gray label t ^ (t >> 1) of the level t = clamp(rint((n-1)/2 data + (n-1)/2), 0, n-1) of
    axis a.  Plain torch ops, on the device data lives on."""
    n = int(n_lev)
    b = n.bit_length() - 1
    scale = 0.5 * (n - 1)
    t = torch.clamp(torch.round(scale * data.to(torch.float16).to(torch.float32) + scale), 0, n - 1).to(torch.int32)
    g = t ^ (t >> 1)
    k = torch.arange(b, dtype=torch.int32, device=data.device)
    bits = (g.unsqueeze(-2) >> k.unsqueeze(-1)) & 1                              # [..., 2, b, N]
    return bits.reshape(*data.shape[:-2], 2 * b, data.shape[-1]).to(torch.int8)


class LdpcCode:
    """A quasi-cyclic LDPC code for ldpc_decode: shifts[mb, nb] of circulant shifts, -1 = a zero block, 0 <= s < Z = the Z x Z block that connects
    check l Z + i to variable c Z + (i + s) mod Z.  n = nb Z bits, m = mb Z checks.  The decoder's envelope (1 <= mb <= 8, 2 <= nb <= 64,
    2 <= Z <= 512, 2 .. 32 non-zero blocks in every block row, 64 KiB of state) is vaeq_ldpc_decode's to refuse."""

    def __init__(self, shifts, Z):
        import numpy as np
        self.shifts = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32))
        if self.shifts.ndim != 2:
            raise ValueError(f"expected shifts[mb, nb], got shape {self.shifts.shape}")
        self.Z = int(Z)
        self.mb, self.nb = (int(d) for d in self.shifts.shape)
        self.n, self.m = self.nb * self.Z, self.mb * self.Z

    def H(self):
        """The dense parity-check matrix, uint8 [m, n] (for tests: n m bytes)."""
        import numpy as np
        H = np.zeros((self.m, self.n), np.uint8)
        i = np.arange(self.Z)
        for l in range(self.mb):
            for c in range(self.nb):
                s = int(self.shifts[l, c])
                if s >= 0:
                    H[l * self.Z + i, c * self.Z + (i + s) % self.Z] = 1
        return H


def array_code(mb, nb, Z):
    """The array code: shift (l c) mod Z in block (l, c).  For a prime Z >= nb it has no 4-cycles."""
    import numpy as np
    return LdpcCode(np.outer(np.arange(mb), np.arange(nb)) % Z, Z)


QUANT_KEYS = ("bits", "scale", "app_bits", "num", "beta")


def resolve_quant(quant):
    """ldpc_decode's quant= dict(bits, scale=None, app_bits=None, num=6, beta=0) with its defaults filled in: app_bits = bits + 2 and
    scale = 2 ** (bits - 5), a clip near +-16 nats at every width and one nat per step at 5 bits.  ValueError for an unknown key, a missing or
    non-integer bits; the ranges are vaeq_ldpc_decode_q's to refuse."""
    import numbers
    if not isinstance(quant, dict) or set(quant) - set(QUANT_KEYS) or "bits" not in quant:
        raise ValueError(f"quant takes a dict of {', '.join(QUANT_KEYS)} with bits in it; got {sorted(quant) if isinstance(quant, dict) else quant!r}")
    bits = quant["bits"]
    if not isinstance(bits, numbers.Integral) or isinstance(bits, bool):
        raise ValueError(f"quant['bits'] is an integer number of bits, got {bits!r}")
    bits = int(bits)
    scale, app = quant.get("scale"), quant.get("app_bits")
    return dict(bits=bits, scale=2.0 ** (bits - 5) if scale is None else float(scale), app_bits=bits + 2 if app is None else int(app),
                num=int(quant.get("num", 6)), beta=int(quant.get("beta", 0)))


def _ldpc_fit(N, w, n, t0, depth):
    """The most codewords of n bits that fit behind t0 into N symbols of w bits: bit-packed (depth None) or in whole symbols."""
    if depth is None:
        return (N - int(t0)) * w // n if n > 0 else 0
    return (N - int(t0)) // -(-n // w) if n > 0 and w > 0 else 0


def _ldpc_rule(alpha, quant):
    """alpha= and quant= of ldpc_decode and ldpc_sc_decode -> (alpha with its default, the resolved quant dict or None)."""
    if quant is not None:
        if alpha is not None:
            raise ValueError("alpha belongs to the float decoder; the fixed-point one is normalised by quant['num'] and quant['beta']")
        quant = resolve_quant(quant)
    return (0.75 if alpha is None else alpha), quant


def _ldpc_frame(llr, bits):
    """llr and bits of one shape [R,2,2b,N] or [R,w,N] -> (dev, R, N, w, llr[R,w,N], bits[R,w,N]), both contiguous."""
    if llr.shape != bits.shape or llr.dim() not in (3, 4):
        raise ValueError(f"expected llr and bits of one shape [R,2,2b,N] or [R,w,N], got {tuple(llr.shape)}, {tuple(bits.shape)}")
    R, N = llr.shape[0], llr.shape[-1]
    llr = llr.reshape(R, -1, N).contiguous()
    return llr.device, R, N, llr.shape[1], llr, bits.reshape(R, -1, N).contiguous()


def _ldpc_count(given, what, N, w, n, t0, depth):
    """The codewords (chains) of a run: as given, or the most that fit behind t0, which must be one at least."""
    if given is not None:
        return int(given)
    C_ = _ldpc_fit(N, w, n, t0, depth)
    if C_ < 1:
        raise ValueError(f"no {what} of {n} bits fits into {N - int(t0)} symbols of {w} bits")
    return C_


def _ldpc_figures(out, C_, n):
    """The dict both decoders return, from out[R, C, >= 5] int32 -> (out as int64, dict)."""
    o = out.long()
    tot = torch.full((out.shape[0],), float(max(C_ * n, 1)), dtype=torch.float64, device=out.device)   # a tensor divisor: a true division, not a product with 1 / tot
    return o, dict(iters=o[..., 0], ok=o[..., 1], bit_err=o[..., 2], pre_err=o[..., 3], erased=o[..., 4],
                   BER_post=(o[..., 2].sum(1).double() / tot).float(), BER_pre=(o[..., 3].sum(1).double() / tot).float(),
                   FER=((o[..., 2] > 0).sum(1).double() / torch.full_like(tot, float(max(C_, 1)))).float())


def ldpc_decode(llr, bits, code, t0=0, codewords=None, max_iter=20, alpha=None, want_post=False, depth=None, quant=None, outer=None):
    """Post-FEC figures of per-bit LLRs on the device (vaeq_ldpc_decode): layered normalized min-sum towards the syndrome of the TX bits (no
    encoder).  llr f32 and bits int8 of one shape, [R,2,2b,N] (dp_epilogue_llr / cma_epilogue_llr with label_bits) or [R,w,N] (awgn_llr,
    awgn_track_llr); bit j of codeword c of a run is global bit c n + j, at symbol t0 + (c n + j) // w in plane (c n + j) % w.  codewords: per
    run, default the most that fit behind t0.  -> dict(iters, ok, bit_err, pre_err, erased [R,C] int64; BER_post[R], BER_pre[R], FER[R] f32
    (FER: the share of codewords with bit_err > 0); post[R,C,n] f32, the final LLRs in codeword order, if want_post).  alpha defaults to 0.75.
    depth: an int puts a symbol interleaver over groups of `depth` codewords in front of the decoder (vaeq_ldpc_decode_il): codewords of
    S = ceil(n / w) whole symbols, symbol u of the codeword with local index d of a group of D at symbol base + u D + d; codewords then defaults
    to (N - t0) // S.  None: the contiguous bit-packed codewords above.
    quant: dict(bits, scale=None, app_bits=None, num=6, beta=0) decodes in fixed point instead (vaeq_ldpc_decode_q): LLRs quantised to `bits`
    bits as rint(llr * scale) (default scale 2 ** (bits - 5)), `bits`-bit check messages, a-posteriori values saturating at app_bits (default
    bits + 2) bits, messages normalised as max(((num m + 4) >> 3) - beta, 0).  Unlike the float decoder this one sees the scale of the LLRs: what
    a wrong noise variance costs after FEC.  alpha has no meaning there and is a ValueError if passed.  The same dict comes back, post int16,
    erased counting what the quantiser rounded to zero, and the resolved dict under "quant".
    outer: dict(code=BchCode, payload=None, spread=True, codewords=None) puts a hard-decision outer decoder behind this one: bch_outer on the
    final LLRs (kept on the device, returned only with want_post), its dict under "outer".  payload defaults to (nb - mb) Z, the first bits of
    every codeword."""
    if outer is not None:
        outer = resolve_outer(outer, code)
    alpha, quant = _ldpc_rule(alpha, quant)
    dev, R, N, w, llr, bits = _ldpc_frame(llr, bits)
    n = code.n
    C_ = _ldpc_count(codewords, "codeword", N, w, n, t0, depth)
    out = torch.empty(R, max(C_, 0), 5, dtype=torch.int32, device=dev)
    post = torch.empty(R, max(C_, 0), n, dtype=torch.float32 if quant is None else torch.int16, device=dev) if want_post or outer is not None else None
    with torch.cuda.device(dev):
        head = (code.mb, code.nb, code.Z, code.shifts.ctypes.data_as(C.c_void_p), nat.ptr(llr), nat.ptr(bits, torch.int8))
        tail = (int(max_iter), nat.ptr(out, torch.int32), nat.ptr(post, torch.float32 if quant is None else torch.int16), nat.current_stream(dev))
        if quant is not None:
            nat.check(nat.lib().vaeq_ldpc_decode_q(R, C_, N, w, int(t0), 0 if depth is None else int(depth), *head, quant["bits"], quant["app_bits"],
                                                   quant["scale"], quant["num"], quant["beta"], *tail), "vaeq_ldpc_decode_q")
        elif depth is None:
            nat.check(nat.lib().vaeq_ldpc_decode(R, C_, N, w, int(t0), *head, float(alpha), *tail), "vaeq_ldpc_decode")
        else:
            nat.check(nat.lib().vaeq_ldpc_decode_il(R, C_, N, w, int(t0), int(depth), *head, float(alpha), *tail), "vaeq_ldpc_decode_il")
    _, ret = _ldpc_figures(out, C_, n)
    if want_post:
        ret["post"] = post
    if quant is not None:
        ret["quant"] = quant
    if outer is not None:
        ret["outer"] = bch_outer(post, bits, outer["code"], n, t0=t0, depth=depth, payload=outer["payload"], spread=outer["spread"],
                                 codewords=outer["codewords"])
    return ret


class ScLdpcCode:
    """A spatially coupled LDPC code for ldpc_sc_decode: components[ms + 1, mb, nb] of circulant shifts (-1 = a zero block, 0 <= s < Z as in
    LdpcCode) coupled into a terminated chain of L positions.  Block row (t, l), t = 0 .. L + ms - 1, holds components[t - i, l, c] in block
    column (i, c) for 0 <= t - i <= ms.  .ms, .mb, .nb, .Z, .L; .n = L nb Z bits (n_chain), .m = (L + ms) mb Z checks, .rate = the design rate
    1 - (L + ms) mb / (L nb).  The decoder's envelope is vaeq_ldpc_sc_decode's to refuse."""

    def __init__(self, components, Z, L):
        import numpy as np
        self.components = np.ascontiguousarray(np.asarray(components, dtype=np.int32))
        if self.components.ndim != 3 or self.components.shape[0] < 1:
            raise ValueError(f"expected components[ms + 1, mb, nb], got shape {self.components.shape}")
        self.Z, self.L = int(Z), int(L)
        if self.L < 1:
            raise ValueError(f"a chain has at least one position, got L={L}")
        self.ms = int(self.components.shape[0]) - 1
        self.mb, self.nb = (int(d) for d in self.components.shape[1:])
        self.n, self.m = self.L * self.nb * self.Z, (self.L + self.ms) * self.mb * self.Z
        self.rate = 1.0 - (self.L + self.ms) * self.mb / (self.L * self.nb)

    def coupled(self):
        """The LdpcCode of the coupled shifts[(L + ms) mb, L nb] (for tests and small chains)."""
        import numpy as np
        s = np.full(((self.L + self.ms) * self.mb, self.L * self.nb), -1, np.int32)
        for i in range(self.L):
            for d in range(self.ms + 1):
                s[(i + d) * self.mb:(i + d + 1) * self.mb, i * self.nb:(i + 1) * self.nb] = self.components[d]
        return LdpcCode(s, self.Z)


def sc_array_code(ms, nb, Z, L):
    """The coupled array code: mb = 1, shift (2^d (2c + 1)) mod Z in component d, column c; column weight ms + 1, row weight (ms + 1) nb.
    For a prime Z > (2 nb - 1) 2^ms the coupled matrix has no 4-cycles.  Why: write b = 2c + 1, odd and at most 2 nb - 1.  A 4-cycle joins two
    row blocks t > t' and two block columns, b at offsets d, d' and b' at offsets e, e' with d - d' = e - e' = t - t' = k, and needs
    b (2^d - 2^d') = b' (2^e - 2^e') mod Z, that is b 2^d' (2^k - 1) = b' 2^e' (2^k - 1).  0 < 2^k - 1 < Z is invertible modulo the prime Z,
    so b 2^d' = b' 2^e' mod Z; both sides are integers below Z, so they are equal as integers, and an odd number times a power of two factors
    in one way: b = b' and d' = e', the same block column twice.  tests/test_ref_ldpc_sc_host.py checks H^T H."""
    import numpy as np
    d, c = np.arange(int(ms) + 1)[:, None, None], np.arange(int(nb))[None, None, :]
    return ScLdpcCode((2 ** d * (2 * c + 1)) % int(Z), Z, L)


def ldpc_sc_decode(llr, bits, code, window, t0=0, chains=None, iters=10, alpha=None, test=None, want_post=False, want_profile=False, outer=None,
                   quant=None):
    """Post-FEC figures of per-bit LLRs under a spatially coupled code on the device (vaeq_ldpc_sc_decode): a window of `window` row-block
    positions slides along the chain of the ScLdpcCode `code`; at each of the P = max(1, L + ms - window + 1) positions at most `iters`
    iterations of ldpc_decode's layered normalized min-sum over the rows inside, until the rows of the first `test` positions of the window
    (default ms + 1: the rows that touch the block about to leave) are satisfied.  llr, bits, t0 and the bit map as for ldpc_decode with
    n = code.n; chains: per run, default the most that fit behind t0.  alpha defaults to 0.75.
    -> ldpc_decode's dict, a chain where it has a codeword (iters [R,C]: the sum over the positions; ok: every position's last test passed; FER:
    the share of chains with bit_err > 0), plus iters_max [R,C] (the most iterations at one position) and positions (P).  want_post:
    post[R,C,n] f32.  want_profile: pos_err [R,C,L] (the errors of each column block in its final state) and pos_iters [R,C,P].
    outer: as for ldpc_decode, bch_outer over the final LLRs seen as [R, C L, nb Z]: every column block is a codeword of nb Z bits under the
    same bit map, its first (nb - mb) Z bits the default payload.  No interleaver here.
    quant: ldpc_decode's dict(bits, scale=None, app_bits=None, num=6, beta=0) with its defaults decodes in fixed point instead
    (vaeq_ldpc_sc_decode_q): the same window with ldpc_decode's integer layer rule, which sees the scale of the LLRs.  alpha is a ValueError
    then; post is int16, erased counts what the quantiser rounded to zero, and the resolved dict comes back under "quant"."""
    if not isinstance(code, ScLdpcCode):
        raise ValueError(f"ldpc_sc_decode takes an ScLdpcCode, got {code!r}")
    if outer is not None:
        outer = resolve_outer(outer, code)
    alpha, quant = _ldpc_rule(alpha, quant)
    test = code.ms + 1 if test is None else test
    dev, R, N, w, llr, bits = _ldpc_frame(llr, bits)
    n = code.n
    C_ = _ldpc_count(chains, "chain", N, w, n, t0, None)
    P = max(1, code.L + code.ms - int(window) + 1)
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 6, dtype=torch.int32, device=dev)
    post_t = torch.float32 if quant is None else torch.int16
    post = torch.empty(R, Cn, n, dtype=post_t, device=dev) if want_post or outer is not None else None
    pos_err = torch.empty(R, Cn, code.L, dtype=torch.int32, device=dev) if want_profile else None
    pos_iters = torch.empty(R, Cn, P, dtype=torch.int32, device=dev) if want_profile else None
    with torch.cuda.device(dev):
        head = (R, C_, N, w, int(t0), code.ms, code.mb, code.nb, code.Z, code.L, code.components.ctypes.data_as(C.c_void_p), nat.ptr(llr),
                nat.ptr(bits, torch.int8), int(window), int(test))
        tail = (int(iters), nat.ptr(out, torch.int32), nat.ptr(post, post_t), nat.ptr(pos_err, torch.int32), nat.ptr(pos_iters, torch.int32),
                nat.current_stream(dev))
        if quant is not None:
            nat.check(nat.lib().vaeq_ldpc_sc_decode_q(*head, quant["bits"], quant["app_bits"], quant["scale"], quant["num"], quant["beta"], *tail),
                      "vaeq_ldpc_sc_decode_q")
        else:
            nat.check(nat.lib().vaeq_ldpc_sc_decode(*head, float(alpha), *tail), "vaeq_ldpc_sc_decode")
    o, ret = _ldpc_figures(out, C_, n)
    ret.update(iters_max=o[..., 5], positions=P)
    if want_post:
        ret["post"] = post
    if want_profile:
        ret["pos_err"], ret["pos_iters"] = pos_err.long(), pos_iters.long()
    if quant is not None:
        ret["quant"] = quant
    if outer is not None:
        ret["outer"] = bch_outer(post.view(R, Cn * code.L, code.nb * code.Z), bits, outer["code"], code.nb * code.Z, t0=t0, payload=outer["payload"],
                                 spread=outer["spread"], codewords=outer["codewords"])
    return ret


class BchCode:
    """A narrow-sense primitive binary BCH code over GF(2^m) with designed correction t, shortened to n bits (default 2^m - 1), for bch_outer:
    .m, .t, .n, .parity (the size of the union of the cyclotomic cosets of 1 .. 2t modulo 2^m - 1), .k = n - parity, .rate = k / n.  ValueError
    outside vaeq_bch_outer's envelope: m in 4 .. 13, t in 1 .. 16, parity < n <= 2^m - 1."""

    def __init__(self, m, t, n=None):
        import numbers
        if any(not isinstance(x, numbers.Integral) or isinstance(x, bool) for x in (m, t) + (() if n is None else (n,))):
            raise ValueError(f"BchCode takes integers, got m={m!r}, t={t!r}, n={n!r}")
        self.m, self.t = int(m), int(t)
        if not 4 <= self.m <= 13 or not 1 <= self.t <= 16:
            raise ValueError(f"BchCode: m in 4 .. 13 and t in 1 .. 16, got m={m}, t={t}")
        q = (1 << self.m) - 1
        seen = set()
        for j in range(1, 2 * self.t + 1):
            x = j % q
            while x not in seen:
                seen.add(x)
                x = 2 * x % q
        self.parity = len(seen)
        self.n = q if n is None else int(n)
        if not self.parity < self.n <= q:
            raise ValueError(f"BchCode({m}, {t}): {self.parity} parity bits need {self.parity} < n <= {q}, got n={self.n}")
        self.k = self.n - self.parity
        self.rate = self.k / self.n


OUTER_KEYS = ("code", "payload", "spread", "codewords")
OUTER_POST_BYTES = 256 << 20                               # fec_figures with an outer code: the most bytes of `post` alive at a time


def resolve_outer(outer, code=None):
    """ldpc_decode's outer= dict(code, payload=None, spread=True, codewords=None) with its defaults filled in; code: the LdpcCode in front, whose
    (nb - mb) Z is the default payload.  ValueError for an unknown key, a missing code or one that is no BchCode, a payload outside 1 .. n."""
    if not isinstance(outer, dict) or set(outer) - set(OUTER_KEYS) or not isinstance(outer.get("code"), BchCode):
        raise ValueError(f"outer takes a dict of {', '.join(OUTER_KEYS)} with a BchCode under code; got {sorted(outer) if isinstance(outer, dict) else outer!r}")
    payload = outer.get("payload")
    if payload is None and code is not None:
        payload = (code.nb - code.mb) * code.Z
    n = None if code is None else code.nb * code.Z             # (a column block of an ScLdpcCode is the codeword of the outer decoder's map)
    if payload is not None and (int(payload) < 1 or (n is not None and int(payload) > n)):
        raise ValueError(f"outer['payload'] = {payload}: the first 1 .. n bits of a codeword")
    return dict(code=outer["code"], payload=None if payload is None else int(payload), spread=bool(outer.get("spread", True)),
                codewords=outer.get("codewords"))


def bch_outer(post, bits, code, n, t0=0, depth=None, payload=None, spread=True, codewords=None, want_loc=False):
    """The hard-decision outer decoder behind ldpc_decode (vaeq_bch_outer): bounded-distance decoding of the BchCode `code` over the payload
    bits of post[R, C, n] (float32 or int16: ldpc_decode's post; a negative value is bit 1) against the TX bits `bits` ([R,2,2b,N] or [R,w,N],
    as for ldpc_decode, with its t0 and depth).  No encoder: the figures depend on the error pattern alone.  payload: the first K bits of every
    LDPC codeword are payload (default n: all of them; ldpc_decode's outer= defaults to (nb - mb) Z); the run's stream of C K bits holds
    `codewords` outer codewords (default C K // code.n; ValueError if none fits), bit-interleaved over the run if spread (position p of outer
    codeword a is stream bit p C_o + a) and back to back otherwise.
    -> dict(status, pre_err, bit_err, nflip [R,C_o] int64: status 0 = zero syndromes, 1 = corrected nflip <= t positions, 2 = detected and left
    alone; BER_outer[R], BER_in[R] f32 over the C_o n_o bits, FER_outer[R] the share of outer codewords with bit_err > 0; miscorrected[R]
    (status 1 with bit_err > 0) and undetected[R] (status 0 with pre_err > 0) int64; loc[R,C_o,t] int16, the flipped positions ascending and
    padded with -1, if want_loc)."""
    if not isinstance(code, BchCode):
        raise ValueError(f"bch_outer takes a BchCode, got {code!r}")
    if post.dim() != 3 or post.shape[2] != int(n) or post.dtype not in (torch.float32, torch.int16) or bits.dim() not in (3, 4) or bits.shape[0] != post.shape[0]:
        raise ValueError(f"expected post[R,C,{n}] float32 or int16 and bits[R,2,2b,N] or [R,w,N], got {tuple(post.shape)} {post.dtype}, {tuple(bits.shape)}")
    dev, R, C_, N = post.device, post.shape[0], post.shape[1], bits.shape[-1]
    post = post.contiguous()
    w = bits.shape[1] * (bits.shape[2] if bits.dim() == 4 else 1)
    bits = bits.reshape(R, w, N).contiguous()                  # (an empty batch leaves a -1 ambiguous)
    K = int(n) if payload is None else int(payload)
    if not 1 <= K <= int(n):
        raise ValueError(f"payload = {K}: the first 1 .. {n} bits of a codeword")
    Co = C_ * K // code.n if codewords is None else int(codewords)
    if codewords is None and Co < 1:
        raise ValueError(f"no outer codeword of {code.n} bits fits into the {C_} x {K} payload bits of a run")
    out = torch.empty(R, max(Co, 0), 4, dtype=torch.int32, device=dev)
    loc = torch.empty(R, max(Co, 0), code.t, dtype=torch.int16, device=dev) if want_loc else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_bch_outer(R, C_, N, w, int(t0), 0 if depth is None else int(depth), int(n), K, code.m, code.t, code.n, Co,
                                           int(bool(spread)), nat.ptr(post, post.dtype), int(post.dtype == torch.int16), nat.ptr(bits, torch.int8),
                                           nat.ptr(out, torch.int32), nat.ptr(loc, torch.int16), nat.current_stream(dev)), "vaeq_bch_outer")
    o = out.long()
    tot = torch.full((R,), float(max(Co * code.n, 1)), dtype=torch.float64, device=dev)
    ret = dict(status=o[..., 0], pre_err=o[..., 1], bit_err=o[..., 2], nflip=o[..., 3],
               BER_outer=(o[..., 2].sum(1).double() / tot).float(), BER_in=(o[..., 1].sum(1).double() / tot).float(),
               FER_outer=((o[..., 2] > 0).sum(1).double() / torch.full_like(tot, float(max(Co, 1)))).float(),
               miscorrected=((o[..., 0] == 1) & (o[..., 2] > 0)).sum(1), undetected=((o[..., 0] == 0) & (o[..., 1] > 0)).sum(1))
    if want_loc:
        ret["loc"] = loc
    return ret


class StaircaseCode:
    """A staircase code for staircase_decode: a chain of L blocks of s x s bits over the BchCode `component`, whose even length is 2 s.  Component
    j of pair i is the word [column j of block i - 1 | row j of block i]; block 0 is all zero and is not transmitted.  .component, .L, .s = n // 2,
    .n = L s^2 bits (n_chain), .rate = 1 - parity / s.  A rate of zero or below is allowed: that is a decoder test, not a code.  ValueError
    outside vaeq_staircase_decode's envelope: m in 4 .. 10, t in 1 .. 8, s in 2 .. 511, L in 1 .. 65535."""

    def __init__(self, component, L):
        import numbers
        if not isinstance(component, BchCode):
            raise ValueError(f"StaircaseCode takes a BchCode as its component, got {component!r}")
        if not isinstance(L, numbers.Integral) or isinstance(L, bool) or not 1 <= int(L) <= 65535:
            raise ValueError(f"StaircaseCode: a chain of 1 .. 65535 blocks, got L={L!r}")
        if component.n % 2 or not 4 <= component.m <= 10 or not 1 <= component.t <= 8 or not 2 <= component.n // 2 <= 511:
            raise ValueError(f"StaircaseCode: a component with m in 4 .. 10, t in 1 .. 8 and an even n = 2 s, s in 2 .. 511; got m={component.m}, "
                             f"t={component.t}, n={component.n}")
        self.component, self.L, self.s = component, int(L), component.n // 2
        self.n = self.L * self.s * self.s
        self.rate = 1.0 - component.parity / self.s


def staircase_decode(llr, bits, code, window, t0=0, chains=None, iters=8, want_hard=False, want_profile=False):
    """Post-FEC figures of per-bit LLRs behind a hard-decision staircase code on the device (vaeq_staircase_decode): the hard decisions llr < 0
    against the TX bits give the error pattern of every chain of the StaircaseCode `code`; a window of `window` pairs of neighbouring blocks
    slides along the chain, and at each of the P = max(1, L - window + 1) positions the pairs inside are decoded component by component, at most
    `iters` times, until an iteration flips nothing.  llr, bits, t0 and the bit map as for ldpc_decode with n = code.n; chains: per run, default
    the most that fit behind t0.  No encoder: the figures depend on the error pattern alone.
    -> ldpc_sc_decode's dict, a chain where it has one (iters [R,C]: the sum over the positions; ok: at every position the last iteration found
    every component clean; bit_err, pre_err, erased, iters_max [R,C] int64; positions (P); BER_post[R], BER_pre[R], FER[R] f32), plus nflip and
    bad_flips [R,C] (all flips, and those of a bit that was right at that moment: what miscorrection costs).  want_hard: hard[R,C,n] int8, the
    final decisions.  want_profile: pos_err [R,C,L] (the errors of each block in its final state; the last block has one component per bit and
    keeps more than the steady state) and pos_iters [R,C,P]."""
    if not isinstance(code, StaircaseCode):
        raise ValueError(f"staircase_decode takes a StaircaseCode, got {code!r}")
    if llr.shape != bits.shape or llr.dim() not in (3, 4):
        raise ValueError(f"expected llr and bits of one shape [R,2,2b,N] or [R,w,N], got {tuple(llr.shape)}, {tuple(bits.shape)}")
    dev, R, N = llr.device, llr.shape[0], llr.shape[-1]
    llr = llr.reshape(R, -1, N).contiguous()
    bits = bits.reshape(R, -1, N).contiguous()
    w, n = llr.shape[1], code.n
    C_ = int(chains) if chains is not None else _ldpc_fit(N, w, n, t0, None)
    if chains is None and C_ < 1:
        raise ValueError(f"no chain of {n} bits fits into {N - int(t0)} symbols of {w} bits")
    P = max(1, code.L - int(window) + 1)
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 8, dtype=torch.int32, device=dev)
    hard = torch.empty(R, Cn, n, dtype=torch.int8, device=dev) if want_hard else None
    pos_err = torch.empty(R, Cn, code.L, dtype=torch.int32, device=dev) if want_profile else None
    pos_iters = torch.empty(R, Cn, P, dtype=torch.int32, device=dev) if want_profile else None
    bch = code.component
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_staircase_decode(R, C_, N, w, int(t0), bch.m, bch.t, code.s, code.L, nat.ptr(llr), nat.ptr(bits, torch.int8),
                                                  int(window), int(iters), nat.ptr(out, torch.int32), nat.ptr(hard, torch.int8),
                                                  nat.ptr(pos_err, torch.int32), nat.ptr(pos_iters, torch.int32), nat.current_stream(dev)),
                  "vaeq_staircase_decode")
    o = out.long()
    tot = torch.full((R,), float(max(C_ * n, 1)), dtype=torch.float64, device=dev)
    ret = dict(iters=o[..., 0], ok=o[..., 1], bit_err=o[..., 2], pre_err=o[..., 3], erased=o[..., 4],
               BER_post=(o[..., 2].sum(1).double() / tot).float(), BER_pre=(o[..., 3].sum(1).double() / tot).float(),
               FER=((o[..., 2] > 0).sum(1).double() / torch.full_like(tot, float(max(C_, 1)))).float(), iters_max=o[..., 5], positions=P,
               nflip=o[..., 6], bad_flips=o[..., 7])
    if want_hard:
        ret["hard"] = hard
    if want_profile:
        ret["pos_err"], ret["pos_iters"] = pos_err.long(), pos_iters.long()
    return ret


class HammingCode:
    """A single-error-correcting code for chase_decode, given by the columns of its parity-check matrix: cols[n], column j an r-bit integer.
    .n, .r, .cols (int32), .rank (of the columns over GF(2)), .k = n - rank, .rate = k / n.  ValueError outside vaeq_chase_decode's envelope: n in
    3 .. 256, r in 2 .. 10, integer columns that are distinct, non-zero and below 2^r.  hamming_code builds the two textbook families; a standard's
    own matrix (the OIF 400ZR (128,119) word among them) is not in this package: a user who has its columns passes them here."""

    def __init__(self, cols, r):
        import numbers
        import numpy as np
        if not isinstance(r, numbers.Integral) or isinstance(r, bool) or not 2 <= int(r) <= 10:
            raise ValueError(f"HammingCode: r in 2 .. 10, got {r!r}")
        c = np.asarray(cols)
        if c.ndim != 1 or not 3 <= c.size <= 256 or c.dtype == bool or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"HammingCode: 3 .. 256 integer columns, got {c.dtype} of shape {c.shape}")
        if (c < 1).any() or (c >= 1 << int(r)).any() or np.unique(c).size != c.size:
            raise ValueError(f"HammingCode: the columns are distinct, non-zero and below 2^{int(r)}")
        self.cols, self.n, self.r = np.ascontiguousarray(c.astype(np.int32)), int(c.size), int(r)
        basis = {}                                             # leading bit -> a reduced column: Gaussian elimination over GF(2)
        for x in (int(v) for v in self.cols):
            while x and x.bit_length() in basis:
                x ^= basis[x.bit_length()]
            if x:
                basis[x.bit_length()] = x
        self.rank = len(basis)
        self.k = self.n - self.rank
        self.rate = self.k / self.n


def hamming_code(m, extended=True, n=None):
    """The HammingCode of the textbook column rules, shortened to its first n columns: extended (d = 4): r = m + 1, cols[j] = (j << 1) | 1,
    n <= 2^m (the default); plain (d = 3): r = m, cols[j] = j + 1, n <= 2^m - 1 (the default).  hamming_code(7) is the extended (128, 120) code,
    hamming_code(3, extended=False) the perfect (7, 4) code.  .k = n - r wherever the kept columns have rank r.  This is NOT the (128, 119) matrix of
    the OIF 400ZR agreement, which this package does not hold: pass its columns to HammingCode."""
    import numbers
    import numpy as np
    if not isinstance(m, numbers.Integral) or isinstance(m, bool) or (n is not None and (not isinstance(n, numbers.Integral) or isinstance(n, bool))):
        raise ValueError(f"hamming_code takes integers, got m={m!r}, n={n!r}")
    m, full = int(m), (1 << int(m)) - (0 if extended else 1) if 1 <= int(m) <= 10 else 0
    n = full if n is None else int(n)
    if not 1 <= n <= full:
        raise ValueError(f"hamming_code({m}, extended={bool(extended)}): n in 1 .. {full}, got {n}")
    j = np.arange(n, dtype=np.int64)
    return HammingCode((j << 1) | 1 if extended else j + 1, m + 1 if extended else m)


class EbchCode:
    """An (extended) double-error-correcting BCH code for chase_decode and ProductCode (vaeq_chase_bch_decode): vaeq_bch_outer's narrow-sense
    primitive binary BCH code over GF(2^m) with designed correction t = 2, shortened to n_i inner bits and, where `extended`, followed by one
    overall parity bit: n = n_i + extended (default the full length, 2^m - 1 + extended).  .m, .n, .n_i, .extended, .k = n_i - 2 m,
    .rate = k / n.  EbchCode(7) is the extended (128, 113) word, d = 6.  ValueError outside the envelope: m in 4 .. 8, 2 m < n_i <= 2^m - 1.
    t = 3 and beyond are out of scope."""

    def __init__(self, m, n=None, extended=True):
        import numbers
        if not isinstance(m, numbers.Integral) or isinstance(m, bool) or (n is not None and (not isinstance(n, numbers.Integral) or isinstance(n, bool))):
            raise ValueError(f"EbchCode takes integers, got m={m!r}, n={n!r}")
        if not 4 <= int(m) <= 8:
            raise ValueError(f"EbchCode: m in 4 .. 8, got {m!r}")
        ext = int(bool(extended))
        m, n = int(m), (1 << int(m)) - 1 + ext if n is None else int(n)
        if not 2 * m < n - ext <= (1 << m) - 1:
            raise ValueError(f"EbchCode(m={m}, extended={bool(ext)}): n in {2 * m + 1 + ext} .. {(1 << m) - 1 + ext}, got {n}")
        self.m, self.n, self.n_i, self.extended = m, n, n - ext, bool(ext)
        self.k = self.n_i - 2 * m
        self.rate = self.k / self.n

    def __repr__(self):
        return f"EbchCode(m={self.m}, n={self.n}, extended={self.extended})"


def ebch_code(m, extended=True, n=None):
    """The EbchCode over GF(2^m), shortened to n bits in all (the parity bit included), in the style of hamming_code: ebch_code(5) is the extended
    (32, 21) word, ebch_code(4, extended=False) the (15, 7) code, ebch_code(8, n=201) the inner 200 bits of the (255, 239) code and a parity bit."""
    return EbchCode(m, n, extended)


def chase_decode(llr, bits, code, t0=0, codewords=None, depth=None, patterns=4, payload=None, spread=True, want_stream=False):
    """The soft-in / hard-out inner decoder in front of the hard-decision FEC (vaeq_chase_decode; vaeq_chase_bch_decode where `code` is an
    EbchCode, whose test patterns are completed by bounded-distance decoding of up to two errors and the parity bit): Chase decoding of `code` over
    per-bit LLRs against the TX bits (no encoder: the rule acts on the error pattern).  llr, bits, t0, depth and the bit map as for ldpc_decode with
    n = code.n; codewords: per run, default the most that fit behind t0.  patterns = p in 0 .. min(6, n): the 2^p test patterns over the p least
    reliable positions, each completed by syndrome decoding; the candidate with the smallest sum of |llr| over its flips wins.  p = 0 is plain
    syndrome decoding of the hard decisions.  payload: the first K bits of every codeword (default code.k).
    -> dict(status, pre_err, bit_err, nflip, erased, pay_err [R,C] int64: status 0 = zero syndrome, 1 = flipped nflip bits, 2 = no candidate,
    left alone; bit_err the errors after decoding over the n bits, pay_err those among the payload; BER_post[R], BER_pre[R] over the C n bits,
    BER_payload[R] over the C K payload bits, FER[R] the share of codewords with bit_err > 0, f32; miscorrected[R] (status 1 with bit_err > 0) and
    undetected[R] (status 0 with pre_err > 0) int64).  want_stream: stream = dict(llr[R,1,C K] f32, bits[R,1,C K] int8), the decided payload
    bits as +-1.0 and their TX bits, codeword after codeword or, with spread, bit-interleaved over the run (payload bit i of codeword c at
    i C + c): a valid input of every decoder here with t0 = 0, which is how staircase_decode runs behind this one."""
    if not isinstance(code, (HammingCode, EbchCode)):
        raise ValueError(f"chase_decode takes a HammingCode or an EbchCode, got {code!r}")
    if llr.shape != bits.shape or llr.dim() not in (3, 4):
        raise ValueError(f"expected llr and bits of one shape [R,2,2b,N] or [R,w,N], got {tuple(llr.shape)}, {tuple(bits.shape)}")
    dev, R, N = llr.device, llr.shape[0], llr.shape[-1]
    llr = llr.reshape(R, -1, N).contiguous()
    bits = bits.reshape(R, -1, N).contiguous()
    w, n = llr.shape[1], code.n
    C_ = int(codewords) if codewords is not None else _ldpc_fit(N, w, n, t0, depth)
    if codewords is None and C_ < 1:
        raise ValueError(f"no codeword of {n} bits fits into {N - int(t0)} symbols of {w} bits")
    K = code.k if payload is None else int(payload)
    if not 1 <= K <= n:
        raise ValueError(f"payload = {K}: the first 1 .. {n} bits of a codeword")
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 6, dtype=torch.int32, device=dev)
    s_llr = torch.empty(R, 1, Cn * K, dtype=torch.float32, device=dev) if want_stream else None
    s_bits = torch.empty(R, 1, Cn * K, dtype=torch.int8, device=dev) if want_stream else None
    tail = (nat.ptr(llr), nat.ptr(bits, torch.int8), int(patterns), K, int(bool(spread)), nat.ptr(out, torch.int32), nat.ptr(s_llr),
            nat.ptr(s_bits, torch.int8), nat.current_stream(dev))
    with torch.cuda.device(dev):
        if isinstance(code, EbchCode):
            nat.check(nat.lib().vaeq_chase_bch_decode(R, C_, N, w, int(t0), 0 if depth is None else int(depth), code.m, n, int(code.extended), *tail),
                      "vaeq_chase_bch_decode")
        else:
            nat.check(nat.lib().vaeq_chase_decode(R, C_, N, w, int(t0), 0 if depth is None else int(depth), n, code.r,
                                                  code.cols.ctypes.data_as(C.c_void_p), *tail), "vaeq_chase_decode")
    o = out.long()
    tot = torch.full((R,), float(max(C_ * n, 1)), dtype=torch.float64, device=dev)
    ret = dict(status=o[..., 0], pre_err=o[..., 1], bit_err=o[..., 2], nflip=o[..., 3], erased=o[..., 4], pay_err=o[..., 5],
               BER_post=(o[..., 2].sum(1).double() / tot).float(), BER_pre=(o[..., 1].sum(1).double() / tot).float(),
               BER_payload=(o[..., 5].sum(1).double() / torch.full_like(tot, float(max(C_ * K, 1)))).float(),
               FER=((o[..., 2] > 0).sum(1).double() / torch.full_like(tot, float(max(C_, 1)))).float(),
               miscorrected=((o[..., 0] == 1) & (o[..., 2] > 0)).sum(1), undetected=((o[..., 0] == 0) & (o[..., 1] > 0)).sum(1))
    if want_stream:
        ret["stream"] = dict(llr=s_llr, bits=s_bits)
    return ret


class ProductCode:
    """A product code for tpc_decode: blocks of col.n x row.n bits whose columns are words of the HammingCode `col` and whose rows are words of
    the HammingCode `row`.  .col, .row, .n = col.n row.n, .k = col.k row.k, .rate = k / n.  ValueError for anything but two HammingCodes, or a
    block whose state passes the LDS bound of vaeq_tpc_decode (include/vaeq.h; the extended (128, 120)^2 block fits).  Or two EbchCodes, which
    may differ in m, n and extended (vaeq_tpc_bch_decode; the extended (128, 113)^2 block fits, the (256, 239)^2 block does not).  .bch says which.
    One code of each kind is a ValueError: a mixed product is out of scope."""

    def __init__(self, col, row):
        self.bch = isinstance(col, EbchCode) and isinstance(row, EbchCode)
        if not self.bch and (not isinstance(col, HammingCode) or not isinstance(row, HammingCode)):
            raise ValueError(f"ProductCode takes two HammingCodes or two EbchCodes, got {col!r} and {row!r}")
        self.col, self.row = col, row
        self.n, self.k = col.n * row.n, col.k * row.k
        self.rate = self.k / self.n
        fits = (nat.lib().vaeq_tpc_bch_lds_bytes(col.m, col.n, int(col.extended), row.m, row.n, int(row.extended)) if self.bch
                else nat.lib().vaeq_tpc_lds_bytes(col.n, col.r, row.n, row.r))
        if fits < 0:
            raise ValueError(f"ProductCode: the state of a block of {col.n} x {row.n} bits does not fit the LDS of a CU (vaeq_tpc_lds_bytes)")


TPC_ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)          # Pyndiah's schedules per half-iteration, continued with 1
TPC_BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
TPC_CLIP = 2.0 ** 60


def _tpc_schedule(name, given, default, iters, hi):
    """-> float32[2 iters]: `given` (2 iters values) or the default continued with 1; ValueError outside vaeq_tpc_decode's bounds."""
    import numpy as np
    if given is None:
        v = np.array((list(default) + [1.0] * (2 * iters))[:2 * iters], np.float32)
    else:
        try:
            v = np.ascontiguousarray(np.asarray(given, dtype=np.float32).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError(f"{name}: 2 iters = {2 * iters} numbers, got {given!r}") from None
    if v.shape != (2 * iters,) or not np.isfinite(v).all() or (v < 0).any() or (hi is not None and (v > hi).any()):
        raise ValueError(f"{name}: 2 iters = {2 * iters} finite values in [0, {'inf' if hi is None else hi}{')' if hi is None else ']'}, got {given!r}")
    return v


def resolve_tpc(code, iters=4, patterns=4, alpha=None, beta=None, clip=None, payload=None):
    """tpc_decode's host-side arguments with their defaults filled in -> dict(iters, patterns, alpha, beta (float32[2 iters]), clip, payload
    (K1, K2)).  ValueError outside vaeq_tpc_decode's bounds."""
    import math
    import numbers
    if not isinstance(code, ProductCode):
        raise ValueError(f"tpc_decode takes a ProductCode, got {code!r}")
    for name, v, lo, hi in (("iters", iters, 1, 16), ("patterns", patterns, 0, min(6, code.col.n, code.row.n))):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError(f"{name} = {v!r}: an integer in {lo} .. {hi}")
    iters = int(iters)
    clip = TPC_CLIP if clip is None else clip
    if not isinstance(clip, numbers.Real) or isinstance(clip, bool) or not math.isfinite(clip) or not 0 < clip <= 2.0 ** 96:
        raise ValueError(f"clip = {clip!r}: finite, in (0, 2^96]")
    K = (code.col.k, code.row.k) if payload is None else payload
    if (not isinstance(K, (tuple, list)) or len(K) != 2 or any(not isinstance(v, numbers.Integral) or isinstance(v, bool) for v in K)
            or not 1 <= K[0] <= code.col.n or not 1 <= K[1] <= code.row.n):
        raise ValueError(f"payload = {K!r}: (K1, K2), the first 1 .. {code.col.n} rows and 1 .. {code.row.n} columns of a block")
    return dict(iters=iters, patterns=int(patterns), alpha=_tpc_schedule("alpha", alpha, TPC_ALPHA, iters, 16.0),
                beta=_tpc_schedule("beta", beta, TPC_BETA, iters, None), clip=float(clip), payload=(int(K[0]), int(K[1])))


def tpc_decode(llr, bits, code, t0=0, blocks=None, iters=4, patterns=4, alpha=None, beta=None, scale=None, clip=None, payload=None,
               want_stream=False, want_ext=False, want_profile=False):
    """Post-FEC figures of per-bit LLRs behind a soft-decision turbo product code on the device (vaeq_tpc_decode): Chase-Pyndiah decoding of the
    ProductCode `code`, rows in the even half-iterations and columns in the odd ones, at most 2 iters of them, each word by a Chase decoder over
    2^patterns test patterns whose competing candidates give the extrinsic values (vaeq_tpc_bch_decode where the code holds two EbchCodes: the same
    rule over double-error-correcting words).  llr, bits, t0 and the bit map as for ldpc_decode with
    n = code.n; blocks: per run, default the most that fit behind t0.  No encoder: the rule is stated on the LLRs towards the TX bits.
    alpha, beta: 2 iters values per half-iteration, default Pyndiah's schedules (0, .2, .3, .5, .7, .9, 1, 1 and .2, .4, .6, .8, 1, 1, continued
    with 1).  scale: per run ([R] tensor or a number), the unit of beta; default the float32 mean of |llr| over the run's tensor, non-finite
    entries counted as 0, formed on the device without a host synchronisation.  Unlike min-sum LDPC decoding the result depends on the scale of
    the LLRs.  clip: the bound of |r| and |W|, default 2^60.  payload = (K1, K2): the first rows and columns of a block, default (col.k, row.k).
    -> staircase_decode's common keys (iters [R,C]: half-iterations executed; ok: stopped on a product codeword; bit_err, pre_err, erased [R,C]
    int64; BER_post[R], BER_pre[R], FER[R] f32) plus pay_err, nstat2 (words without a candidate), nbeta (positions without a competitor) [R,C],
    BER_payload[R] over the C K1 K2 payload bits, and the resolved alpha, beta (tuples of float), scale ([R] f32) and clip.  want_stream:
    stream = dict(llr[R,1,C n] f32, bits[R,1,C n] int8), the decided bits as +-1.0 and their TX bits, a valid input of every decoder here with
    t0 = 0.  want_ext: ext[R,C,n] f32, the extrinsic values after the last executed half-iteration.  want_profile: half_err[R,C,2 iters] int64,
    the errors after each executed half-iteration, -1 behind the stop."""
    prm = resolve_tpc(code, iters, patterns, alpha, beta, clip, payload)
    if llr.shape != bits.shape or llr.dim() not in (3, 4):
        raise ValueError(f"expected llr and bits of one shape [R,2,2b,N] or [R,w,N], got {tuple(llr.shape)}, {tuple(bits.shape)}")
    dev, R, N = llr.device, llr.shape[0], llr.shape[-1]
    llr = llr.reshape(R, -1, N).contiguous()
    bits = bits.reshape(R, -1, N).contiguous()
    w, n = llr.shape[1], code.n
    C_ = int(blocks) if blocks is not None else _ldpc_fit(N, w, n, t0, None)
    if blocks is None and C_ < 1:
        raise ValueError(f"no block of {n} bits fits into {N - int(t0)} symbols of {w} bits")
    if scale is None:
        scale = torch.where(torch.isfinite(llr), llr.abs(), torch.zeros((), dtype=llr.dtype, device=dev)).mean(dim=(1, 2), dtype=torch.float32)
    elif not torch.is_tensor(scale):
        scale = torch.full((R,), float(scale), dtype=torch.float32, device=dev)
    scale = scale.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if scale.shape != (R,):
        raise ValueError(f"scale: one value per run, [{R}], got {tuple(scale.shape)}")
    Cn, H = max(C_, 0), 2 * prm["iters"]
    out = torch.empty(R, Cn, 8, dtype=torch.int32, device=dev)
    s_llr = torch.empty(R, 1, Cn * n, dtype=torch.float32, device=dev) if want_stream else None
    s_bits = torch.empty(R, 1, Cn * n, dtype=torch.int8, device=dev) if want_stream else None
    ext = torch.empty(R, Cn, n, dtype=torch.float32, device=dev) if want_ext else None
    half = torch.empty(R, Cn, H, dtype=torch.int32, device=dev) if want_profile else None
    K1, K2 = prm["payload"]
    tail = (nat.ptr(llr), nat.ptr(bits, torch.int8), prm["patterns"], prm["iters"], prm["alpha"].ctypes.data_as(C.c_void_p),
            prm["beta"].ctypes.data_as(C.c_void_p), nat.ptr(scale) if R else None, prm["clip"], K1, K2, nat.ptr(out, torch.int32), nat.ptr(s_llr),
            nat.ptr(s_bits, torch.int8), nat.ptr(ext), nat.ptr(half, torch.int32), nat.current_stream(dev))
    with torch.cuda.device(dev):
        if code.bch:
            nat.check(nat.lib().vaeq_tpc_bch_decode(R, C_, N, w, int(t0), code.col.m, code.col.n, int(code.col.extended), code.row.m, code.row.n,
                                                    int(code.row.extended), *tail), "vaeq_tpc_bch_decode")
        else:
            nat.check(nat.lib().vaeq_tpc_decode(R, C_, N, w, int(t0), code.col.n, code.col.r, code.col.cols.ctypes.data_as(C.c_void_p), code.row.n,
                                                code.row.r, code.row.cols.ctypes.data_as(C.c_void_p), *tail), "vaeq_tpc_decode")
    o = out.long()
    tot = torch.full((R,), float(max(C_ * n, 1)), dtype=torch.float64, device=dev)
    ret = dict(iters=o[..., 0], ok=o[..., 1], bit_err=o[..., 2], pre_err=o[..., 3], erased=o[..., 4], pay_err=o[..., 5], nstat2=o[..., 6],
               nbeta=o[..., 7], BER_post=(o[..., 2].sum(1).double() / tot).float(), BER_pre=(o[..., 3].sum(1).double() / tot).float(),
               BER_payload=(o[..., 5].sum(1).double() / torch.full_like(tot, float(max(C_ * K1 * K2, 1)))).float(),
               FER=((o[..., 2] > 0).sum(1).double() / torch.full_like(tot, float(max(C_, 1)))).float(),
               alpha=tuple(float(v) for v in prm["alpha"]), beta=tuple(float(v) for v in prm["beta"]), scale=scale, clip=prm["clip"])
    if want_stream:
        ret["stream"] = dict(llr=s_llr, bits=s_bits)
    if want_ext:
        ret["ext"] = ext
    if want_profile:
        ret["half_err"] = half.long()
    return ret


INNER_KEYS = ("code", "patterns", "depth", "payload", "spread")


def resolve_inner(inner):
    """The inner= dict(code=HammingCode or EbchCode, patterns=4, depth=None, payload=None, spread=True) of a fec= with a StaircaseCode, its defaults
    filled in.  ValueError for an unknown key, a missing code or one of another kind, patterns outside 0 .. min(6, n), a payload outside 1 .. n (or a
    code without a payload bit where none is given), a depth below 1."""
    import numbers
    if not isinstance(inner, dict) or set(inner) - set(INNER_KEYS) or not isinstance(inner.get("code"), (HammingCode, EbchCode)):
        raise ValueError(f"inner takes a dict of {', '.join(INNER_KEYS)} with a HammingCode or an EbchCode under code; got {sorted(inner) if isinstance(inner, dict) else inner!r}")
    code = inner["code"]
    patterns, payload, depth = inner.get("patterns", 4), inner.get("payload"), inner.get("depth")
    payload = code.k if payload is None else payload
    for name, v, lo, hi in (("patterns", patterns, 0, min(6, code.n)), ("payload", payload, 1, code.n), ("depth", 1 if depth is None else depth, 1, None)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"inner[{name!r}] = {v!r}: an integer in {lo} .. {'' if hi is None else hi}")
    return dict(code=code, patterns=int(patterns), depth=None if depth is None else int(depth), payload=int(payload), spread=bool(inner.get("spread", True)))


FEC_KEYS = ("code", "t0", "max_iter", "alpha", "depth", "quant", "window", "iters", "test", "fixed", "outer")
FEC_BLOCK_ONLY, FEC_SC_ONLY = ("max_iter", "depth", "quant"), ("window", "iters", "test", "fixed")
FEC_STAIRCASE_KEYS = ("code", "window", "t0", "iters")
FEC_TPC_KEYS = ("code", "t0", "iters", "patterns", "alpha", "beta", "scale", "clip")


def check_fec(fec):
    """ValueError for a fec= dict that fec_figures would refuse (None passes): for a runner to call before it allocates or launches anything."""
    if isinstance(fec, dict) and isinstance(fec.get("code"), ProductCode):
        if set(fec) - set(FEC_TPC_KEYS):
            raise ValueError(f"fec with a ProductCode takes {', '.join(FEC_TPC_KEYS)}; got {sorted(fec)}")
        resolve_tpc(fec["code"], **{k: fec[k] for k in ("iters", "patterns", "alpha", "beta", "clip") if fec.get(k) is not None})
        return
    if isinstance(fec, dict) and isinstance(fec.get("code"), StaircaseCode):
        if set(fec) - set(FEC_STAIRCASE_KEYS) - {"inner"} or fec.get("window") is None:
            raise ValueError(f"fec with a StaircaseCode takes {', '.join(FEC_STAIRCASE_KEYS)}, inner, window required; got {sorted(fec)}")
        if fec.get("inner") is not None:
            resolve_inner(fec["inner"])
        return
    if fec is not None and (set(fec) - set(FEC_KEYS) or "code" not in fec):
        raise ValueError(f"fec takes {', '.join(FEC_KEYS)}; got {sorted(fec)}")
    if fec is not None:
        sc = isinstance(fec["code"], ScLdpcCode)
        wrong = [k for k in (FEC_BLOCK_ONLY if sc else FEC_SC_ONLY) if k in fec]
        if wrong:
            raise ValueError(f"fec with {'an ScLdpcCode' if sc else 'an LdpcCode'} does not take {', '.join(wrong)}")
        if sc and fec.get("window") is None:
            raise ValueError("fec with an ScLdpcCode needs window, the row-block positions inside the decoding window")
    for key in ("quant", "fixed"):                              # the fixed-point rule: quant with an LdpcCode, fixed with an ScLdpcCode
        if fec is not None and fec.get(key) is not None:
            resolve_quant(fec[key])
            if fec.get("alpha") is not None:
                raise ValueError(f"fec takes alpha for the float decoder or {key} for the fixed-point one, not both")
    if fec is not None and fec.get("outer") is not None:
        resolve_outer(fec["outer"], fec["code"])


def _cat_figures(parts):
    """The dicts of the chunks of a batch as one: tensors joined along the runs, nested dicts likewise, anything else (the resolved quant) once."""
    first = parts[0]
    return {k: torch.cat([p[k] for p in parts]) if torch.is_tensor(v) else _cat_figures([p[k] for p in parts]) if k == "outer" else v
            for k, v in first.items()}


def fec_figures(llr, fec):
    """The batch runners' fec= : ldpc_decode of an "llr" dict (llr, bits) under fec = dict(code, t0, max_iter, alpha, depth, quant, outer; all but
    code optional; quant = dict(bits, ...) decodes in fixed point, vaeq_ldpc_decode_q; outer = dict(code=BchCode, ...) adds bch_outer's figures
    under "outer").  With an outer code the runs are walked in chunks whose `post` stays within OUTER_POST_BYTES; codewords are independent, so
    the figures are those of one call.  With an ScLdpcCode under code it is ldpc_sc_decode under fec = dict(code, window, t0, iters, alpha, test,
    fixed, outer; code and window required): max_iter, depth and quant are a ValueError there, as window, iters, test and fixed are with an
    LdpcCode.  fixed = dict(bits, ...), quant's format, is the window decoder's quant=: fixed point, vaeq_ldpc_sc_decode_q.  With a StaircaseCode
    under code it is staircase_decode, hard-decision FEC, under fec = dict(code, window, t0, iters; code and window required); every other key
    is a ValueError there, but for inner = dict(code=HammingCode or EbchCode, patterns=4, depth=None, payload=None, spread=True): the concatenated scheme,
    chase_decode on the LLRs behind t0 and the staircase code on its payload stream from 0 (as many chains as fit the C K stream bits).  The
    staircase's dict comes back with BER_pre the inner decoder's -- the channel's, what a sweep's BER_pre_fec column means -- and the inner
    decoder's dict under "inner".  With a ProductCode (of two HammingCodes or of two EbchCodes) under code it is tpc_decode, the soft-decision turbo
    product decoder, under fec = dict(code, t0, iters, patterns, alpha, beta, scale, clip; all but code optional); every other key is a
    ValueError there."""
    check_fec(fec)
    if isinstance(fec["code"], ProductCode):
        return tpc_decode(llr["llr"], llr["bits"], **{k: v for k, v in fec.items() if v is not None})
    if isinstance(fec["code"], StaircaseCode) and fec.get("inner") is not None:
        inner = resolve_inner(fec["inner"])
        first = chase_decode(llr["llr"], llr["bits"], inner["code"], t0=fec.get("t0", 0), depth=inner["depth"], patterns=inner["patterns"],
                             payload=inner["payload"], spread=inner["spread"], want_stream=True)
        stream = first.pop("stream")
        ret = staircase_decode(stream["llr"], stream["bits"], **{k: v for k, v in fec.items() if k not in ("inner", "t0")})
        ret["BER_pre"], ret["inner"] = first["BER_pre"], first
        return ret
    if isinstance(fec["code"], StaircaseCode):
        return staircase_decode(llr["llr"], llr["bits"], **{k: v for k, v in fec.items() if k != "inner"})
    kw = {"quant" if k == "fixed" else k: v for k, v in fec.items() if k != "code"}
    L, B = llr["llr"], llr["bits"]
    decode = ldpc_sc_decode if isinstance(fec["code"], ScLdpcCode) else ldpc_decode
    if fec.get("outer") is None or L.shape[0] == 0:
        return decode(L, B, fec["code"], **kw)
    R, N, n = L.shape[0], L.shape[-1], fec["code"].n
    w = L.numel() // max(R * N, 1)
    C_ = int(kw["codewords"]) if kw.get("codewords") is not None else _ldpc_fit(N, w, n, kw.get("t0", 0), kw.get("depth"))
    per_run = max(C_, 1) * n * (4 if kw.get("quant") is None else 2)
    step = max(1, int(OUTER_POST_BYTES) // per_run)
    return _cat_figures([decode(L[r:r + step], B[r:r + step], fec["code"], **kw) for r in range(0, R, step)])


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

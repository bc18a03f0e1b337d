"""torch.autograd.Function wrappers of the stand-alone operators (FIR + demapper, ELBO, VAE-NN encoder), forward AND backward on HIP kernels.

They make a reference-style training loop

    q, out = net(minibatch, amp_levels, var, nu_sc)                       # shared_funcs.twoXtwoFIR
    loss, var_est = loss_function_shaping(q, minibatch, h_est, amp_levels, P)
    loss.backward(); optimizer.step()                                     # func_VAELE_DP_MQAM_shaping.py:60-66

work on the GPU with torch.optim -- the differentiable form of the drop-in operator surface.  It is NOT how
the product trains (one fused kernel does forward, loss, backward and Adam: engine.DPEngine); it exists so that code written
against the reference's operators keeps working.  No CPU path: CPU tensors are refused by _native.ptr().

Every operator is differentiable in its parameters AND in its input signal, so a differentiable stage in front of the equalizer (an IQ
compensator, a pre-filter, another network) receives its gradient like behind the reference's torch modules:
    fir_demap, awgn_fir_demap   d/dW (vaeq_dp_forward_bwd, vaeq_awgn_forward_bwd)  and d/dx  (vaeq_dp_forward_bwd_x, vaeq_awgn_forward_bwd_x)
    elbo_loss, awgn_elbo_loss   d/dq, d/dh_est (vaeq_dp_loss_bwd, vaeq_awgn_loss_bwd)  and d/drx (vaeq_dp_loss_bwd_x, vaeq_awgn_loss_bwd_x)
    nn_encode                   d/dparams (vaeq_nn_enc_backward)                       and d/dx  (vaeq_nn_enc_backward_x, with d/dparams in the same pass)
A backward kernel is launched only for the gradients ctx.needs_input_grad asks for.  The backward passes are once_differentiable: a double
backward raises torch's error.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .engine import _f32, dp_forward, dp_loss, pad_to_symbols


class _FIRDemap(torch.autograd.Function):
    """twoXtwoFIR.forward (shared_funcs.py:500-527): (x[2,2,L], W[2,4,M]) -> (q[2,2n,B], out[2,2,B])."""

    @staticmethod
    def forward(ctx, x, W, amp, var, nu_sc, sps):
        q, y = dp_forward(x, W, amp, var, nu_sc, sps)
        ctx.save_for_backward(x, W, q, y, amp, var)
        ctx.sps, ctx.M = sps, W.shape[-1]
        return q, y

    @staticmethod
    @once_differentiable
    def backward(ctx, gq, gy):
        x, W, q, y, amp, var = ctx.saved_tensors
        gq = gq.contiguous()
        gy = gy.contiguous() if gy is not None else None
        gx = _fir_bwd_x(x, W, q, y, gq, gy, amp, var, ctx.sps, ctx.M) if ctx.needs_input_grad[0] else None
        gW = _fir_bwd(x, q, y, gq, gy, amp, var, ctx.sps, ctx.M) if ctx.needs_input_grad[1] else None
        return gx, gW, None, None, None, None


def _fir_bwd(x, q, y, gq, gy, amp, var, sps, M):
    dev, N = x.device, q.shape[-1]
    n = amp.numel()
    gW = torch.empty(2, 4, M, dtype=torch.float32, device=dev)
    var2 = _f32(var, dev).reshape(1, 2).contiguous()
    x, q, y = x.contiguous(), q.contiguous(), y.contiguous()      # locals: every argument lives until the launch is queued
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_forward_bwd(1, N, sps, M, n, nat.ptr(x), nat.ptr(q), nat.ptr(y), nat.ptr(gq), nat.ptr(gy),
                                                nat.ptr(amp), nat.ptr(var2), nat.ptr(gW), nat.current_stream(dev)), "vaeq_dp_forward_bwd")
    return gW


def _fir_bwd_x(x, W, q, y, gq, gy, amp, var, sps, M):
    dev, N = x.device, q.shape[-1]
    gx = torch.empty(x.shape, dtype=torch.float32, device=dev)    # x holds whole symbols here (fir_demap pads inside the graph)
    var2 = _f32(var, dev).reshape(1, 2).contiguous()
    W, q, y = W.detach().to(torch.float32).contiguous(), q.contiguous(), y.contiguous()
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_dp_forward_bwd_x(1, N, sps, M, amp.numel(), nat.ptr(W), nat.ptr(q), nat.ptr(y), nat.ptr(gq), nat.ptr(gy),
                                                  nat.ptr(amp), nat.ptr(var2), nat.ptr(gx), nat.current_stream(dev)), "vaeq_dp_forward_bwd_x")
    return gx


def fir_demap(x, W, amp_levels, var, nu_sc, sps):
    """Differentiable twoXtwoFIR.forward: gradients flow to W and to x (the zero padding to whole symbols is part of the graph: the gradient
    of the padded tail is dropped by its slice)."""
    amp = _f32(amp_levels, x.device).reshape(-1)
    var_t = _f32(var, x.device).reshape(2)
    return _FIRDemap.apply(pad_to_symbols(x, sps).contiguous(), W, amp, var_t, float(nu_sc), int(sps))


class _Loss(torch.autograd.Function):
    """loss_function_shaping (shared_funcs.py:92-137): (q, h_est) -> (loss, var_est); var_est is detached like the reference (:137)."""

    @staticmethod
    def forward(ctx, q, rx, h, amp, P):
        loss, ve = dp_loss(q, rx, h, amp, P)
        ctx.save_for_backward(q, rx, h, amp, P)
        ctx.mark_non_differentiable(ve)
        return loss, ve

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_ve):
        q, rx, h, amp, P = ctx.saved_tensors
        dev, B = q.device, q.shape[-1]
        sps, M, n = rx.shape[-1] // B, h.shape[-1], amp.numel()
        up = g_loss.reshape(1).to(torch.float32).contiguous()
        qc, rxc, hc = q.contiguous(), rx.contiguous(), h.contiguous()   # locals: temporaries freed before the launch could alias
        gq = gh = grx = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
                # the kernel writes row-major: allocate contiguous (empty_like would keep a permuted q's strides) and return in q's / h's shape
                gq = torch.empty(q.shape, dtype=torch.float32, device=dev)
                gh = torch.empty(h.shape, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_dp_loss_bwd(1, B, sps, M, n, nat.ptr(qc), nat.ptr(rxc), nat.ptr(hc), nat.ptr(amp), nat.ptr(P),
                                                     nat.ptr(up), nat.ptr(gq), nat.ptr(gh), nat.current_stream(dev)), "vaeq_dp_loss_bwd")
            if ctx.needs_input_grad[1]:
                grx = torch.empty(rx.shape, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_dp_loss_bwd_x(1, B, sps, M, n, nat.ptr(qc), nat.ptr(rxc), nat.ptr(hc), nat.ptr(amp), nat.ptr(up),
                                                       nat.ptr(grx), nat.current_stream(dev)), "vaeq_dp_loss_bwd_x")
        return gq, grx, gh, None, None


def elbo_loss(q, rx, h_est, amp_levels, P):
    """Differentiable loss_function_shaping: gradients flow to q, h_est and rx."""
    dev = q.device
    amp = _f32(amp_levels, dev).reshape(-1)
    Pt = _f32(P, dev).reshape(1, -1).contiguous()
    return _Loss.apply(q, rx.contiguous(), h_est, amp, Pt)


# ------------------------------------------------------------------ the single-polarisation (AWGN) pair
class _AwgnFIRDemap(torch.autograd.Function):
    """twoFIR.forward (AWGN_channel/func_VAELE_MQAM_shaping.py:214-231): (x[2,L], W[1,2,M]) -> (q[2n,B], out[2,B])."""

    @staticmethod
    def forward(ctx, x, W, amp, amp_mean, var, sps):
        from .engine import AWGNEngine
        M = W.shape[-1]
        eng = AWGNEngine(1, M, amp, torch.full((amp.numel(),), 1.0 / amp.numel()), float(amp_mean), float(var), x.device, sps)
        eng.set_state(W.detach(), None)
        q, y = eng.forward(x.reshape(1, 2, -1))
        ctx.save_for_backward(x, W.detach().reshape(1, 2, M).contiguous(), amp, eng.amp_mean, eng.var)
        ctx.sps, ctx.wshape = sps, tuple(W.shape)
        return q[0], y[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gq, gy):
        x, W, amp, amp_mean, var = ctx.saved_tensors
        dev, N, M = x.device, gq.shape[-1], W.shape[-1]
        x, gq = x.contiguous(), gq.contiguous()
        gy = gy.contiguous() if gy is not None else None
        gx = gW = None
        with torch.cuda.device(dev):
            args = (1, N, ctx.sps, M, amp.numel(), nat.ptr(x), nat.ptr(W), nat.ptr(amp), nat.ptr(amp_mean), nat.ptr(var), nat.ptr(gq), nat.ptr(gy))
            if ctx.needs_input_grad[0]:
                gx = torch.empty(x.shape, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_awgn_forward_bwd_x(*args, nat.ptr(gx), nat.current_stream(dev)), "vaeq_awgn_forward_bwd_x")
            if ctx.needs_input_grad[1]:
                gW = torch.empty(1, 2, M, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_awgn_forward_bwd(*args, nat.ptr(gW), nat.current_stream(dev)), "vaeq_awgn_forward_bwd")
                gW = gW.reshape(ctx.wshape)
        return gx, gW, None, None, None, None


def awgn_fir_demap(x, W, amp_levels, amp_mean, var, sps):
    """Differentiable twoFIR.forward: gradients flow to W and to x (the padding to whole symbols stays inside the graph)."""
    return _AwgnFIRDemap.apply(pad_to_symbols(x, sps).contiguous(), W, _f32(amp_levels, x.device).reshape(-1), float(amp_mean), float(var),
                               int(sps))


class _AwgnLoss(torch.autograd.Function):
    """loss_function of the AWGN modules (func_VAELE_MQAM_shaping.py:63-95 with the prior P, func_VAENN_MQAM.py:63-95 without):
    (q[2n,B], h[2,M]) -> loss."""

    @staticmethod
    def forward(ctx, q, rx, h, amp, P):
        from .engine import awgn_loss
        ctx.save_for_backward(q.detach(), rx, h.detach(), amp, P if P is not None else torch.empty(0, device=q.device))
        ctx.has_P = P is not None
        return awgn_loss(q.detach(), rx, h.detach(), amp, P)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, rx, h, amp, P = ctx.saved_tensors
        dev, B, M, n = q.device, q.shape[-1], h.shape[-1], amp.numel()
        sps = rx.shape[-1] // B
        Pt = P.reshape(1, n).contiguous() if ctx.has_P else None
        up = g.reshape(1).to(torch.float32).contiguous()
        qc, rxc, hc = q.contiguous(), rx.contiguous(), h.contiguous()   # locals: temporaries freed before the launch could alias
        gq = gh = grx = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
                gq = torch.empty(1, 2 * n, B, dtype=torch.float32, device=dev)
                gh = torch.empty(1, 2, M, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_awgn_loss_bwd(1, B, sps, M, n, nat.ptr(qc), nat.ptr(rxc), nat.ptr(hc), nat.ptr(amp),
                                                       nat.ptr(Pt), nat.ptr(up), nat.ptr(gq), nat.ptr(gh), nat.current_stream(dev)),
                          "vaeq_awgn_loss_bwd")
                gq, gh = gq[0], gh[0]
            if ctx.needs_input_grad[1]:
                grx = torch.empty(rx.shape, dtype=torch.float32, device=dev)
                nat.check(nat.lib().vaeq_awgn_loss_bwd_x(1, B, sps, M, n, nat.ptr(qc), nat.ptr(rxc), nat.ptr(hc), nat.ptr(amp), nat.ptr(up),
                                                         nat.ptr(grx), nat.current_stream(dev)), "vaeq_awgn_loss_bwd_x")
        return gq, grx, gh, None, None


def awgn_elbo_loss(q, rx, h_est, amp_levels, P=None):
    """Differentiable AWGN loss_function: gradients flow to q, h_est and rx.  P None = the VAE-NN form (entropy instead of KL)."""
    dev = q.device
    Pt = None if P is None else _f32(P, dev).reshape(-1).contiguous()
    return _AwgnLoss.apply(q, rx.contiguous().float(), h_est, _f32(amp_levels, dev).reshape(-1).contiguous(), Pt)


# ------------------------------------------------------------------ the VAE-NN encoder (func_VAENN_MQAM.Net / Net_BN)
def _enc_check(code, what):
    if int(code) == -3:
        raise nat.VaeqError(f"{what} failed: VAEQ_ERR_LDS: {nat.lib().vaeq_strerror(-3).decode()} -- the training-mode Net_BN forward and "
                            "the backward pass keep the whole input in LDS (vaeq_nn_enc_lds_bytes); shorten the minibatch (code -3)")
    nat.check(code, what)


def _enc_dims(params, sps, batch_norm):
    if len(params) != (6 if batch_norm else 4):
        raise ValueError(f"expected {'6 (fc1, fc2, batch1)' if batch_norm else '4 (fc1, fc2)'} parameter tensors, got {len(params)}")
    w1, w2 = params[0], params[2]
    C_ = w2.shape[0]
    if w1.dim() != 3 or w2.dim() != 3 or tuple(w1.shape[:2]) != (C_, 2) or w2.shape[1] != C_ or C_ % 2:
        raise ValueError(f"fc1.weight must be [C, 2, k1] and fc2.weight [C, C, k2], got {tuple(w1.shape)} and {tuple(w2.shape)}")
    return int(sps), C_ // 2, int(w1.shape[-1]), int(w2.shape[-1])


def _enc_forward(x, theta, dims, batch_norm, training, bn):
    """x[R,2,L] contiguous f32, theta[R,NP] -> (q[R,2n,N], saved statistics or None); bn[R,2C] is updated in place in training mode."""
    sps, n, k1, k2 = dims
    px, dev, (R, _, L) = nat.ptr(x), x.device, x.shape         # (a CPU tensor is refused here, before anything is allocated)
    q = torch.empty(R, 2 * n, -(-L // sps), dtype=torch.float32, device=dev)
    saved = torch.empty(R, 4 * n, dtype=torch.float32, device=dev) if batch_norm and training else None
    with torch.cuda.device(dev):
        _enc_check(nat.lib().vaeq_nn_enc_forward(R, L, sps, n, k1, k2, int(batch_norm), int(training), px, nat.ptr(theta), nat.ptr(bn),
                                                 nat.ptr(saved), nat.ptr(q), nat.current_stream(dev)), "vaeq_nn_enc_forward")
    return q, saved


LAST_BACKWARD_KERNEL = None     # instantiation the latest encoder backward launched: autograd runs backward on a thread of its own, and
                                # vaeq_last_kernel answers per calling thread


def _enc_backward(x, theta, q, gq, stats, dims, batch_norm, training, gx=None):
    """-> dL/dtheta_net[R,NP].  gx[R,2,L] given: vaeq_nn_enc_backward_x fills it with dL/dx in the same pass."""
    global LAST_BACKWARD_KERNEL
    sps, n, k1, k2 = dims
    dev, (R, _, L) = x.device, x.shape
    g = torch.empty_like(theta)
    with torch.cuda.device(dev):
        args = (R, L, sps, n, k1, k2, int(batch_norm), int(training), nat.ptr(x), nat.ptr(theta), nat.ptr(q), nat.ptr(gq), nat.ptr(stats), nat.ptr(g))
        if gx is not None:
            _enc_check(nat.lib().vaeq_nn_enc_backward_x(*args, nat.ptr(gx), nat.current_stream(dev)), "vaeq_nn_enc_backward_x")
        else:
            _enc_check(nat.lib().vaeq_nn_enc_backward(*args, nat.current_stream(dev)), "vaeq_nn_enc_backward")
    LAST_BACKWARD_KERNEL = nat.last_kernel()
    return g


class _NNEncode(torch.autograd.Function):
    """Net.forward / Net_BN.forward (func_VAENN_MQAM.py:178-188, :200-211): (x[1,2,L], the network's parameters) -> q[1,2n,N].  The saved state
    is x, a flat COPY of the parameters, q and the 2 C BatchNorm statistics: ELU(fc1(x)) is recomputed by the backward kernel."""

    @staticmethod
    def forward(ctx, x, dims, batch_norm, training, bn, *params):
        theta = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).reshape(1, -1).contiguous()
        q, saved = _enc_forward(x, theta, dims, batch_norm, training, bn)
        stats = saved if batch_norm and training else (bn.clone() if batch_norm else None)
        ctx.save_for_backward(x, theta, q, stats)
        ctx.dims, ctx.batch_norm, ctx.training, ctx.shapes = dims, batch_norm, training, [tuple(p.shape) for p in params]
        return q

    @staticmethod
    @once_differentiable
    def backward(ctx, gq):
        x, theta, q, stats = ctx.saved_tensors
        gq = gq.to(torch.float32).contiguous()                  # a local: lives until the launch is queued
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
        g = _enc_backward(x, theta, q, gq, stats, ctx.dims, ctx.batch_norm, ctx.training, gx)
        parts = torch.split(g[0], [int(torch.Size(s).numel()) for s in ctx.shapes])
        grads = tuple(p.reshape(s) if need else None for p, s, need in zip(parts, ctx.shapes, ctx.needs_input_grad[5:]))
        return (gx, None, None, None, None) + grads


def nn_encode(x, params, sps, batch_norm=False, training=False, running_mean=None, running_var=None):
    """Differentiable VAE-NN encoder: x[1,2,L] (or [2,L]) -> q[1,2n,ceil(L/sps)] (or [2n,N]); gradients flow to ``params`` =
    (fc1.weight, fc1.bias, fc2.weight, fc2.bias[, batch1.weight, batch1.bias]) and, when it requires one, to x.  batch_norm + training: batch statistics, and
    running_mean / running_var (when given) move in place by momentum 0.1; batch_norm without training: they normalise.
    With autograd off, or neither x nor a parameter requiring a gradient, this is a plain kernel call."""
    params = tuple(params)
    dims = _enc_dims(params, sps, batch_norm)
    if x.dim() not in (2, 3) or x.shape[-2] != 2 or (x.dim() == 3 and x.shape[0] != 1) or x.shape[-1] < 1:
        raise ValueError(f"x must be [1, 2, L] or [2, L], got {tuple(x.shape)}")
    if not x.is_cuda:
        nat.ptr(x)                                              # raises: the kernels take device tensors (no CPU path)
    graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    xc = (x if graph and x.requires_grad else x.detach()).to(torch.float32).reshape(1, 2, -1).contiguous()
    bn = None
    if batch_norm:
        if (running_mean is None or running_var is None) and not training:
            raise ValueError("eval-mode BatchNorm needs running_mean and running_var")
        if running_mean is not None and running_var is not None:
            bn = torch.cat([running_mean.detach().reshape(-1), running_var.detach().reshape(-1)]).to(torch.float32).reshape(1, -1).contiguous()
    if graph:
        q = _NNEncode.apply(xc, dims, bool(batch_norm), bool(training), bn, *params)
    else:
        theta = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).reshape(1, -1).contiguous()
        q = _enc_forward(xc, theta, dims, bool(batch_norm), bool(training), bn)[0]
    if batch_norm and training and bn is not None:
        C_ = 2 * dims[1]
        with torch.no_grad():
            running_mean.copy_(bn[0, :C_])
            running_var.copy_(bn[0, C_:])
    return q if x.dim() == 3 else q[0]

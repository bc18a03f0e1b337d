"""Float64 restatement of the drop-in operators, written from the math for the tests (not imported by the package).

Every function takes and returns torch tensors and is differentiable, so torch.autograd on the CPU supplies the gradients the HIP
backward kernels are checked against, including vector-Jacobian products for arbitrary upstream gradients.  Citations are to the
reference scripts the package mirrors (optical_DP_channel/shared_funcs.py, AWGN_channel/func_VAELE_MQAM_shaping.py,
AWGN_channel/func_VAENN_MQAM.py).

Conventions shared with the kernels and the C oracle:
  - the FIRs are Conv1d cross-correlations with padding M // 2 and stride sps, so L samples give ceil(L / sps) outputs;
  - the loss windows run over samples [mh, L - mh) and, for the KL / entropy term, over SYMBOLS [mh, B - mh) with the sample-domain
    mh = M // 2.  The reference writes these as ``[mh:-mh]``, which is empty at M = 1; here (as in the kernels) M = 1 takes the
    whole window.
"""
import torch
import torch.nn.functional as F


def _taps_window(s, M):
    """s[..., L] -> w[..., L - M + 1, M] with w[..., t, j] = s[..., t + (M - 1) - j]: the samples tap j of the channel FIR sees
    at output t + M - 1 (the ``idx - j`` of shared_funcs.py:119-125 / func_VAELE_MQAM_shaping.py:84-87)."""
    return s.unfold(-1, M, 1).flip(-1)


def _moments(q, amp):
    """q[..., 2n, B] -> (E_q[x], E_q[x^2]) per axis, [..., 2, B] (shared_funcs.py:107-111, func_VAELE_MQAM_shaping.py:75-79)."""
    n = amp.numel()
    qq = q.reshape(*q.shape[:-2], 2, n, q.shape[-1])
    a = amp.reshape(n, 1)
    return (qq * a).sum(-2), (qq * a * a).sum(-2)


def _upsample(s, sps):
    """s[..., B] -> [..., B * sps] with s on every sps-th sample and zeros between (the ``[..., ::sps]`` of :110-111)."""
    u = s.new_zeros(*s.shape, sps)
    u[..., 0] = s
    return u.reshape(*s.shape[:-1], s.shape[-1] * sps)


def _kl(q, P, mh):
    """sum over symbols [mh, B - mh) of q log(q / P + 1e-12) (shared_funcs.py:130-131); P None: q log(q + 1e-12)
    (func_VAENN_MQAM.py:90)."""
    B, n2 = q.shape[-1], q.shape[-2]
    qs = q[..., mh:B - mh]
    if P is None:
        return (qs * torch.log(qs + 1e-12)).sum()
    Pm = P.reshape(-1).repeat(n2 // P.numel()).reshape(n2, 1)
    return (qs * torch.log(qs / Pm + 1e-12)).sum()


# ------------------------------------------------------------------ dual polarisation
def dp_fir(x, W, sps):
    """Butterfly FIR of twoXtwoFIR.forward (shared_funcs.py:500-516): x[2,2,L], W[2,4,M] -> out[2 pol, 2 (I,Q), ceil(L/sps)].
    Input channels of the I conv are (x_I0, x_I1, -x_Q0, -x_Q1), of the Q conv (x_Q0, x_Q1, x_I0, x_I1)."""
    M = W.shape[-1]
    xin_i = torch.stack([x[0, 0], x[1, 0], -x[0, 1], -x[1, 1]])
    xin_q = torch.stack([x[0, 1], x[1, 1], x[0, 0], x[1, 0]])
    y_i = F.conv1d(xin_i[None], W, padding=M // 2, stride=sps)[0]
    y_q = F.conv1d(xin_q[None], W, padding=M // 2, stride=sps)[0]
    return torch.stack([y_i, y_q], 1)


def soft_dec(out, var, amp, nu_sc):
    """soft_dec (shared_funcs.py:529-542): out[2,2,N] -> q[2,2n,N]; q[p, c*n + i] = softmin_i((y - a_i)^2 / (2 var_p) + nu a_i^2)."""
    n, N = amp.numel(), out.shape[-1]
    d = out[:, :, None, :] - amp.reshape(1, 1, n, 1)
    z = d * d / (2 * var.reshape(2, 1, 1, 1)) + nu_sc * amp.reshape(1, 1, n, 1) ** 2
    return torch.softmax(-z, dim=2).reshape(2, 2 * n, N)


def dp_forward(x, W, amp, var, nu_sc, sps):
    """twoXtwoFIR.forward (shared_funcs.py:500-527) -> (q[2,2n,N], out[2,2,N])."""
    out = dp_fir(x, W, sps)
    return soft_dec(out, var, amp, nu_sc), out


def dp_loss(q, rx, h, amp, P):
    """loss_function_shaping (shared_funcs.py:92-137): q[2,2n,B], rx[2,2,B*sps], h[2 chi,2 nu,2 (re,im),M] -> (loss, var_est[2]).

    C_chi = |rx_chi - D_chi|^2 + sum_j |h_chi,nu,j|^2 Var_nu (windows of :115-127), loss = nm sum_chi log C_chi + sum q log(q/P + 1e-12),
    var_est = C / nm detached (:137)."""
    B, L, M = q.shape[-1], rx.shape[-1], h.shape[-1]
    sps = L // B
    assert L == B * sps, "rx must hold B * sps samples"
    mh = M // 2
    nm = L - 2 * mh
    mu, rho = _moments(q, amp)                                  # [nu, c, B]
    Eq, Var = _upsample(mu, sps), _upsample(rho - mu * mu, sps)  # [nu, c, L]
    w = _taps_window(Eq, M)                                     # [nu, c, nm, M]
    hr, hi = h[:, :, 0], h[:, :, 1]                             # [chi, nu, M]
    Dr = torch.einsum("xvj,vtj->xt", hr, w[:, 0]) - torch.einsum("xvj,vtj->xt", hi, w[:, 1])
    Di = torch.einsum("xvj,vtj->xt", hi, w[:, 0]) + torch.einsum("xvj,vtj->xt", hr, w[:, 1])
    VS = _taps_window(Var, M).sum(dim=(1, 2))                   # [nu, M]
    E = torch.einsum("xvj,vj->x", hr * hr + hi * hi, VS)
    r = rx[:, :, mh:L - mh]
    C = ((r[:, 0] - Dr) ** 2 + (r[:, 1] - Di) ** 2).sum(-1) + E
    loss = nm * torch.log(C).sum() + _kl(q, P, mh)
    return loss, (C / nm).detach()


# ------------------------------------------------------------------ single polarisation (AWGN / ISI)
def awgn_fir(x, W, sps):
    """The FIR of twoFIR.forward (func_VAELE_MQAM_shaping.py:214-223): x[2,L], W[1,2,M] -> out[2,ceil(L/sps)] (un-normalised);
    the I conv sees (x_I, x_Q), the Q conv (x_Q, -x_I)."""
    M = W.shape[-1]
    y_i = F.conv1d(x[None], W, padding=M // 2, stride=sps)[0, 0]
    y_q = F.conv1d(torch.stack([x[1], -x[0]])[None], W, padding=M // 2, stride=sps)[0, 0]
    return torch.stack([y_i, y_q])


def awgn_forward(x, W, amp, amp_mean, var, sps):
    """twoFIR.forward (func_VAELE_MQAM_shaping.py:214-231) -> (q[2n,N], out[2,N]): each axis scaled to mean |y| = amp_mean (:228),
    then q = softmin_i((y_hat - a_i)^2 / var) (:229)."""
    out = awgn_fir(x, W, sps)
    yh = out / out.abs().mean(-1, keepdim=True) * amp_mean
    n, N = amp.numel(), out.shape[-1]
    d = yh[:, None, :] - amp.reshape(1, n, 1)
    return torch.softmax(-(d * d) / var, dim=1).reshape(2 * n, N), out


def awgn_loss(q, rx, h, amp, P=None):
    """loss_function of func_VAELE_MQAM_shaping.py:63-95 (prior P) or, with P None, of func_VAENN_MQAM.py:63-95 (entropy):
    q[2n,B], rx[2,B*sps], h[2 (re,im),M] -> loss."""
    B, L, M = q.shape[-1], rx.shape[-1], h.shape[-1]
    sps = L // B
    assert L == B * sps, "rx must hold B * sps samples"
    mh = M // 2
    mu, rho = _moments(q, amp)                                  # [c, B]
    Eq, Var = _upsample(mu, sps), _upsample(rho - mu * mu, sps)
    w = _taps_window(Eq, M)                                     # [c, nm, M]
    Dr = w[0] @ h[0] - w[1] @ h[1]
    Di = w[1] @ h[0] + w[0] @ h[1]
    E = (_taps_window(Var, M).sum(0) @ (h[0] ** 2 + h[1] ** 2)).sum()
    r = rx[:, mh:L - mh]
    C = ((r[0] - Dr) ** 2 + (r[1] - Di) ** 2).sum() + E
    return (L - 2 * mh) * torch.log(C) + _kl(q, P, mh)


# ------------------------------------------------------------------ the VAE-NN encoder, for composed gradients
def vaenn_net(x, theta, n, k1, k2, sps, M):
    """Net.forward of func_VAENN_MQAM.py (Conv1d(2, 2n, k1) -> ELU -> Conv1d(2n, 2n, k2, stride sps) -> softmax per axis) on the flat
    parameter vector [fc1.weight | fc1.bias | fc2.weight | fc2.bias | h_est] -> (q[2n,B], h[2,M])."""
    C_ = 2 * n
    sizes = [C_ * 2 * k1, C_, C_ * C_ * k2, C_, 2 * M]
    w1, b1, w2, b2, h = torch.split(theta, sizes)
    a1 = F.elu(F.conv1d(x[None], w1.reshape(C_, 2, k1), b1, padding=k1 // 2))
    a2 = F.conv1d(a1, w2.reshape(C_, C_, k2), b2, padding=k2 // 2, stride=sps)[0]
    return torch.cat([torch.softmax(a2[:n], 0), torch.softmax(a2[n:], 0)]), h.reshape(2, M)

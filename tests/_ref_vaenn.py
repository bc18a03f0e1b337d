"""Float64 restatement of the AWGN VAE-NN equalizer (AWGN_channel/func_VAENN_MQAM.py), written from the math for the tests (not imported
by the package): the `Net` / `Net_BN` encoders in training and eval mode, the ELBO, torch.autograd gradients, the AMSGrad step, the
multi-step training loop of the kernels and the validation pass (find_shift, SER_q).

Parameters are the flat vector in NNEngine.offsets() order:
    Net:    [fc1.weight | fc1.bias | fc2.weight | fc2.bias | h_est]
    Net_BN: [fc1.weight | fc1.bias | fc2.weight | fc2.bias | batch1.weight | batch1.bias | h_est]
and the BatchNorm running statistics as bn = [running_mean | running_var] (2 C values, C = 2 n).
"""
import numpy as np
import torch
import torch.nn.functional as F

from _ref_operators import awgn_loss, vaenn_net

BN_EPS, BN_MOMENTUM = 1e-5, 0.1                          # nn.BatchNorm1d defaults (func_VAENN_MQAM.py:196)
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8                # optim.Adam defaults (:256)


def _t(a):
    return a.detach().to(torch.float64) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def sizes(n, k1, k2, M, batch_norm):
    C_ = 2 * n
    s = [C_ * 2 * k1, C_, C_ * C_ * k2, C_]
    return s + ([C_, C_] if batch_norm else []) + [2 * M]


def offsets(n, k1, k2, M, batch_norm):
    return [int(v) for v in np.cumsum([0] + sizes(n, k1, k2, M, batch_norm))]


def forward(x, theta, n, k1, k2, sps, M, batch_norm=False, bn=None, train=True):
    """Net.forward (:178-189) / Net_BN.forward (:200-211) on x[2, L] -> (q[2n, ceil(L / sps)], h[2, M], bn after the step or None).

    The reference adds x_res (the mean of the sps samples of a symbol, :183-185 / :205-207) to every logit of an axis before the softmax:
    a constant across the levels of that axis, so it cancels in the softmax and is left out here (the kernels leave it out too).
    Net_BN in training mode normalises with the batch statistics over the L samples (biased variance) and moves the running statistics
    by momentum 0.1 with the unbiased variance; in eval mode (net.eval(), :283) it normalises with the running statistics."""
    x, theta = _t(x), theta if torch.is_tensor(theta) else _t(theta)
    if not batch_norm:
        q, h = vaenn_net(x, theta, n, k1, k2, sps, M)
        return q, h, None
    C_ = 2 * n
    w1, b1, w2, b2, ga, be, h = torch.split(theta, sizes(n, k1, k2, M, True))
    z = F.elu(F.conv1d(x[None], w1.reshape(C_, 2, k1), b1, padding=k1 // 2))[0]           # (:201) ELU(fc1(x)), [C, L]
    bn = _t(bn)
    rm, rv = bn[:C_], bn[C_:]
    if train:
        L = z.shape[-1]
        mean = z.mean(-1)
        var = ((z - mean[:, None]) ** 2).mean(-1)
        zh = (z - mean[:, None]) / torch.sqrt(var[:, None] + BN_EPS)
        d = var.detach() * L / (L - 1)
        bn_new = torch.cat([(1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean.detach(), (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * d])
    else:
        zh = (z - rm[:, None]) / torch.sqrt(rv[:, None] + BN_EPS)
        bn_new = None
    zb = ga[:, None] * zh + be[:, None]                                                     # batch1 (:196, :201)
    a2 = F.conv1d(zb[None], w2.reshape(C_, C_, k2), b2, padding=k2 // 2, stride=sps)[0]      # fc2 (:195)
    q = torch.cat([torch.softmax(a2[:n], 0), torch.softmax(a2[n:], 0)])                     # softmax per axis (:208-210)
    return q, h.reshape(2, M), bn_new


def step_grads(x, theta, amp, n, k1, k2, M, sps, batch_norm=False, bn=None):
    """One teacher-forced step (:272-279): q, loss_function (:60-91, the entropy form of _ref_operators.awgn_loss) and its gradient
    with respect to every parameter by torch.autograd -> dict(q, loss, g, bn) in float64 numpy."""
    th = _t(theta).clone().requires_grad_(True)
    x = _t(x)
    q, h, bn_new = forward(x, th, n, k1, k2, sps, M, batch_norm, bn, train=True)
    loss = awgn_loss(q, x, h, _t(amp), None)
    loss.backward()
    return dict(q=q.detach().numpy(), loss=float(loss.detach()), g=th.grad.numpy().copy(), bn=None if bn_new is None else bn_new.numpy())


class State:
    """theta and its AMSGrad state (m, v, vmax, step) plus the BatchNorm running statistics, float64."""

    def __init__(self, theta, n=None, batch_norm=False, bn=None):
        self.theta = np.array(theta, np.float64).reshape(-1)
        self.m, self.v, self.vmax = (np.zeros_like(self.theta) for _ in range(3))
        self.step = 0
        self.bn = None
        if batch_norm:
            self.bn = np.array(bn, np.float64) if bn is not None else np.concatenate([np.zeros(2 * n), np.ones(2 * n)])


def amsgrad_step(st, g, lr):
    """optim.Adam(amsgrad=True).step() (:256, :280), written out so that m, v and vmax can be compared:
    m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, vmax = max(vmax, v), theta -= lr / (1 - b1^t) m / (sqrt(vmax / (1 - b2^t)) + eps)."""
    st.step += 1
    st.m = BETA1 * st.m + (1 - BETA1) * g
    st.v = BETA2 * st.v + (1 - BETA2) * g * g
    st.vmax = np.maximum(st.vmax, st.v)
    bc1, bc2 = 1 - BETA1 ** st.step, 1 - BETA2 ** st.step
    st.theta = st.theta - lr / bc1 * st.m / (np.sqrt(st.vmax) / np.sqrt(bc2) + ADAM_EPS)


def train(st, rx, steps, B, amp, n, k1, k2, M, sps, lr, batch_norm=False, no_update=False):
    """The training loop (:271-280) as vaeq_nn_train runs it: minibatch s is rx[:, s B sps : (s + 1) B sps] (:273), the running statistics
    carry from step to step.  Updates st in place (unless no_update) and returns (losses[steps], last step's gradient, q[2n, steps B]);
    st.grads keeps the gradient of every step."""
    rx = np.asarray(rx, np.float64)
    L = B * sps
    losses, qs, gs, g = [], [], [], None
    for s in range(steps):
        r = step_grads(rx[:, s * L:(s + 1) * L], st.theta, amp, n, k1, k2, M, sps, batch_norm, st.bn)
        losses.append(r["loss"])
        qs.append(r["q"])
        g = r["g"]
        gs.append(g)
        if not no_update:
            if batch_norm:
                st.bn = r["bn"]
            amsgrad_step(st, g, lr)
    st.grads = gs
    return np.array(losses), g, np.concatenate(qs, 1)


def eval_forward(x, theta, n, k1, k2, sps, M, batch_norm=False, bn=None):
    """The validation forward pass (:287-288) over a whole block x[2, N sps]: zero padding only at the block's two ends, eval-mode
    BatchNorm -> q[2n, N] float64 numpy."""
    return forward(x, _t(theta), n, k1, k2, sps, M, batch_norm, bn, train=False)[0].numpy()


def find_shift(q, tx, n_shift, amp, n):
    """find_shift (:152-168) on q[2n, N], tx[2, N] -> (shift, corr_I, corr_Q) in float64."""
    amp = np.asarray(amp, np.float64)
    E = amp @ q[:n, :1000]
    half = n_shift // 2
    Em = np.stack([np.roll(E, i - half) for i in range(n_shift)], 1)
    tI, tQ = np.asarray(tx[0, :1000], np.float64), np.asarray(tx[1, :1000], np.float64)
    cI, cQ = np.abs(tI @ Em), np.abs(tQ @ Em)
    if cI.max() >= 0.02 * q.shape[-1]:
        return half - int(np.argmax(cI)), cI, cQ
    if cQ.max() >= cI.max():
        return half - int(np.argmax(cQ)), cI, cQ
    return half - int(np.argmax(cI)), cI, cQ


def decisions(q, n):
    """argmax per axis (:102) -> dec[2, N] and the decision margin (largest minus second largest q of either axis)."""
    dec = np.stack([q[:n].argmax(0), q[n:].argmax(0)])
    srt = [np.sort(q[:n], 0), np.sort(q[n:], 0)]
    margin = np.minimum(srt[0][-1] - srt[0][-2], srt[1][-1] - srt[1][-2])
    return dec, margin


def ser_q(q, tx, n):
    """SER_q (:93-119): hard decisions of q against the levels of tx, the minimum over the four quadrant rotations."""
    N = tx.shape[-1]
    if N == 0 or q.shape[-1] < N:                        # an empty window: torch.mean over no symbols is NaN
        return float("nan")
    scale = (n - 1) / 2
    data = np.round(scale * np.asarray(tx, np.float64) + scale)
    dec = decisions(q[:, :N], n)[0].astype(np.float64)
    dpi = -(dec - 2 * scale)
    dpi4 = np.stack([-(dec[1] - 2 * scale), dec[0]])
    d3 = -(dpi4 - 2 * scale)
    return min(float(np.mean((data != d).any(0))) for d in (dec, dpi, dpi4, d3))


def validate(q, tx, n_shift, amp, n):
    """The validation pass (:292-293): shift = find_shift(q, tx, n_shift), SER = SER_q(q[:, 11 + shift : -11], tx[:, 11 : -11 - shift]),
    sliced as Python slices them: from shift = -11 down the TX window is empty and the SER is NaN."""
    sh = find_shift(q, tx, n_shift, amp, n)[0]
    return sh, ser_q(q[:, 11 + sh:-11], tx[:, 11:-11 - sh], n)


def levels(n):
    """The amplitude levels of n^2-QAM at unit average power (:226-239)."""
    lev = np.arange(-(n - 1), n, 2).astype(np.float64)
    return (lev / np.sqrt(np.mean(lev ** 2) * 2)).astype(np.float32)


def init_theta(rng, n, k1, k2, M, batch_norm, scale=1.0):
    """Random parameters near the reference's initialisation (:173-176, :194-198, :251-252), with h_est off the Dirac and gamma / beta
    off (1, 0) so that every term of the gradient is exercised.  float32."""
    C_ = 2 * n
    parts = [rng.uniform(-1, 1, C_ * 2 * k1) * np.sqrt(6.0 / (2 * k1 + C_ * k1)) * scale, rng.uniform(-1, 1, C_) / np.sqrt(2 * k1),
             rng.uniform(-1, 1, C_ * C_ * k2) * np.sqrt(6.0 / (2 * C_ * k2)), rng.uniform(-1, 1, C_) / np.sqrt(C_ * k2)]
    if batch_norm:
        parts += [1 + 0.2 * rng.standard_normal(C_), 0.1 * rng.standard_normal(C_)]
    h = 0.05 * rng.standard_normal((2, M))
    h[0, M // 2] += 1
    parts.append(h.reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def random_bn(rng, n):
    """Running statistics away from (0, 1)."""
    return np.concatenate([0.3 * rng.standard_normal(2 * n), rng.uniform(0.3, 2.0, 2 * n)]).astype(np.float32)

"""func_VAENN_MQAM.Net / Net_BN as torch modules on the HIP encoder kernels (vaeq_nn_enc_forward / vaeq_nn_enc_backward), against the float64
restatement of tests/_ref_vaenn.py and the goldens captured from the reference (G8: Net, G11: Net_BN).

Tolerances are the project's: against float64 an error may be FACTOR x the float32 baseline's own error against float64, with the floors of
test_vaenn_envelope_gpu.py (q 2e-5, loss 1e-5, gradients 5e-5 relative per tensor, running statistics 1e-5, free-step theta 2e-5, m / v / vmax
1e-4).  The float32 baseline is the C oracle where it has the quantity, and the same restatement in float32 torch on the CPU (_torch_case)
where it has not (an arbitrary upstream gradient).  Against the goldens: q 5e-6, loss 1e-5 relative, gradients 2e-4 relative per tensor,
theta 5e-6 on the entries whose gradient was not rounding-level.  Where two paths run the same kernel the comparison is bit for bit.
The largest error of each quantity and its ratio to the baseline's is printed at the end of the module (-s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import _ref_vaenn as ref
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = {}
SEEN = set()
FACTOR = 4.0
LDS_MAX = 160 * 1024


def _note(key, value):
    STATS[key] = max(STATS.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(STATS):
        print(f"  {k}: {STATS[k]:.3g}")


def _np(t):
    return t.detach().cpu().numpy()


def _last():
    from vae_equalizer_amd import _native as nat
    name = nat.last_kernel()
    SEEN.add(name)
    return name


def _check(tag, err, base, floor):
    _note(f"{tag} err", err)
    _note(f"{tag} err / f32-baseline err", err / max(base, 1e-30))
    _note(f"{tag} err / tolerance", err / max(FACTOR * base, floor))
    assert err <= max(FACTOR * base, floor), (tag, err, base)


def _names(bn):
    return ["w1", "b1", "w2", "b2"] + (["gamma", "beta"] if bn else [])


def _module(n, bn, k1, k2, sps, theta=None, bn0=None):
    """A module on the device, optionally loaded from a flat vector [network | h_est] -> (net, h_est or None)."""
    from vae_equalizer_amd.func_VAENN_MQAM import Net, Net_BN, theta_to_net
    net = (Net_BN if bn else Net)(k1, k2, n, sps).to(DEV)
    h = None
    if theta is not None:
        h = theta_to_net(torch.from_numpy(np.asarray(theta, np.float32)).to(DEV), net, None if bn0 is None else torch.from_numpy(np.asarray(bn0, np.float32)))
    return net, h


def _grads(net):
    return np.concatenate([_np(p.grad).reshape(-1) for p in net._params()])


def _torch_case(x, theta, gq, n, bn, k1, k2, sps, bn0, train, dtype):
    """The restatement of _ref_vaenn.forward in `dtype` torch on the CPU (its _t() casts to float64, so the float32 baseline restates it here):
    -> (q, gradient of sum(q gq) per network parameter, running statistics after the step)."""
    C_ = 2 * n
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    s = ref.sizes(n, k1, k2, 1, bn)[:-1]
    parts = torch.split(th[:sum(s)], s)
    z = F.elu(F.conv1d(xt[None], parts[0].reshape(C_, 2, k1), parts[1], padding=k1 // 2))[0]
    bn_new = None
    if bn:
        b0 = torch.tensor(np.asarray(bn0), dtype=dtype)
        rm, rv = b0[:C_], b0[C_:]
        if train:
            L = z.shape[-1]
            mean = z.mean(-1)
            var = ((z - mean[:, None]) ** 2).mean(-1)
            zh = (z - mean[:, None]) / torch.sqrt(var[:, None] + ref.BN_EPS)
            bn_new = torch.cat([0.9 * rm + 0.1 * mean.detach(), 0.9 * rv + 0.1 * var.detach() * L / (L - 1)]).numpy()
        else:
            zh = (z - rm[:, None]) / torch.sqrt(rv[:, None] + ref.BN_EPS)
        z = parts[4][:, None] * zh + parts[5][:, None]
    a2 = F.conv1d(z[None], parts[2].reshape(C_, C_, k2), parts[3], padding=k2 // 2, stride=sps)[0]
    q = torch.cat([torch.softmax(a2[:n], 0), torch.softmax(a2[n:], 0)])
    g = None
    if gq is not None:
        (q * torch.tensor(np.asarray(gq), dtype=dtype)).sum().backward()
        g = th.grad.numpy()[:sum(s)].astype(np.float64)
    return q.detach().numpy().astype(np.float64), g, bn_new


def _ref64(x, theta, gq, n, bn, k1, k2, sps, bn0, train):
    """tests/_ref_vaenn.forward in float64 with autograd for an arbitrary upstream gradient."""
    th = torch.tensor(np.asarray(theta, np.float64), requires_grad=True)
    q, _, bn_new = ref.forward(x, th, n, k1, k2, sps, 1, bn, bn0, train=train)
    g = None
    if gq is not None:
        (q * torch.from_numpy(np.asarray(gq, np.float64))).sum().backward()
        g = th.grad.numpy()[:-2]
    return q.detach().numpy(), g, None if bn_new is None else bn_new.numpy()


# n, bn, L, sps, k1, k2: every n_lev with and without BatchNorm, sps 1 / 2 / 3 / 8, k1 1 .. 63, k2 1 .. 9, L % sps != 0, L on both sides of 640
GRID = [
    (2, False, 37, 1, 1, 1), (2, True, 83, 2, 7, 5), (2, True, 640, 2, 3, 1), (2, False, 1001, 3, 63, 9), (2, True, 643, 8, 25, 9),
    (4, False, 121, 2, 11, 3), (4, True, 638, 3, 3, 9), (4, True, 645, 8, 63, 9), (4, False, 700, 1, 5, 5), (4, True, 2, 1, 1, 1),
    (8, False, 600, 2, 25, 3), (8, True, 600, 2, 25, 3), (8, True, 641, 2, 63, 1), (8, False, 803, 8, 5, 9), (8, True, 65, 3, 1, 3),
    (8, True, 690, 2, 9, 7), (8, False, 17, 3, 63, 9), (8, False, 333, 1, 3, 1),
]


def _case(n, bn, L, k1, k2, seed):
    rng = np.random.default_rng(seed)
    theta = ref.init_theta(rng, n, k1, k2, 1, bn)
    bn0 = ref.random_bn(rng, n) if bn else None
    x = (0.5 * rng.standard_normal((2, L))).astype(np.float32)
    N = lambda sps: -(-L // sps)
    return rng, theta, bn0, x, N


def _run(n, bn, L, sps, k1, k2, train, gq_kind="random", seed=None):
    rng, theta, bn0, x, N = _case(n, bn, L, k1, k2, seed or (L * 31 + sps * 7 + k1 * 3 + k2 + n + bn))
    if gq_kind == "onehot":                                    # saturated logits: q is one-hot to rounding
        o = ref.offsets(n, k1, k2, 1, bn)
        theta[o[3]:o[4]] = 0.0
        theta[o[3] + rng.integers(n)] = theta[o[3] + n + rng.integers(n)] = 60.0
    gq = rng.standard_normal((2 * n, N(sps))).astype(np.float32)
    if gq_kind == "zero_axis":
        gq[n:] = 0.0
    net, _ = _module(n, bn, k1, k2, sps, theta, bn0)
    net.train(train)
    q = net(torch.from_numpy(x).to(DEV)[None])
    fwd = _last()
    q.backward(torch.from_numpy(gq).to(DEV)[None])
    from vae_equalizer_amd import autograd_ops
    bwd = autograd_ops.LAST_BACKWARD_KERNEL                    # (autograd's backward thread made the launch: vaeq_last_kernel is per thread)
    SEEN.add(bwd)
    torch.cuda.synchronize()
    q64, g64, b64 = _ref64(x, theta, gq, n, bn, k1, k2, sps, bn0, train)
    q32, g32, b32 = _torch_case(x, theta, gq, n, bn, k1, k2, sps, bn0, train, torch.float32)
    mode = "train" if train else "eval"
    assert tuple(q.shape) == (1, 2 * n, N(sps)) and q.dtype == torch.float32
    _check(f"{mode} q", np.abs(_np(q)[0] - q64).max(), np.abs(q32 - q64).max(), 2e-5)
    if bn and train:
        got = np.concatenate([_np(net.batch1.running_mean), _np(net.batch1.running_var)])
        _check("running statistics", relerr(got, b64), relerr(b32, b64), 1e-5)
        assert int(net.batch1.num_batches_tracked) == 1
    elif bn:
        assert np.array_equal(np.concatenate([_np(net.batch1.running_mean), _np(net.batch1.running_var)]), bn0)
    g = _grads(net)
    o = ref.offsets(n, k1, k2, 1, bn)
    for nm, a, b in zip(_names(bn), o[:-1], o[1:]):
        if np.abs(g64[a:b]).max() == 0.0:
            assert np.abs(g[a:b]).max() == 0.0
            continue
        try:
            _check(f"{mode} grad {nm} ({gq_kind})", relerr(g[a:b], g64[a:b]), relerr(g32[a:b], g64[a:b]), 5e-5)
        except AssertionError:
            raise AssertionError(((n, bn, L, sps, k1, k2, mode, gq_kind), nm, relerr(g[a:b], g64[a:b]), relerr(g32[a:b], g64[a:b])))
    assert fwd == (f"vaeq::nn_enc_bn_forward_kernel<512, {n}>" if bn and train else f"vaeq::nn_enc_forward_kernel<1024, {n}>")
    assert bwd == f"vaeq::nn_enc_backward_kernel<512, {n}, {(1 if train else 2) if bn else 0}>"


@pytest.mark.parametrize("n,bn,L,sps,k1,k2", GRID)
def test_forward_and_backward_training_mode(n, bn, L, sps, k1, k2):
    """q, the running statistics after the forward, and the gradient of every parameter tensor for a RANDOM upstream gradient."""
    _run(n, bn, L, sps, k1, k2, True)


@pytest.mark.parametrize("n,bn,L,sps,k1,k2", [c for c in GRID if c[1] and c[2] > 2] + [GRID[0], GRID[5], GRID[10]])
def test_forward_and_backward_eval_mode(n, bn, L, sps, k1, k2):
    """net.eval(): the running statistics normalise (and stay as they are); backward is a per-channel scale through BatchNorm."""
    _run(n, bn, L, sps, k1, k2, False)


@pytest.mark.parametrize("kind", ["zero_axis", "onehot"])
@pytest.mark.parametrize("n,bn", [(2, True), (4, False), (8, True), (8, False)])
def test_backward_degenerate_upstream(n, bn, kind):
    """An upstream gradient that is zero on the quadrature axis; a one-hot q from saturated logits (softmax backward ~ 0)."""
    _run(n, bn, 301, 2, 9, 3, True, kind)


# ------------------------------------------------------------------ the reference's gradients and its loop (goldens)
def _golden_loop(name, bn):
    """The reference's loop (:271-280) on the captured minibatches; checks every captured quantity on the way."""
    from vae_equalizer_amd.func_VAENN_MQAM import loss_function, net_to_theta
    g = load_golden(name)
    B, sps, M, k1, k2, lr, ns = int(g["B"]), int(g["sps"]), int(g["M_est"]), int(g["k1"]), int(g["k2"]), float(g["lr"]), int(g["n_steps"])
    amp = torch.from_numpy(g["amp_levels"]).to(DEV)
    n = amp.numel()
    net, h0 = _module(n, bn, k1, k2, sps, g["theta0"], g["bn0"] if bn else None)
    h_est = h0.clone().requires_grad_(True)
    optimizer = torch.optim.Adam(net.parameters(), lr=lr, amsgrad=True)
    optimizer.add_param_group({"params": h_est})
    rx = torch.from_numpy(g["rx"]).to(DEV)
    minibatch = torch.empty(1, 2, B * sps, device=DEV, dtype=torch.float32)
    o = ref.offsets(n, k1, k2, M, bn)
    st = ref.State(g["theta0"], n, bn, g["bn0"] if bn else None)                 # float64 loop: only for the rounding-level mask
    ref.train(st, g["rx"], ns, B, g["amp_levels"], n, k1, k2, M, sps, lr, bn)
    net.train()
    for m in range(ns):
        optimizer.zero_grad()
        minibatch[0, :, :] = rx[:, m * B * sps:(m + 1) * B * sps]
        out = net(minibatch)
        loss = loss_function(out.squeeze(), minibatch.squeeze(), h_est, DEV, amp)
        loss.backward()
        if f"q{m}" in g:
            e = np.abs(_np(out)[0] - g[f"q{m}"]).max()
            _note("golden q err", e)
            assert e < 5e-6, (name, m, e)
        if f"g{m}" in g:
            got = np.concatenate([_grads(net), _np(h_est.grad).reshape(-1)])
            for a, b in zip(o[:-1], o[1:]):
                e = relerr(got[a:b], g[f"g{m}"][a:b])
                _note("golden grad err", e)
                assert e < 2e-4, (name, m, a, b, e)
        e = abs(float(loss.detach()) - g["loss"][m]) / abs(g["loss"][m])
        _note(f"golden loss err (step {m})", e)
        assert e < 1e-5, (name, m, e)
        optimizer.step()
        if bn and f"bn{m + 1}" in g:
            e = relerr(_np(net_to_theta(net, h_est)[1]), g[f"bn{m + 1}"])
            _note("golden bn err", e)
            assert e < 1e-5, (name, m, e)
        if f"theta{m + 1}" in g:
            bad = _capped_mask(st.grads[:m + 1], o)
            _cap(bad, o)
            th = _np(net_to_theta(net, h_est)[0])
            e = np.abs(th - g[f"theta{m + 1}"])[~bad].max()
            _note(f"golden theta{m + 1} err", e)
            assert e < 5e-6, (name, m + 1, e)
            assert np.abs(th - g[f"theta{m + 1}"]).max() <= 2.01 * (m + 1) * lr
    if "vmax" in g:
        vm = np.concatenate([_np(optimizer.state[p]["max_exp_avg_sq"]).reshape(-1) for p in list(net.parameters()) + [h_est]])
        e = relerr(vm, g["vmax"])
        _note("golden vmax err", e)
        assert e < 1e-4, (name, e)
    return g, net, h_est


def _capped_mask(grads, o):
    """The rounding-level mask of the envelope test (per tensor: |g| <= 1e-4 max |g| at some step) for captured data, whose seeds cannot be
    chosen: where it flags more entries of a tensor than the cap allows, only the entries with the SMALLEST relative gradient stay masked,
    up to the cap -- the others are checked like any entry (stricter than the plain mask, never weaker)."""
    bad = np.zeros(o[-1], bool)
    for a, b in zip(o[:-1], o[1:]):
        score = np.min([np.abs(g[a:b]) / np.abs(g[a:b]).max() for g in grads], 0)
        idx = np.flatnonzero(score <= 1e-4)
        keep = idx[np.argsort(score[idx])][:max(1, int(0.05 * (b - a)))]
        _note("golden mask entries unmasked by the cap", len(idx) - len(keep))
        bad[a + keep] = True
    return bad


def _cap(bad, o):
    """The rounding-level mask may hide at most 5 % of a parameter tensor or one entry, whichever is larger."""
    for a, b in zip(o[:-1], o[1:]):
        assert bad[a:b].sum() <= max(1, int(0.05 * (b - a))), (a, b, int(bad[a:b].sum()))


@pytest.mark.parametrize("name", ["G8_vaenn_64qam", "G8_vaenn_16qam_small", "G8_vaenn_4qam_k5"])
def test_reference_loop_net(name):
    _golden_loop(name, False)


@pytest.mark.parametrize("name", ["G11_vaennbn_64qam", "G11_vaennbn_16qam_small"])
def test_reference_loop_net_bn_and_eval(name):
    g, net, _ = _golden_loop(name, True)
    B, ns, sps = int(g["B"]), int(g["n_steps"]), int(g["sps"])
    from vae_equalizer_amd.func_VAENN_MQAM import theta_to_net
    theta_to_net(torch.from_numpy(g[f"theta{ns}"]).to(DEV), net, torch.from_numpy(g[f"bn{ns}"]))
    net.eval()
    with torch.no_grad():
        q = net(torch.from_numpy(g["rx"][None, :, :B * min(ns, 3) * sps]).to(DEV))
    assert np.abs(_np(q)[0] - g["q_eval"]).max() < 5e-6


@pytest.mark.parametrize("name", ["G11_vaennbn_64qam", "G11_vaennbn_16qam_small"])
def test_state_dict_interchange(name):
    """A state_dict under the reference's key names, built from the captured theta0 / bn0, loads strictly and reproduces the captured q0."""
    from vae_equalizer_amd.func_VAENN_MQAM import Net_BN
    g = load_golden(name)
    B, sps, M, k1, k2 = int(g["B"]), int(g["sps"]), int(g["M_est"]), int(g["k1"]), int(g["k2"])
    n = g["amp_levels"].size
    C_, o = 2 * n, ref.offsets(n, k1, k2, M, True)
    t = torch.from_numpy(g["theta0"])
    sd = {"fc1.weight": t[o[0]:o[1]].reshape(C_, 2, k1), "fc1.bias": t[o[1]:o[2]], "fc2.weight": t[o[2]:o[3]].reshape(C_, C_, k2),
          "fc2.bias": t[o[3]:o[4]], "batch1.weight": t[o[4]:o[5]], "batch1.bias": t[o[5]:o[6]],
          "batch1.running_mean": torch.from_numpy(g["bn0"][:C_]), "batch1.running_var": torch.from_numpy(g["bn0"][C_:]),
          "batch1.num_batches_tracked": torch.tensor(0)}
    net = Net_BN(k1, k2, n, sps).to(DEV)
    net.load_state_dict(sd, strict=True)
    net.train()
    with torch.no_grad():
        q = net(torch.from_numpy(g["rx"][None, :, :B * sps]).to(DEV))
    assert np.abs(_np(q)[0] - g["q0"]).max() < 5e-6
    assert relerr(np.concatenate([_np(net.batch1.running_mean), _np(net.batch1.running_var)]), g["bn1"]) < 1e-5
    assert int(net.state_dict()["batch1.num_batches_tracked"]) == 1


# ------------------------------------------------------------------ agreement with the fused kernel (both against the float64 loop)
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("n", [4, 8])
def test_module_loop_and_fused_kernel_agree_with_float64(n, bn):
    from vae_equalizer_amd.engine import NNEngine
    from vae_equalizer_amd.func_VAENN_MQAM import loss_function, net_to_theta
    B, sps, k1, k2, M, steps, lr = 300, 2, 25, 3, 25, 5, 1e-3
    rng = np.random.default_rng(7 + n + bn)
    theta = ref.init_theta(rng, n, k1, k2, M, bn)
    bn0 = ref.random_bn(rng, n) if bn else None
    x = (0.5 * rng.standard_normal((2, steps * B * sps))).astype(np.float32)
    amp, o = ref.levels(n), ref.offsets(n, k1, k2, M, bn)
    st = ref.State(theta, n, bn, bn0)
    l64, _, _ = ref.train(st, x, steps, B, amp, n, k1, k2, M, sps, lr, bn)
    if bn:
        so = oracle.NNBNState(theta, n, np.float32)
        so.bn = np.array(bn0, np.float32)
        l32 = oracle.nnbn_train(so, x, steps, B, amp, k1, k2, M, lr, sps, np.float32)
    else:
        so = oracle.NNState(theta, np.float32)
        l32 = oracle.nn_train(so, x, steps, B, amp, k1, k2, M, lr, sps, np.float32)
    bad = np.zeros(o[-1], bool)
    for gg in st.grads:
        for a, b in zip(o[:-1], o[1:]):
            bad[a:b] |= np.abs(gg[a:b]) <= 1e-4 * np.abs(gg[a:b]).max()
    _cap(bad, o)
    ok = ~bad
    # the fused kernel
    eng = NNEngine(1, M, k1, k2, amp, DEV, sps, batch_norm=bn)
    eng.theta.copy_(torch.from_numpy(theta)[None])
    if bn:
        eng.bn.copy_(torch.from_numpy(bn0)[None])
    r = eng.train(torch.from_numpy(x[None]).to(DEV), B, steps, lr)
    # the module loop
    net, h0 = _module(n, bn, k1, k2, sps, theta, bn0)
    h_est = h0.clone().requires_grad_(True)
    opt = torch.optim.Adam(net.parameters(), lr=lr, amsgrad=True)
    opt.add_param_group({"params": h_est})
    xt, ampt = torch.from_numpy(x).to(DEV), torch.from_numpy(amp).to(DEV)
    losses = []
    net.train()
    for m in range(steps):
        opt.zero_grad()
        mb = xt[None, :, m * B * sps:(m + 1) * B * sps]
        loss = loss_function(net(mb).squeeze(), mb.squeeze(), h_est, DEV, ampt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    ps = list(net.parameters()) + [h_est]
    cat = lambda key: np.concatenate([_np(opt.state[p][key]).reshape(-1) for p in ps])
    mod = dict(theta=_np(net_to_theta(net, h_est)[0]), m=cat("exp_avg"), v=cat("exp_avg_sq"), vmax=cat("max_exp_avg_sq"), loss=np.array(losses),
               bn=_np(net_to_theta(net, h_est)[1]) if bn else None)
    fus = dict(theta=_np(eng.theta)[0], m=_np(eng.m)[0], v=_np(eng.v)[0], vmax=_np(eng.vmax)[0], loss=_np(r["loss"])[0], bn=_np(eng.bn)[0] if bn else None)
    for tag, d in (("module", mod), ("fused", fus)):
        _check(f"{tag} loop loss", np.max(np.abs(d["loss"] - l64) / np.abs(l64)), np.max(np.abs(l32 - l64) / np.abs(l64)), 1e-5)
        _check(f"{tag} loop theta", np.abs(d["theta"] - st.theta)[ok].max(), np.abs(so.theta - st.theta)[ok].max(), 2e-5)
        for nm, theirs, mine in (("m", so.m, st.m), ("v", so.v, st.v), ("vmax", so.vmax, st.vmax)):
            _check(f"{tag} loop {nm}", relerr(d[nm], mine), relerr(theirs, mine), 1e-4)
        if bn:
            _check(f"{tag} loop bn", relerr(d["bn"], st.bn), relerr(so.bn, st.bn), 1e-5)


# ------------------------------------------------------------------ invariants, bit for bit
def _abi(R, n, bn, L, sps, k1, k2, train, x, theta, bn_run, gq):
    """Raw ABI calls -> (q, g, bn_run after, saved)."""
    from vae_equalizer_amd import autograd_ops as ao
    dims = (sps, n, k1, k2)
    run = bn_run.clone() if bn_run is not None else None
    q, saved = ao._enc_forward(x, theta, dims, bn, train, run)
    g = ao._enc_backward(x, theta, q, gq, saved if (bn and train) else run, dims, bn, train)
    torch.cuda.synchronize()
    return q, g, run, saved


@pytest.mark.parametrize("n,bn,L,sps,k1,k2,train", [(8, True, 601, 2, 25, 3, True), (4, True, 300, 3, 7, 5, False), (2, False, 333, 2, 9, 3, True),
                                                    (8, False, 250, 1, 11, 1, True), (4, True, 90, 8, 3, 9, True), (2, True, 700, 2, 5, 3, True)])
def test_same_call_twice_and_runs_are_independent(n, bn, L, sps, k1, k2, train):
    """The same call twice gives identical q and g; R = 3 in one call equals three R = 1 calls."""
    rng = np.random.default_rng(L + n)
    NP, N = ref.offsets(n, k1, k2, 1, bn)[-2], -(-L // sps)
    x = torch.from_numpy((0.5 * rng.standard_normal((3, 2, L))).astype(np.float32)).to(DEV)
    theta = torch.from_numpy(np.stack([ref.init_theta(rng, n, k1, k2, 1, bn)[:NP] for _ in range(3)])).to(DEV)
    run = torch.from_numpy(np.stack([ref.random_bn(rng, n) for _ in range(3)])).to(DEV) if bn else None
    gq = torch.from_numpy(rng.standard_normal((3, 2 * n, N)).astype(np.float32)).to(DEV)
    a = _abi(3, n, bn, L, sps, k1, k2, train, x, theta, run, gq)
    b = _abi(3, n, bn, L, sps, k1, k2, train, x, theta, run, gq)
    _last()
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)
    for i in range(3):
        c = _abi(1, n, bn, L, sps, k1, k2, train, x[i:i + 1].contiguous(), theta[i:i + 1].contiguous(), run[i:i + 1].contiguous() if bn else None,
                 gq[i:i + 1].contiguous())
        for u, v in zip(a, c):
            assert (u is None and v is None) or torch.equal(u[i:i + 1], v)


@pytest.mark.parametrize("n,bn", [(8, True), (4, False), (2, True)])
def test_graph_invariants(n, bn):
    """Non-contiguous x == its contiguous copy; two backward calls through one saved graph agree; parameters modified in place after the
    forward do not change the gradient computed from the saved state."""
    L, sps, k1, k2 = 401, 2, 11, 3
    rng, theta, bn0, x, N = _case(n, bn, L, k1, k2, 99 + n)
    gq = torch.from_numpy(rng.standard_normal((1, 2 * n, N(sps))).astype(np.float32)).to(DEV)
    xw = torch.from_numpy(np.ascontiguousarray(np.stack([x, x], -1))).to(DEV)[None, :, :, 0]      # stride 2 along the samples
    assert not xw.is_contiguous()

    def once(xin, twice=False, poke=False):
        net, _ = _module(n, bn, k1, k2, sps, theta, bn0)
        net.train()
        q = net(xin)
        if poke:
            with torch.no_grad():
                for p in net.parameters():
                    p.data.add_(0.25)
        q.backward(gq, retain_graph=twice)
        g1 = _grads(net).copy()
        if twice:
            net.zero_grad()
            q.backward(gq)
            assert np.array_equal(g1, _grads(net))
        return _np(q), g1

    q0, g0 = once(xw.contiguous())
    for kw in (dict(xin=xw), dict(xin=xw.contiguous(), twice=True), dict(xin=xw.contiguous(), poke=True)):
        q1, g1 = once(**kw)
        assert np.array_equal(q0, q1) and np.array_equal(g0, g1), kw.keys()


def test_requires_grad_subsets():
    """fc1 frozen, or only batch1 trainable: frozen parameters get None, the others are unchanged (bit for bit)."""
    n, L, sps, k1, k2 = 8, 300, 2, 9, 3
    rng, theta, bn0, x, N = _case(n, True, L, k1, k2, 5)
    gq = torch.from_numpy(rng.standard_normal((1, 2 * n, N(sps))).astype(np.float32)).to(DEV)
    xt = torch.from_numpy(x).to(DEV)[None]

    def grads(trainable):
        net, _ = _module(n, True, k1, k2, sps, theta, bn0)
        for name, p in net.named_parameters():
            p.requires_grad_(name.split(".")[0] in trainable)
        net(xt).backward(gq)
        return {name: (None if p.grad is None else _np(p.grad)) for name, p in net.named_parameters()}

    full = grads({"fc1", "fc2", "batch1"})
    for trainable in ({"fc2", "batch1"}, {"batch1"}):
        part = grads(trainable)
        for name in full:
            if name.split(".")[0] in trainable:
                assert np.array_equal(part[name], full[name]), name
            else:
                assert part[name] is None, name
    net, _ = _module(n, True, k1, k2, sps, theta, bn0)
    for p in net.parameters():
        p.requires_grad_(False)
    assert not net(xt).requires_grad


# ------------------------------------------------------------------ bounds
def _lds(L, sps, n, k1, k2, bn):
    from vae_equalizer_amd import _native as nat
    return int(nat.lib().vaeq_nn_enc_lds_bytes(L, sps, n, k1, k2, int(bn)))


@pytest.mark.parametrize("n,bn", [(8, True), (8, False), (4, True), (2, True), (2, False)])
def test_lds_ceiling(n, bn):
    """The longest input whose working set fits (found from vaeq_nn_enc_lds_bytes) runs and is right; one SYMBOL more is refused."""
    from vae_equalizer_amd import _native as nat
    sps, k1, k2 = 2, 25, 3
    lo, hi = 2, 1 << 17
    assert _lds(lo, sps, n, k1, k2, bn) <= LDS_MAX < _lds(hi, sps, n, k1, k2, bn)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _lds(mid, sps, n, k1, k2, bn) <= LDS_MAX else (lo, mid)
    _run(n, bn, lo, sps, k1, k2, True)
    Lbig = lo + sps
    assert _lds(Lbig, sps, n, k1, k2, bn) > LDS_MAX
    rng, theta, bn0, x, N = _case(n, bn, Lbig, k1, k2, 3)
    net, _ = _module(n, bn, k1, k2, sps, theta, bn0)
    xt = torch.from_numpy(x).to(DEV)[None]
    if bn:                                                     # the training-mode forward is resident: refused at once
        with pytest.raises(nat.VaeqError, match="VAEQ_ERR_LDS"):
            net(xt)
    else:                                                      # Net's forward is tiled; its backward is resident
        q = net(xt)
        with pytest.raises(nat.VaeqError, match="VAEQ_ERR_LDS"):
            q.sum().backward()


@pytest.mark.parametrize("n,bn", [(8, True), (8, False), (2, True)])
def test_eval_forward_has_no_length_limit(n, bn):
    """N = 15 000 symbols (the sweep's N_valid) under no_grad, across the tiles of the eval kernel."""
    L, sps, k1, k2 = 30000, 2, 25, 3
    assert _lds(L, sps, n, k1, k2, bn) > LDS_MAX
    rng, theta, bn0, x, N = _case(n, bn, L, k1, k2, 8)
    net, _ = _module(n, bn, k1, k2, sps, theta, bn0)
    net.eval()
    with torch.no_grad():
        q = net(torch.from_numpy(x).to(DEV)[None])
    _last()
    q64 = _ref64(x, theta, None, n, bn, k1, k2, sps, bn0, False)[0]
    q32 = _torch_case(x, theta, None, n, bn, k1, k2, sps, bn0, False, torch.float32)[0]
    _check("long eval q", np.abs(_np(q)[0] - q64).max(), np.abs(q32 - q64).max(), 2e-5)


def test_unsupported_shapes_are_refused():
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.func_VAENN_MQAM import Net
    x = torch.zeros(1, 2, 64, device=DEV)
    for args in ((65, 3, 8, 2), (25, 3, 3, 2), (25, 11, 8, 2), (25, 3, 8, 9)):
        with pytest.raises(nat.VaeqError, match="code -2"):
            Net(*args).to(DEV)(x)


def test_every_instantiation_was_reached():
    """Runs last in this file: every instantiation of the three new kernels was launched by some test above."""
    want = {f"vaeq::nn_enc_forward_kernel<1024, {n}>" for n in (2, 4, 8)} | {f"vaeq::nn_enc_bn_forward_kernel<512, {n}>" for n in (2, 4, 8)}
    want |= {f"vaeq::nn_enc_backward_kernel<512, {n}, {m}>" for n in (2, 4, 8) for m in (0, 1, 2)}
    assert want <= SEEN, sorted(want - SEEN)

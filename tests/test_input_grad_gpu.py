"""The input-signal gradients of the five differentiable operators (vaeq_dp_forward_bwd_x, vaeq_dp_loss_bwd_x, vaeq_awgn_forward_bwd_x,
vaeq_awgn_loss_bwd_x, vaeq_nn_enc_backward_x) from the C ABI up to the modules, against float64 torch autograd through the restatements
tests/_ref_operators.py and tests/_ref_vaenn.py.

Policy (the suite's): against float64 a kernel's error may be FACTOR = 4 times the error of the SAME restatement run in float32 torch on the
CPU (the multiple of test_vaenn_envelope_gpu.py and of _check in test_nn_module_gpu.py), with a floor per operator for near-zero baselines.
Errors are conftest.relerr: max |a - b| / max |b|.  The floors were set a small factor above the largest error of one run on an MI355X (the
commit message records error, baseline and floor per operator); the module prints the largest error of each operator at its end (-s).

_ref_vaenn.forward detaches x (its _t() casts through .detach()), so it cannot yield d/dx: the encoder restatement below (_enc_ref) is the
same arithmetic -- _ref_operators.vaenn_net for Net, the BatchNorm lines of _ref_vaenn.forward for Net_BN -- with x left in the graph, and is
checked against _ref_vaenn.forward's q in float64 before it is relied on (test_encoder_restatement_equals_ref_vaenn)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ref_operators as ref
import _ref_vaenn as refnn
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
# three times the largest error of that run, rounded: dp_fir 3.3e-6 (baseline 3.9e-6), awgn_fir 2.2e-6 (2.7e-6), dp_loss 4.7e-7 (2.7e-7), awgn_loss 2.6e-7 (1.7e-7),
# enc 1.05e-6 (3.5e-7), e2e 2.2e-6 (2.7e-6)
FLOOR = dict(dp_fir=1e-5, awgn_fir=7e-6, dp_loss=1.5e-6, awgn_loss=8e-7, enc=3e-6, e2e=7e-6)
LOSS_TOL = 1e-5                                             # the loss tolerance of test_autograd_ops_gpu.py (relative)
VAEQ_ERR_LDS = -3
STATS, SEEN = {}, set()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(STATS):
        print(f"  {k}: {STATS[k]:.3g}")


def _check(tag, got, r64, r32, ctx=""):
    err, base = relerr(got, r64), relerr(r32, r64)
    STATS[f"{tag} err"] = max(STATS.get(f"{tag} err", 0.0), err)
    STATS[f"{tag} f32-baseline err"] = max(STATS.get(f"{tag} f32-baseline err", 0.0), base)
    print(f"{tag} {ctx}: err {err:.3g} baseline {base:.3g}")
    assert np.isfinite(err) and err <= max(FACTOR * base, FLOOR[tag]), (tag, ctx, err, base)


def _lib():
    from vae_equalizer_amd import _native as nat
    return nat, nat.lib()


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _h(t):
    return t.detach().cpu().numpy()


def _t(a, dt):
    """float32 values as the kernel sees them, in `dt` for the restatement."""
    return torch.tensor(np.asarray(a, np.float32)).to(dt)


def _call(fn_name, *args):
    nat, L = _lib()
    rc = getattr(L, fn_name)(*[nat.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], nat.current_stream(torch.device(DEV)))
    name = nat.last_kernel()
    torch.cuda.synchronize()
    return int(rc), name


def _run(fn_name, *args):
    nat, _ = _lib()
    rc, name = _call(fn_name, *args)
    nat.check(rc, fn_name)
    SEEN.add(name)
    return name


def _levels(n):
    return (np.arange(-(n - 1), n, 2) / np.sqrt((n * n - 1) / 3.0 * 2)).astype(np.float32)


def _prior(rng, n):
    p = rng.uniform(0.2, 1.0, n)
    p = (p + p[::-1]) / 2
    return (p / p.sum()).astype(np.float32)


def _q(rng, lead, n, B):
    z = 2.0 * rng.standard_normal((*lead, n, B))
    q = np.exp(z - z.max(-2, keepdims=True))
    q /= q.sum(-2, keepdims=True)
    return q.reshape(*lead[:-1], lead[-1] * n, B).astype(np.float32)


def _taps(rng, shape, M, dirac):
    W = (0.3 * rng.standard_normal(shape) / np.sqrt(M)).astype(np.float32)
    for idx in dirac:
        W[idx + (M // 2,)] += 1.0
    return W


# ------------------------------------------------------------------ DP FIR: vaeq_dp_forward_bwd_x
def _dp_fir_data(rng, R, n, sps, M, N, gy_null):
    d = dict(x=(0.5 * rng.standard_normal((R, 2, 2, N * sps))).astype(np.float32),
             W=np.stack([_taps(rng, (2, 4, M), M, [(0, 0), (1, 1)]) for _ in range(R)]), amp=_levels(n),
             var=rng.uniform(0.01, 0.05, (R, 2)).astype(np.float32), nu=rng.uniform(0, 1, R).astype(np.float32),
             gq=rng.standard_normal((R, 2, 2 * n, N)).astype(np.float32),
             gy=None if gy_null else rng.standard_normal((R, 2, 2, N)).astype(np.float32))
    return d


def _dp_fir_gpu(d, sps, runs=None, scale=1.0):
    """-> gx[R', 2, 2, L] for the runs `runs` (default all) in ONE call."""
    sl = slice(None) if runs is None else runs
    x, W, var, nu = _g(d["x"][sl]), _g(d["W"][sl]), _g(d["var"][sl]), _g(d["nu"][sl])
    R, N, M, n = x.shape[0], x.shape[-1] // sps, W.shape[-1], len(d["amp"])
    q, y = torch.empty(R, 2, 2 * n, N, device=DEV), torch.empty(R, 2, 2, N, device=DEV)
    _run("vaeq_dp_forward", R, N, sps, M, n, x, W, _g(d["amp"]), var, nu, q, y)
    gx = torch.full((R, 2, 2, N * sps), float("nan"), device=DEV)
    gq, gy = _g(scale * d["gq"][sl]), None if d["gy"] is None else _g(scale * d["gy"][sl])
    name = _run("vaeq_dp_forward_bwd_x", R, N, sps, M, n, W, q, y, gq, gy, _g(d["amp"]), var, gx)
    assert name == f"vaeq::dp_forward_bwd_x_kernel<{n}>"
    return _h(gx)


def _dp_fir_ref(d, r, sps, dt):
    x = _t(d["x"][r], dt).requires_grad_(True)
    q, y = ref.dp_forward(x, _t(d["W"][r], dt), _t(d["amp"], dt), _t(d["var"][r], dt), float(d["nu"][r]), sps)
    obj = (q * _t(d["gq"][r], dt)).sum() + (0 if d["gy"] is None else (y * _t(d["gy"][r], dt)).sum())
    return torch.autograd.grad(obj, x)[0].numpy().astype(np.float64)


# n, sps, M, N, gy_null: every n_lev, sps 1 / 2 / 3, M 1 / 9 / 25 / 63, odd and even N, N below M, with and without gy
FIR_GRID = [(2, 1, 1, 40, False), (4, 2, 9, 40, True), (8, 3, 25, 41, False), (8, 2, 63, 100, True), (2, 3, 63, 7, False), (4, 1, 25, 211, True),
            (8, 2, 25, 100, False), (4, 2, 13, 50, False), (2, 2, 9, 1, False), (8, 1, 9, 500, True), (4, 3, 1, 33, False)]


@pytest.mark.parametrize("n,sps,M,N,gy_null", FIR_GRID)
def test_dp_fir_input_gradient(n, sps, M, N, gy_null):
    d = _dp_fir_data(np.random.default_rng(100 + n + 10 * sps + M + N), 1, n, sps, M, N, gy_null)
    gx = _dp_fir_gpu(d, sps)
    assert np.isfinite(gx).all()
    _check("dp_fir", gx[0], _dp_fir_ref(d, 0, sps, torch.float64), _dp_fir_ref(d, 0, sps, torch.float32), (n, sps, M, N, gy_null))


def test_dp_fir_structure():
    """Linear in the upstream gradient (x 2 exactly), R runs in one call == R single calls, two calls identical -- bit for bit."""
    d = _dp_fir_data(np.random.default_rng(7), 3, 8, 2, 25, 101, False)
    a = _dp_fir_gpu(d, 2)
    assert np.array_equal(a, _dp_fir_gpu(d, 2))
    assert np.array_equal(2.0 * a, _dp_fir_gpu(d, 2, scale=2.0))
    for r in range(3):
        assert np.array_equal(a[r:r + 1], _dp_fir_gpu(d, 2, runs=slice(r, r + 1)))


# ------------------------------------------------------------------ AWGN FIR: vaeq_awgn_forward_bwd_x
def _awgn_fir_data(rng, R, n, sps, M, N, gy_null):
    amp = _levels(n)
    return dict(x=(0.5 * rng.standard_normal((R, 2, N * sps))).astype(np.float32), W=np.stack([_taps(rng, (2, M), M, [(0,)]) for _ in range(R)]),
                amp=amp, am=np.full(R, np.mean(np.abs(amp)), np.float32) * rng.uniform(0.9, 1.1, R).astype(np.float32),
                var=rng.uniform(0.02, 0.1, R).astype(np.float32), gq=rng.standard_normal((R, 2 * n, N)).astype(np.float32),
                gy=None if gy_null else rng.standard_normal((R, 2, N)).astype(np.float32))


def _awgn_fir_gpu(d, sps, runs=None, scale=1.0):
    sl = slice(None) if runs is None else runs
    x, W = _g(d["x"][sl]), _g(d["W"][sl])
    R, N, M, n = x.shape[0], x.shape[-1] // sps, W.shape[-1], len(d["amp"])
    gx = torch.full((R, 2, N * sps), float("nan"), device=DEV)
    name = _run("vaeq_awgn_forward_bwd_x", R, N, sps, M, n, x, W, _g(d["amp"]), _g(d["am"][sl]), _g(d["var"][sl]), _g(scale * d["gq"][sl]),
                None if d["gy"] is None else _g(scale * d["gy"][sl]), gx)
    assert name == f"vaeq::awgn_forward_bwd_x_kernel<{n}>"
    return _h(gx)


def _awgn_fir_ref(d, r, sps, dt):
    x = _t(d["x"][r], dt).requires_grad_(True)
    q, y = ref.awgn_forward(x, _t(d["W"][r], dt)[None], _t(d["amp"], dt), float(d["am"][r]), float(d["var"][r]), sps)
    obj = (q * _t(d["gq"][r], dt)).sum() + (0 if d["gy"] is None else (y * _t(d["gy"][r], dt)).sum())
    return torch.autograd.grad(obj, x)[0].numpy().astype(np.float64)


@pytest.mark.parametrize("n,sps,M,N,gy_null", [c for c in FIR_GRID if c[3] > 1] + [(4, 2, 25, 350, False), (2, 2, 9, 1, False)])
def test_awgn_fir_input_gradient(n, sps, M, N, gy_null):
    # (N = 1: the normalisation maps y to +-amp_mean, q does not depend on x; that case carries a gy so that the gradient is not all rounding)
    d = _awgn_fir_data(np.random.default_rng(200 + n + 10 * sps + M + N), 1, n, sps, M, N, gy_null)
    gx = _awgn_fir_gpu(d, sps)
    assert np.isfinite(gx).all()
    _check("awgn_fir", gx[0], _awgn_fir_ref(d, 0, sps, torch.float64), _awgn_fir_ref(d, 0, sps, torch.float32), (n, sps, M, N, gy_null))


def test_awgn_fir_structure():
    d = _awgn_fir_data(np.random.default_rng(8), 3, 4, 2, 25, 101, False)
    a = _awgn_fir_gpu(d, 2)
    assert np.array_equal(a, _awgn_fir_gpu(d, 2))
    assert np.array_equal(2.0 * a, _awgn_fir_gpu(d, 2, scale=2.0))
    for r in range(3):
        assert np.array_equal(a[r:r + 1], _awgn_fir_gpu(d, 2, runs=slice(r, r + 1)))


# ------------------------------------------------------------------ the two ELBO losses: vaeq_dp_loss_bwd_x, vaeq_awgn_loss_bwd_x
def _loss_data(rng, R, dp, n, sps, M, B):
    lead = (2, 2) if dp else (2,)
    return dict(q=np.stack([_q(rng, lead, n, B) for _ in range(R)]), x=rng.standard_normal((R, *lead, B * sps)).astype(np.float32),
                h=(0.3 * rng.standard_normal((R, *lead, 2, M) if dp else (R, 2, M))).astype(np.float32), amp=_levels(n),
                P=np.stack([_prior(rng, n) for _ in range(R)]), up=rng.choice([-2.3, 0.37, 3.1], R).astype(np.float32))


def _loss_gpu(d, dp, sps, runs=None):
    sl = slice(None) if runs is None else runs
    q, x, h = _g(d["q"][sl]), _g(d["x"][sl]), _g(d["h"][sl])
    R, B, M, n = q.shape[0], q.shape[-1], h.shape[-1], len(d["amp"])
    gx = torch.full(x.shape, float("nan"), device=DEV)
    fn = "vaeq_dp_loss_bwd_x" if dp else "vaeq_awgn_loss_bwd_x"
    name = _run(fn, R, B, sps, M, n, q, x, h, _g(d["amp"]), _g(d["up"][sl]), gx)
    assert name == f"vaeq::{fn[5:]}_kernel<{n}>"
    return _h(gx)


def _loss_ref(d, r, dp, dt):
    x = _t(d["x"][r], dt).requires_grad_(True)
    args = (_t(d["q"][r], dt), x, _t(d["h"][r], dt), _t(d["amp"], dt), _t(d["P"][r], dt))
    loss = ref.dp_loss(*args)[0] if dp else ref.awgn_loss(*args)
    return torch.autograd.grad(float(d["up"][r]) * loss, x)[0].numpy().astype(np.float64)


# n, sps, M, B: B from its minimum (2 (M // 2) + 1), odd and even
LOSS_GRID = [(2, 1, 1, 1), (4, 2, 9, 40), (8, 3, 25, 41), (8, 2, 63, 100), (2, 3, 63, 63), (4, 1, 25, 211), (8, 2, 25, 100), (4, 2, 13, 50), (4, 2, 25, 350),
             (8, 2, 25, 300), (2, 2, 9, 9)]


@pytest.mark.parametrize("dp", [True, False])
@pytest.mark.parametrize("n,sps,M,B", LOSS_GRID)
def test_loss_input_gradient(dp, n, sps, M, B):
    d = _loss_data(np.random.default_rng(300 + n + 10 * sps + M + B + dp), 1, dp, n, sps, M, B)
    gx = _loss_gpu(d, dp, sps)
    mh = M // 2
    assert np.isfinite(gx).all()
    assert np.all(gx[..., :mh] == 0.0) and np.all(gx[..., B * sps - mh:] == 0.0)      # exactly zero on the mh samples at either end
    assert np.all(gx[..., mh:B * sps - mh] != 0.0)
    _check("dp_loss" if dp else "awgn_loss", gx[0], _loss_ref(d, 0, dp, torch.float64), _loss_ref(d, 0, dp, torch.float32), (n, sps, M, B))


@pytest.mark.parametrize("dp", [True, False])
def test_loss_structure(dp):
    d = _loss_data(np.random.default_rng(9), 3, dp, 8, 2, 25, 101)
    a = _loss_gpu(d, dp, 2)
    assert np.array_equal(a, _loss_gpu(d, dp, 2))
    for r in range(3):
        assert np.array_equal(a[r:r + 1], _loss_gpu(d, dp, 2, runs=slice(r, r + 1)))
    d2 = dict(d, up=2.0 * d["up"])                             # linear in the upstream gradient
    assert np.array_equal(2.0 * a, _loss_gpu(d2, dp, 2))


# ------------------------------------------------------------------ the VAE-NN encoder: vaeq_nn_enc_backward_x
def _enc_ref(x, theta, gq, n, bn, k1, k2, sps, bn0, train, dt):
    """Net / Net_BN forward with x in the graph -> (q, d sum(q gq) / dx, d / dtheta_net) in float64 numpy."""
    C_ = 2 * n
    th = torch.tensor(np.asarray(theta, np.float32)).to(dt).requires_grad_(True)
    xt = _t(x, dt).requires_grad_(True)
    if not bn:
        q = ref.vaenn_net(xt, th, n, k1, k2, sps, 1)[0]
    else:
        w1, b1, w2, b2, ga, be, _ = torch.split(th, refnn.sizes(n, k1, k2, 1, True))
        z = F.elu(F.conv1d(xt[None], w1.reshape(C_, 2, k1), b1, padding=k1 // 2))[0]
        b0 = _t(bn0, dt)
        if train:
            mean = z.mean(-1)
            var = ((z - mean[:, None]) ** 2).mean(-1)
            zh = (z - mean[:, None]) / torch.sqrt(var[:, None] + refnn.BN_EPS)
        else:
            zh = (z - b0[:C_, None]) / torch.sqrt(b0[C_:, None] + refnn.BN_EPS)
        a2 = F.conv1d((ga[:, None] * zh + be[:, None])[None], w2.reshape(C_, C_, k2), b2, padding=k2 // 2, stride=sps)[0]
        q = torch.cat([torch.softmax(a2[:n], 0), torch.softmax(a2[n:], 0)])
    gx, gth = torch.autograd.grad((q * _t(gq, dt)).sum(), (xt, th))
    return q.detach().numpy().astype(np.float64), gx.numpy().astype(np.float64), gth.numpy()[:-2].astype(np.float64)


@pytest.mark.parametrize("n,bn,train", [(2, False, True), (4, True, True), (8, True, False)])
def test_encoder_restatement_equals_ref_vaenn(n, bn, train):
    rng = np.random.default_rng(n)
    theta, bn0 = refnn.init_theta(rng, n, 9, 3, 1, bn), (refnn.random_bn(rng, n) if bn else None)
    x = (0.5 * rng.standard_normal((2, 77))).astype(np.float32)
    gq = rng.standard_normal((2 * n, 39)).astype(np.float32)
    q, gx, _ = _enc_ref(x, theta, gq, n, bn, 9, 3, 2, bn0, train, torch.float64)
    q_ref = refnn.forward(x, theta, n, 9, 3, 2, 1, bn, bn0, train=train)[0].numpy()
    assert np.abs(q - q_ref).max() < 1e-14
    assert np.isfinite(gx).all() and np.abs(gx).max() > 0


# n, bn, L, sps, k1, k2: every n_lev, Net and Net_BN, sps 1 / 2 / 3, k1 1 / 25 / 63, k2 1 / 3 / 9, L % sps != 0, the goldens' shapes (G8, G11)
ENC_GRID = [(2, False, 37, 1, 1, 1), (2, True, 83, 2, 25, 3), (2, False, 101, 3, 63, 9), (4, False, 121, 2, 25, 3), (4, True, 200, 3, 63, 9),
            (4, True, 64, 1, 1, 1), (8, False, 600, 2, 25, 3), (8, True, 600, 2, 25, 3), (8, True, 641, 2, 63, 1), (8, False, 17, 3, 63, 9),
            (8, True, 65, 3, 1, 9), (4, False, 120, 2, 11, 3)]


def _enc_case(n, bn, L, sps, k1, k2, train):
    from vae_equalizer_amd import autograd_ops
    from vae_equalizer_amd.func_VAENN_MQAM import Net, Net_BN, theta_to_net
    rng = np.random.default_rng(L * 31 + sps * 7 + k1 * 3 + k2 + n + bn)
    theta, bn0 = refnn.init_theta(rng, n, k1, k2, 1, bn), (refnn.random_bn(rng, n) if bn else None)
    x = (0.5 * rng.standard_normal((2, L))).astype(np.float32)
    gq = rng.standard_normal((2 * n, -(-L // sps))).astype(np.float32)
    grads = []
    for with_x in (True, False):
        net = (Net_BN if bn else Net)(k1, k2, n, sps).to(DEV)
        theta_to_net(torch.from_numpy(theta).to(DEV), net, None if bn0 is None else torch.from_numpy(bn0))
        net.train(train)
        xt = _g(x)[None].requires_grad_(with_x)
        q = net(xt)
        q.backward(_g(gq)[None])
        torch.cuda.synchronize()
        SEEN.add(autograd_ops.LAST_BACKWARD_KERNEL)
        mode = (1 if train else 2) if bn else 0
        assert autograd_ops.LAST_BACKWARD_KERNEL == f"vaeq::nn_enc_backward{'_x' if with_x else ''}_kernel<512, {n}, {mode}>"
        grads.append([p.grad.clone() for p in net._params()])
        if with_x:
            gx = _h(xt.grad)[0]
        else:
            assert xt.grad is None
    for a, b in zip(*grads):                                   # the parameter gradients do not change when x asks for its own
        assert a.abs().max() > 0 and torch.equal(a, b)
    r64 = _enc_ref(x, theta, gq, n, bn, k1, k2, sps, bn0, train, torch.float64)
    r32 = _enc_ref(x, theta, gq, n, bn, k1, k2, sps, bn0, train, torch.float32)
    assert gx.shape == (2, L) and np.isfinite(gx).all()
    _check("enc", gx, r64[1], r32[1], (n, bn, L, sps, k1, k2, train))
    return x, theta, bn0, gq, gx


@pytest.mark.parametrize("n,bn,L,sps,k1,k2", ENC_GRID)
def test_encoder_input_gradient_training_mode(n, bn, L, sps, k1, k2):
    _enc_case(n, bn, L, sps, k1, k2, True)


@pytest.mark.parametrize("n,bn,L,sps,k1,k2", [c for c in ENC_GRID if c[1]])
def test_encoder_input_gradient_eval_mode(n, bn, L, sps, k1, k2):
    _enc_case(n, bn, L, sps, k1, k2, False)


def _enc_abi(R, n, bn, train, L, sps, k1, k2, x, theta, bn0, gq):
    """vaeq_nn_enc_forward + vaeq_nn_enc_backward_x through ctypes -> (rc of the backward, g_theta[R, NP], gx[R, 2, L])."""
    N = -(-L // sps)
    xg, th = _g(x), _g(theta)
    q = torch.empty(R, 2 * n, N, device=DEV)
    run_stats = _g(bn0) if bn else None
    saved = torch.empty(R, 4 * n, device=DEV) if bn and train else None
    rc, _ = _call("vaeq_nn_enc_forward", R, L, sps, n, k1, k2, int(bn), int(train), xg, th, run_stats.clone() if bn else None, saved, q)
    g, gx = torch.full_like(th, float("nan")), torch.full((R, 2, L), float("nan"), device=DEV)
    stats = saved if bn and train else run_stats
    rc2, name = _call("vaeq_nn_enc_backward_x", R, L, sps, n, k1, k2, int(bn), int(train), xg, th, q, _g(gq), stats, g, gx)
    return rc, rc2, name, _h(g), _h(gx)


@pytest.mark.parametrize("n,bn,train", [(8, True, True), (4, False, True), (2, True, False)])
def test_encoder_structure(n, bn, train):
    """R runs in one call == R single calls, and two calls are identical -- bit for bit, parameter and input gradients alike."""
    rng = np.random.default_rng(11 + n)
    R, L, sps, k1, k2 = 3, 203, 2, 25, 3
    theta = np.stack([refnn.init_theta(rng, n, k1, k2, 1, bn)[:-2] for _ in range(R)])
    bn0 = np.stack([refnn.random_bn(rng, n) for _ in range(R)]) if bn else None
    x = (0.5 * rng.standard_normal((R, 2, L))).astype(np.float32)
    gq = rng.standard_normal((R, 2 * n, -(-L // sps))).astype(np.float32)
    rc, rc2, name, g, gx = _enc_abi(R, n, bn, train, L, sps, k1, k2, x, theta, bn0, gq)
    assert (rc, rc2) == (0, 0) and np.isfinite(g).all() and np.isfinite(gx).all()
    again = _enc_abi(R, n, bn, train, L, sps, k1, k2, x, theta, bn0, gq)
    assert np.array_equal(g, again[3]) and np.array_equal(gx, again[4])
    for r in range(R):
        one = _enc_abi(1, n, bn, train, L, sps, k1, k2, x[r:r + 1], theta[r:r + 1], None if bn0 is None else bn0[r:r + 1], gq[r:r + 1])
        assert np.array_equal(g[r:r + 1], one[3]) and np.array_equal(gx[r:r + 1], one[4])


@pytest.mark.parametrize("n,bn", [(8, True), (4, False)])
def test_encoder_lds_ceiling(n, bn):
    """The longest input vaeq_nn_enc_lds_bytes admits runs and is right; one symbol more is refused with VAEQ_ERR_LDS."""
    _, L_ = _lib()
    sps, k1, k2, LDS_MAX = 2, 25, 3, 160 * 1024
    lds = lambda L: int(L_.vaeq_nn_enc_lds_bytes(L, sps, n, k1, k2, int(bn)))
    lo, hi = 2, 1 << 17
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lds(mid) <= LDS_MAX else (lo, mid)
    assert lds(lo) <= LDS_MAX < lds(lo + sps)
    rng = np.random.default_rng(5)
    theta = refnn.init_theta(rng, n, k1, k2, 1, bn)
    bn0 = refnn.random_bn(rng, n) if bn else None
    for L, want in ((lo, 0), (lo + sps, VAEQ_ERR_LDS)):
        x = (0.5 * rng.standard_normal((2, L))).astype(np.float32)
        gq = rng.standard_normal((2 * n, -(-L // sps))).astype(np.float32)
        if want == 0:
            rc, rc2, name, g, gx = _enc_abi(1, n, bn, True, L, sps, k1, k2, x[None], theta[None, :-2], None if bn0 is None else bn0[None], gq[None])
            assert (rc, rc2) == (0, 0)
            r64 = _enc_ref(x, theta, gq, n, bn, k1, k2, sps, bn0, True, torch.float64)
            r32 = _enc_ref(x, theta, gq, n, bn, k1, k2, sps, bn0, True, torch.float32)
            _check("enc", gx[0], r64[1], r32[1], ("ceiling", n, bn, L))
        else:                                                  # refused before anything is launched: no forward needed, the buffers stay as they are
            g, gx = torch.zeros(1, theta.size - 2, device=DEV), torch.zeros(1, 2, L, device=DEV)
            q = torch.zeros(1, 2 * n, -(-L // sps), device=DEV)
            rc2, _ = _call("vaeq_nn_enc_backward_x", 1, L, sps, n, k1, k2, int(bn), 1, _g(x[None]), _g(theta[None, :-2]), q, _g(gq[None]),
                           torch.zeros(1, 4 * n, device=DEV) if bn else None, g, gx)
            assert rc2 == want and not gx.any() and not g.any()


# ------------------------------------------------------------------ the wrappers: ragged lengths, gy = None, frozen weights, no graph
@pytest.mark.parametrize("dp", [True, False])
@pytest.mark.parametrize("L,sps", [(201, 2), (100, 3), (99, 2)])
def test_fir_modules_pad_inside_the_graph(dp, L, sps):
    """L not a multiple of sps: the padded tail's gradient is dropped; out unused (gy = None) in one case, used in the other."""
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw, shared_funcs as sfun
    rng = np.random.default_rng(L + sps + dp)
    n, M = 4, 9
    amp = _levels(n)
    x = (0.5 * rng.standard_normal((2, 2, L) if dp else (2, L))).astype(np.float32)
    W = _taps(rng, (2, 4, M), M, [(0, 0), (1, 1)]) if dp else _taps(rng, (1, 2, M), M, [(0, 0)])
    var = np.array([0.02, 0.03], np.float32) if dp else 0.05
    N = -(-L // sps)
    gq, gy = rng.standard_normal((2, 2 * n, N) if dp else (2 * n, N)).astype(np.float32), rng.standard_normal((2, 2, N) if dp else (2, N)).astype(np.float32)
    net = (sfun.twoXtwoFIR if dp else aw.twoFIR)(M, sps).to(DEV)
    with torch.no_grad():
        net.conv_w.weight.copy_(_g(W))
    for use_y in (False, True):
        xt = _g(x).requires_grad_(True)
        q, y = net(xt, _g(amp), _g(var), 0.3) if dp else net(xt, _g(amp), 0.6, var)
        ((q * _g(gq)).sum() + ((y * _g(gy)).sum() if use_y else 0)).backward()
        assert xt.grad.shape == xt.shape

        def r(dt):
            x_ = _t(x, dt).requires_grad_(True)
            q_, y_ = ref.dp_forward(x_, _t(W, dt), _t(amp, dt), _t(var, dt), 0.3, sps) if dp else ref.awgn_forward(x_, _t(W, dt), _t(amp, dt), 0.6, var, sps)
            return torch.autograd.grad((q_ * _t(gq, dt)).sum() + ((y_ * _t(gy, dt)).sum() if use_y else 0), x_)[0].numpy().astype(np.float64)
        _check("dp_fir" if dp else "awgn_fir", _h(xt.grad), r(torch.float64), r(torch.float32), ("module", L, sps, use_y))


@pytest.mark.parametrize("kind", ["dp", "awgn", "vaenn"])
def test_parameter_gradients_do_not_change_when_the_input_asks_for_its_own(kind):
    """FIR module -> loss function, with and without the received signal requiring a gradient: conv_w.weight.grad, h.grad and dL/dq (through a
    retained q) are torch.equal -- the same kernels run on the same operands either way.  vaenn: the VAE-NN loss (P = None) behind twoFIR."""
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw, func_VAENN_MQAM as nn_, shared_funcs as sfun
    rng = np.random.default_rng(31)
    n, M, sps, B = 4, 9, 2, 60
    amp, P = _g(_levels(n)), _g(_prior(rng, n))
    dp = kind == "dp"
    x = (0.5 * rng.standard_normal((2, 2, B * sps) if dp else (2, B * sps))).astype(np.float32)
    W = _taps(rng, (2, 4, M), M, [(0, 0), (1, 1)]) if dp else _taps(rng, (1, 2, M), M, [(0, 0)])
    h0 = (0.3 * rng.standard_normal((2, 2, 2, M) if dp else (2, M))).astype(np.float32)
    got = []
    for with_x in (False, True):
        net = (sfun.twoXtwoFIR if dp else aw.twoFIR)(M, sps).to(DEV)
        with torch.no_grad():
            net.conv_w.weight.copy_(_g(W))
        h = _g(h0).requires_grad_(True)
        rx = _g(x).requires_grad_(with_x)
        q, out = net(rx, amp, _g([0.02, 0.03]), 0.3) if dp else net(rx, amp, 0.6, 0.05)
        q.retain_grad()
        if dp:
            loss = sfun.loss_function_shaping(q, rx, h, amp, P)[0]
        else:
            loss = aw.loss_function(q, rx, h, DEV, amp, P) if kind == "awgn" else nn_.loss_function(q, rx, h, DEV, amp)
        (loss + 0.5 * (out * out).sum()).backward()            # `out` used too: gy is not None
        assert (rx.grad is not None) == with_x
        got.append((net.conv_w.weight.grad.clone(), h.grad.clone(), q.grad.clone(), loss.detach().clone()))
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)


@pytest.mark.parametrize("dp", [True, False])
def test_loss_gradients_alone_do_not_change_when_rx_asks_for_its_own(dp):
    """The loss functions on their own (q and h leaves): dL/dq and dL/dh with rx.requires_grad are torch.equal to those without."""
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw, func_VAENN_MQAM as nn_, shared_funcs as sfun
    d = _loss_data(np.random.default_rng(32), 1, dp, 8, 2, 25, 100)
    amp, P = _g(d["amp"]), _g(d["P"][0])
    forms = ["dp"] if dp else ["awgn", "vaenn"]
    for form in forms:
        got = []
        for with_x in (False, True):
            q, h, rx = _g(d["q"][0]).requires_grad_(True), _g(d["h"][0]).requires_grad_(True), _g(d["x"][0]).requires_grad_(with_x)
            loss = (sfun.loss_function_shaping(q, rx, h, amp, P)[0] if dp else
                    aw.loss_function(q, rx, h, DEV, amp, P) if form == "awgn" else nn_.loss_function(q, rx, h, DEV, amp))
            (1.7 * loss).backward()
            assert (rx.grad is not None) == with_x
            got.append((q.grad.clone(), h.grad.clone()))
        for a, b in zip(*got):
            assert a.abs().max() > 0 and torch.equal(a, b)


def test_no_graph_without_a_gradient_anywhere():
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.func_VAENN_MQAM import Net
    net = sfun.twoXtwoFIR(9, 2).to(DEV).requires_grad_(False)
    x = torch.randn(2, 2, 80, device=DEV)
    q, out = net(x, _g(_levels(4)), _g([0.02, 0.02]), 0.0)
    assert not q.requires_grad and q.grad_fn is None
    with torch.no_grad():
        q, out = net(x.clone().requires_grad_(True), _g(_levels(4)), _g([0.02, 0.02]), 0.0)
    assert not q.requires_grad
    enc = Net(9, 3, 4, 2).to(DEV).requires_grad_(False)
    assert enc(torch.randn(1, 2, 80, device=DEV)).grad_fn is None
    assert enc(torch.randn(1, 2, 80, device=DEV, requires_grad=True)).grad_fn is not None


def test_double_backward_raises():
    from vae_equalizer_amd import shared_funcs as sfun
    net = sfun.twoXtwoFIR(9, 2).to(DEV)
    x = torch.randn(2, 2, 80, device=DEV, requires_grad=True)
    q, out = net(x, _g(_levels(4)), _g([0.02, 0.02]), 0.0)
    (gx,) = torch.autograd.grad((q * q).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ------------------------------------------------------------------ end to end: a trainable IQ compensator in front of the equalizer
def _mix(x, A):
    """x[..., 2 (I, Q), L] through a real 2 x 2 matrix per polarisation: A[2, 2, 2] (DP) or A[2, 2] (single polarisation)."""
    return torch.einsum("pij,pjl->pil", A, x) if A.dim() == 3 else A @ x


def _front(rng, dp, dt=torch.float32, dev="cpu"):
    A = np.eye(2) + 0.05 * rng.standard_normal((2, 2, 2) if dp else (2, 2))
    return torch.tensor(A.astype(np.float32), device=dev).to(dt).requires_grad_(True)


def _e2e_dp_ref(A0, x, W, h, amp, P, var, nu, sps, dt):
    A = _t(A0, dt).requires_grad_(True)
    rx = _mix(_t(x, dt), A)
    q, _ = ref.dp_forward(rx, _t(W, dt), _t(amp, dt), _t(var, dt), nu, sps)
    loss = ref.dp_loss(q, rx, _t(h, dt), _t(amp, dt), _t(P, dt))[0]
    loss.backward()
    return float(loss.detach()), A.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("frozen", [False, True])
def test_end_to_end_dp_front_end(frozen):
    """rx = A x feeds both twoXtwoFIR and loss_function_shaping (G1's first minibatch); dL/dA against the float64 restatement of the same graph.
    frozen: the equalizer's taps do not require a gradient."""
    from vae_equalizer_amd import shared_funcs as sfun
    g = load_golden("G1_dp_step_64qam_pcs")
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    x = g["rx"][:, :, :B * sps]
    rng = np.random.default_rng(21)
    A0 = _h(_front(rng, True))
    net = sfun.twoXtwoFIR(M, sps).to(DEV)
    with torch.no_grad():
        net.conv_w.weight.copy_(_g(g["W0"]))
    net.requires_grad_(not frozen)
    h = _g(g["h0"]).requires_grad_(not frozen)
    A = _g(A0).requires_grad_(True)
    rx = _mix(_g(x), A)
    q, out = net(rx, _g(g["amp_levels"]), _g(g["var"]), float(g["nu_sc"]))
    loss, _ = sfun.loss_function_shaping(q, rx, h, _g(g["amp_levels"]), _g(g["P"]))
    loss.backward()
    assert A.grad is not None, "the front end received no gradient"
    assert (net.conv_w.weight.grad is None) == frozen and (h.grad is None) == frozen
    args = (A0, x, g["W0"], g["h0"], g["amp_levels"], g["P"], g["var"], float(g["nu_sc"]), sps)
    (l64, g64), (l32, g32) = _e2e_dp_ref(*args, torch.float64), _e2e_dp_ref(*args, torch.float32)
    assert abs(float(loss.detach()) - l64) / abs(l64) < LOSS_TOL
    _check("e2e", _h(A.grad), g64, g32, ("dp", frozen))


def test_end_to_end_awgn_front_end():
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw
    g = load_golden("G4_awgn_16qam_cfg1")
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    x, am, var = g["rx"][:, :B * sps], float(g["amp_mean"]), float(g["var"])
    A0 = _h(_front(np.random.default_rng(22), False))
    net = aw.twoFIR(M, sps).to(DEV)
    with torch.no_grad():
        net.conv_w.weight.copy_(_g(g["W0"]).reshape(1, 2, M))
    h = _g(g["h0"]).requires_grad_(True)
    A = _g(A0).requires_grad_(True)
    rx = _mix(_g(x), A)
    q, out = net(rx, _g(g["amp_levels"]), am, var)
    loss = aw.loss_function(q, rx, h, DEV, _g(g["amp_levels"]), _g(g["P"]))
    loss.backward()
    assert A.grad is not None, "the front end received no gradient"

    def r(dt):
        A_ = _t(A0, dt).requires_grad_(True)
        rx_ = _mix(_t(x, dt), A_)
        q_, _ = ref.awgn_forward(rx_, _t(g["W0"], dt).reshape(1, 2, M), _t(g["amp_levels"], dt), am, var, sps)
        l_ = ref.awgn_loss(q_, rx_, _t(g["h0"], dt), _t(g["amp_levels"], dt), _t(g["P"], dt))
        l_.backward()
        return float(l_.detach()), A_.grad.numpy().astype(np.float64)
    (l64, g64), (l32, g32) = r(torch.float64), r(torch.float32)
    assert abs(float(loss.detach()) - l64) / abs(l64) < LOSS_TOL
    _check("e2e", _h(A.grad), g64, g32, "awgn")


def test_end_to_end_vaenn_front_end():
    """Net + the VAE-NN loss (P = None) on G8's first minibatch."""
    from vae_equalizer_amd import func_VAENN_MQAM as nn_
    g = load_golden("G8_vaenn_64qam")
    B, sps, k1, k2, M = int(g["B"]), int(g["sps"]), int(g["k1"]), int(g["k2"]), int(g["M_est"])
    n = len(g["amp_levels"])
    x = g["rx"][:, :B * sps]
    A0 = _h(_front(np.random.default_rng(23), False))
    net = nn_.Net(k1, k2, n, sps).to(DEV)
    h = nn_.theta_to_net(torch.from_numpy(g["theta0"]).to(DEV), net).requires_grad_(True)
    A = _g(A0).requires_grad_(True)
    rx = _mix(_g(x), A)
    q = net(rx[None])[0]
    loss = nn_.loss_function(q, rx, h, DEV, _g(g["amp_levels"]))
    loss.backward()
    assert A.grad is not None, "the front end received no gradient"

    def r(dt):
        A_ = _t(A0, dt).requires_grad_(True)
        rx_ = _mix(_t(x, dt), A_)
        q_, h_ = ref.vaenn_net(rx_, _t(g["theta0"], dt), n, k1, k2, sps, M)
        l_ = ref.awgn_loss(q_, rx_, h_, _t(g["amp_levels"], dt), None)
        l_.backward()
        return float(l_.detach()), A_.grad.numpy().astype(np.float64)
    (l64, g64), (l32, g32) = r(torch.float64), r(torch.float32)
    assert abs(float(loss.detach()) - l64) / abs(l64) < LOSS_TOL
    _check("e2e", _h(A.grad), g64, g32, "vaenn")


def test_five_adam_steps_of_the_front_end():
    """Five Adam steps of the IQ compensator alone (frozen Dirac equalizer and channel estimate) on G2's first frame: the loss goes down and
    follows the float64 loop."""
    from vae_equalizer_amd import shared_funcs as sfun
    g = load_golden("G2_dp_freerun")
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    x = g["rx"][:, :, :B * sps]
    A0 = _h(_front(np.random.default_rng(24), True))
    net = sfun.twoXtwoFIR(M, sps).to(DEV).requires_grad_(False)
    W0 = _h(net.conv_w.weight)
    h0 = np.zeros((2, 2, 2, M), np.float32)
    h0[0, 0, 0, M // 2] = h0[1, 1, 0, M // 2] = 1
    amp, P, var = _g(g["amp_levels"]), _g(g["P"]), _g(g["var"])
    A = _g(A0).requires_grad_(True)
    A64 = _t(A0, torch.float64).requires_grad_(True)
    opt, opt64 = torch.optim.Adam([A], lr=5e-3), torch.optim.Adam([A64], lr=5e-3)
    got, want = [], []
    for _ in range(5):
        opt.zero_grad()
        rx = _mix(_g(x), A)
        q, _ = net(rx, amp, var, float(g["nu_sc"]))
        loss, _ = sfun.loss_function_shaping(q, rx, _g(h0), amp, P)
        loss.backward()
        opt.step()
        got.append(float(loss.detach()))
        opt64.zero_grad()
        rx64 = _mix(_t(x, torch.float64), A64)
        q64, _ = ref.dp_forward(rx64, _t(W0, torch.float64), _t(g["amp_levels"], torch.float64), _t(g["var"], torch.float64), float(g["nu_sc"]), sps)
        l64 = ref.dp_loss(q64, rx64, _t(h0, torch.float64), _t(g["amp_levels"], torch.float64), _t(g["P"], torch.float64))[0]
        l64.backward()
        opt64.step()
        want.append(float(l64.detach()))
    print("losses", got, want)
    assert got[-1] < got[0]
    assert np.max(np.abs(np.array(got) - np.array(want)) / np.abs(want)) < LOSS_TOL


def test_every_instantiation_was_reached():
    """Runs last in this file: every instantiation of the five new kernels was launched by some test above."""
    want = {f"vaeq::{k}_kernel<{n}>" for k in ("dp_forward_bwd_x", "dp_loss_bwd_x", "awgn_forward_bwd_x", "awgn_loss_bwd_x") for n in (2, 4, 8)}
    want |= {f"vaeq::nn_enc_backward_x_kernel<512, {n}, {m}>" for n in (2, 4, 8) for m in (0, 1, 2)}
    assert want <= SEEN, sorted(want - SEEN)

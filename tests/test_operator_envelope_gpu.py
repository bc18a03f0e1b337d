"""The drop-in operator kernels (include/vaeq.h: soft demapper, FIR + demapper, ELBO and their backward passes, dual- and single-
polarisation) against the float64 restatement tests/_ref_operators.py, across the whole envelope their ABI accepts:
  - every entry point through the ctypes bindings, backward ones with arbitrary upstream gradients, over a covering shape grid
    (n_lev 2/4/8, sps 1-4, M 1-63, B from its minimum past the dynamic-LDS threshold);
  - the LDS ceiling of every entry point with a dynamic LDS path, from the size formulas written out below;
  - the batched ABI (R = 3, per-run P / var / nu_sc / g_up) against R = 1 calls, bit for bit;
  - numeric edges (one-hot q, exact zeros, near-zero var, N = 1, the grid-stride loop);
  - the autograd wrappers through the mirrors users call, with non-contiguous inputs and ragged input lengths.
Bounds are those the existing tests use against the reference; gq, which had none, gets relerr 1e-4."""
import json
import os

import numpy as np
import pytest
import torch

import _ref_operators as ref
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAEQ_ERR_LDS = -3
TOL = dict(y=2e-6, q=2e-4, loss=1e-5, var_est=1e-5, gh=2e-5, gW_dp=1e-4, gW_awgn=2e-4, gq=1e-4)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("VAEQ_ERROR_REPORT")                 # optional: the largest error of each quantity, for reviews
    if path:
        with open(path, "w") as f:
            json.dump(_WORST, f, indent=1, sort_keys=True)


def _ok(kind, err, ctx=""):
    _WORST[kind] = max(_WORST.get(kind, 0.0), float(err))
    assert np.isfinite(err) and err <= TOL[kind], (kind, err, ctx)


def _rel(a, b):
    return relerr(np.asarray(a), np.asarray(b))


def _maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def _lib():
    from vae_equalizer_amd import _native as nat
    return nat, nat.lib()


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _h(t):
    return t.detach().cpu().numpy()


def _d(a):
    """float32 values as the kernel sees them, in float64 for the reference."""
    return torch.tensor(np.asarray(a, np.float32), dtype=torch.float64)


def _call(fn_name, *args):
    nat, L = _lib()
    rc = getattr(L, fn_name)(*[nat.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], nat.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return int(rc)


def _run(fn_name, *args):
    nat, _ = _lib()
    nat.check(_call(fn_name, *args), fn_name)


# ------------------------------------------------------------------ the entry points' LDS formulas (csrc/vaeq_ops.hip)
LDS = {  # bytes of dynamic LDS for size B (or N), sps, M
    "vaeq_dp_loss": lambda B, sps, M: 4 * (8 * B + 8 * M + 2 * M + 64),
    "vaeq_dp_loss_bwd": lambda B, sps, M: 4 * (8 * B + 4 * (B * sps - 2 * (M // 2)) + 10 * M + 64),
    "vaeq_dp_forward_bwd": lambda N, sps, M: 4 * 4 * N,
    "vaeq_awgn_loss": lambda B, sps, M: 4 * 4 * B,
    "vaeq_awgn_loss_bwd": lambda B, sps, M: 4 * (4 * B + 2 * (B * sps - 2 * (M // 2))),
    "vaeq_awgn_forward_bwd": lambda N, sps, M: 4 * 4 * N,
}
DYN = {"dp": 48 * 1024, "awgn": 32 * 1024}                    # above this the launch raises the dynamic-LDS attribute
CEIL = {"dp": 160 * 1024, "awgn": 150 * 1024}                 # above this the entry point refuses with VAEQ_ERR_LDS


def _largest(fn_name, limit, sps, M):
    f, lo, hi = LDS[fn_name], 1, 1 << 20                       # largest B with f(B) <= limit (f is increasing in B)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if f(mid, sps, M) <= limit else (lo, mid - 1)
    return lo


def test_worked_example_of_the_lds_formula():
    assert LDS["vaeq_dp_loss_bwd"](2546, 2, 25) <= CEIL["dp"] < LDS["vaeq_dp_loss_bwd"](2547, 2, 25)
    assert _largest("vaeq_dp_loss_bwd", CEIL["dp"], 2, 25) == 2546 and _largest("vaeq_dp_loss_bwd", DYN["dp"], 2, 25) == 754


def _size(kind, fn_name, sps, M, minimum):
    fam = "dp" if fn_name.startswith("vaeq_dp") else "awgn"
    return {"min": minimum, "prime": 211, "typical": 500, "below": _largest(fn_name, DYN[fam], sps, M),
            "above": _largest(fn_name, DYN[fam], sps, M) + 1}[kind]


NLEV, SPS, MS, BK = [2, 4, 8], [1, 2, 3, 4], [1, 3, 9, 25, 63], ["min", "prime", "typical", "below", "above"]
GRID = [(NLEV[i % 3], SPS[i % 4], MS[i % 5], BK[(2 * i + i // 5) % 5], i) for i in range(30)]   # every value of every axis, 30 cases


def test_grid_covers_every_axis_value():
    for ax, vals in ((0, NLEV), (1, SPS), (2, MS), (3, BK)):
        assert {c[ax] for c in GRID} == set(vals)
    assert {(c[2], c[3]) for c in GRID} == {(m, b) for m in MS for b in BK}


# ------------------------------------------------------------------ data
def _levels(n):
    return (np.arange(-(n - 1), n, 2) / np.sqrt((n * n - 1) / 3.0 * 2)).astype(np.float32)


def _prior(rng, n):
    p = rng.uniform(0.2, 1.0, n)
    p = (p + p[::-1]) / 2
    return (p / p.sum()).astype(np.float32)


def _q(rng, lead, n, B, zeros=False):
    z = 2.0 * rng.standard_normal((*lead, n, B))
    q = np.exp(z - z.max(-2, keepdims=True))
    q /= q.sum(-2, keepdims=True)
    if zeros:                                                  # one-hot symbols and exact zeros: the +1e-12 branch of the KL gradient
        q[..., 0, 1::3] = 0.0
        q /= q.sum(-2, keepdims=True)
        hot = rng.integers(0, n, (*lead, B))
        oh = (np.arange(n)[:, None] == hot[..., None, :]).astype(np.float64)
        q = np.where(rng.random((*lead, 1, B)) < 0.5, oh, q)
    return q.reshape(*lead[:-1], lead[-1] * n, B).astype(np.float32)


def _taps(rng, shape, M, dirac):
    W = (0.3 * rng.standard_normal(shape) / np.sqrt(M)).astype(np.float32)
    for idx in dirac:
        W[idx + (M // 2,)] += 1.0
    return W


# ------------------------------------------------------------------ dual polarisation: soft_demap / dp_forward / dp_forward_bwd
def _dp_fwd_case(rng, n, sps, M, N, gy_null):
    x = (0.5 * rng.standard_normal((1, 2, 2, N * sps))).astype(np.float32)
    W = _taps(rng, (1, 2, 4, M), M, [(0, 0, 0), (0, 1, 1)])
    amp, var, nu = _levels(n), rng.uniform(0.01, 0.05, (1, 2)).astype(np.float32), rng.uniform(0, 1, 1).astype(np.float32)
    q, y = torch.empty(1, 2, 2 * n, N, device=DEV), torch.empty(1, 2, 2, N, device=DEV)
    xg, Wg, ag, vg, ng = _g(x), _g(W), _g(amp), _g(var), _g(nu)
    _run("vaeq_dp_forward", 1, N, sps, M, n, xg, Wg, ag, vg, ng, q, y)
    W64 = _d(W[0]).requires_grad_(True)
    qr, yr = ref.dp_forward(_d(x[0]), W64, _d(amp), _d(var[0]), float(nu[0]), sps)
    ctx = (n, sps, M, N)
    _ok("y", _rel(_h(y)[0], _h(yr)), ctx)
    _ok("q", _maxabs(_h(q)[0], _h(qr)), ctx)
    qs = torch.empty_like(q)
    _run("vaeq_soft_demap", 1, N, n, y, ag, vg, ng, qs)
    _ok("q", _maxabs(_h(qs)[0], _h(ref.soft_dec(_d(_h(y)[0]), _d(var[0]), _d(amp), float(nu[0])))), ctx)
    gq = rng.standard_normal((1, 2, 2 * n, N)).astype(np.float32)
    gy = None if gy_null else rng.standard_normal((1, 2, 2, N)).astype(np.float32)
    gW = torch.empty(1, 2, 4, M, device=DEV)
    _run("vaeq_dp_forward_bwd", 1, N, sps, M, n, xg, q, y, _g(gq), None if gy is None else _g(gy), ag, vg, gW)
    obj = (qr * _d(gq[0])).sum() + (0 if gy is None else (yr * _d(gy[0])).sum())
    (gWr,) = torch.autograd.grad(obj, (W64,))
    _ok("gW_dp", _rel(_h(gW)[0], _h(gWr)), ctx)


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_dp_forward_demap_and_forward_bwd_grid(n, sps, M, kind, i):
    N = _size(kind, "vaeq_dp_forward_bwd", sps, M, 1)
    _dp_fwd_case(np.random.default_rng(1000 + i), n, sps, M, N, gy_null=bool(i % 2))


# ------------------------------------------------------------------ dual polarisation: dp_loss / dp_loss_bwd
def _dp_loss_case(rng, n, sps, M, B, zeros=False, which=("vaeq_dp_loss", "vaeq_dp_loss_bwd")):
    q = _q(rng, (2, 2), n, B, zeros)
    x = rng.standard_normal((2, 2, B * sps)).astype(np.float32)
    h = (0.3 * rng.standard_normal((2, 2, 2, M))).astype(np.float32)
    amp, P = _levels(n), _prior(rng, n)
    up = np.float32(rng.choice([-2.3, 0.37, 3.1]))
    q64, h64 = _d(q).requires_grad_(True), _d(h).requires_grad_(True)
    lr_, ver = ref.dp_loss(q64, _d(x), h64, _d(amp), _d(P))
    ctx = (n, sps, M, B, zeros)
    args = (_g(q[None]), _g(x[None]), _g(h[None]), _g(amp), _g(P[None]))
    if "vaeq_dp_loss" in which:
        loss, ve = torch.empty(1, device=DEV), torch.empty(1, 2, device=DEV)
        _run("vaeq_dp_loss", 1, B, sps, M, n, *args, loss, ve)
        _ok("loss", abs(float(_h(loss)[0]) - float(lr_.detach())) / abs(float(lr_.detach())), ctx)
        _ok("var_est", _rel(_h(ve)[0], _h(ver)), ctx)
    if "vaeq_dp_loss_bwd" in which:
        gq, gh = torch.empty(1, 2, 2 * n, B, device=DEV), torch.empty(1, 2, 2, 2, M, device=DEV)
        _run("vaeq_dp_loss_bwd", 1, B, sps, M, n, *args, _g(np.array([up])), gq, gh)
        gqr, ghr = torch.autograd.grad(float(up) * lr_, (q64, h64))
        assert torch.isfinite(gq).all() and torch.isfinite(gh).all()
        _ok("gq", _rel(_h(gq)[0], _h(gqr)), ctx)
        _ok("gh", _rel(_h(gh)[0], _h(ghr)), ctx)


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_dp_loss_grid(n, sps, M, kind, i):
    _dp_loss_case(np.random.default_rng(2000 + i), n, sps, M, _size(kind, "vaeq_dp_loss", sps, M, M), which=("vaeq_dp_loss",))


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_dp_loss_bwd_grid(n, sps, M, kind, i):
    _dp_loss_case(np.random.default_rng(3000 + i), n, sps, M, _size(kind, "vaeq_dp_loss_bwd", sps, M, M), which=("vaeq_dp_loss_bwd",))


# ------------------------------------------------------------------ single polarisation: awgn_forward / awgn_forward_bwd
def _awgn_fwd_case(rng, n, sps, M, N, gy_null):
    x = (0.5 * rng.standard_normal((1, 2, N * sps))).astype(np.float32)
    W = _taps(rng, (1, 2, M), M, [(0, 0)])
    amp = _levels(n)
    am, var = np.array([np.mean(np.abs(amp))], np.float32), rng.uniform(0.02, 0.1, 1).astype(np.float32)
    q, y = torch.empty(1, 2 * n, N, device=DEV), torch.empty(1, 2, N, device=DEV)
    xg, Wg, ag, amg, vg = _g(x), _g(W), _g(amp), _g(am), _g(var)
    _run("vaeq_awgn_forward", 1, N, sps, M, n, xg, Wg, ag, amg, vg, q, y)
    W64 = _d(W).requires_grad_(True)
    qr, yr = ref.awgn_forward(_d(x[0]), W64, _d(amp), float(am[0]), float(var[0]), sps)
    ctx = (n, sps, M, N)
    _ok("y", _rel(_h(y)[0], _h(yr)), ctx)
    _ok("q", _maxabs(_h(q)[0], _h(qr)), ctx)
    gq = rng.standard_normal((1, 2 * n, N)).astype(np.float32)
    gy = None if gy_null else rng.standard_normal((1, 2, N)).astype(np.float32)
    gW = torch.empty(1, 2, M, device=DEV)
    _run("vaeq_awgn_forward_bwd", 1, N, sps, M, n, xg, Wg, ag, amg, vg, _g(gq), None if gy is None else _g(gy), gW)
    obj = (qr * _d(gq[0])).sum() + (0 if gy is None else (yr * _d(gy[0])).sum())
    (gWr,) = torch.autograd.grad(obj, (W64,))
    _ok("gW_awgn", _rel(_h(gW), _h(gWr)), ctx)


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_awgn_forward_and_forward_bwd_grid(n, sps, M, kind, i):
    N = _size(kind, "vaeq_awgn_forward_bwd", sps, M, 1)
    # at N = 1 the normalisation (:228) maps y to +-amp_mean: q does not depend on W and dL/dW through q is exactly 0, so the kernel's
    # rounding residue (~1e-8) has nothing to be relative to.  The N = 1 cases therefore always carry an upstream gy.
    _awgn_fwd_case(np.random.default_rng(4000 + i), n, sps, M, N, gy_null=bool(i % 2) and N > 1)


# ------------------------------------------------------------------ single polarisation: awgn_loss / awgn_loss_bwd (P, or NULL = VAE-NN)
def _awgn_loss_case(rng, n, sps, M, B, with_P, zeros=False, which=("vaeq_awgn_loss", "vaeq_awgn_loss_bwd")):
    q = _q(rng, (2,), n, B, zeros)
    # a loud x keeps nm log C above the entropy term of the P = NULL form (|sum q log q| <= 2 log n per symbol): at B = M = 1 a
    # unit-power x lets the two cancel, and a relative bound on a near-zero loss measures the cancellation, not the kernel
    x = (10.0 * rng.standard_normal((2, B * sps))).astype(np.float32)
    h = (0.3 * rng.standard_normal((2, M))).astype(np.float32)
    amp, P = _levels(n), (_prior(rng, n) if with_P else None)
    up = np.float32(rng.choice([-2.3, 0.37, 3.1]))
    q64, h64 = _d(q).requires_grad_(True), _d(h).requires_grad_(True)
    lr_ = ref.awgn_loss(q64, _d(x), h64, _d(amp), None if P is None else _d(P))
    ctx = (n, sps, M, B, with_P, zeros)
    args = (_g(q[None]), _g(x[None]), _g(h[None]), _g(amp), None if P is None else _g(P[None]))
    if "vaeq_awgn_loss" in which:
        loss = torch.empty(1, device=DEV)
        _run("vaeq_awgn_loss", 1, B, sps, M, n, *args, loss)
        _ok("loss", abs(float(_h(loss)[0]) - float(lr_.detach())) / abs(float(lr_.detach())), ctx)
    if "vaeq_awgn_loss_bwd" in which:
        gq, gh = torch.empty(1, 2 * n, B, device=DEV), torch.empty(1, 2, M, device=DEV)
        _run("vaeq_awgn_loss_bwd", 1, B, sps, M, n, *args, _g(np.array([up])), gq, gh)
        gqr, ghr = torch.autograd.grad(float(up) * lr_, (q64, h64))
        assert torch.isfinite(gq).all() and torch.isfinite(gh).all()
        _ok("gq", _rel(_h(gq)[0], _h(gqr)), ctx)
        _ok("gh", _rel(_h(gh)[0], _h(ghr)), ctx)


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_awgn_loss_grid(n, sps, M, kind, i):
    _awgn_loss_case(np.random.default_rng(5000 + i), n, sps, M, _size(kind, "vaeq_awgn_loss", sps, M, M), bool(i % 2),
                    which=("vaeq_awgn_loss",))


@pytest.mark.parametrize("n,sps,M,kind,i", GRID)
def test_awgn_loss_bwd_grid(n, sps, M, kind, i):
    _awgn_loss_case(np.random.default_rng(6000 + i), n, sps, M, _size(kind, "vaeq_awgn_loss_bwd", sps, M, M), bool(i % 2),
                    which=("vaeq_awgn_loss_bwd",))


# ------------------------------------------------------------------ the LDS ceiling
CEILING = ["vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_dp_forward_bwd", "vaeq_awgn_loss", "vaeq_awgn_loss_bwd", "vaeq_awgn_forward_bwd"]


@pytest.mark.parametrize("fn_name", CEILING)
def test_lds_ceiling(fn_name):
    """The largest size the entry point's own formula admits runs (with every byte of the 160 KiB / 150 KiB) and matches the reference;
    one more is refused with VAEQ_ERR_LDS before anything is launched."""
    nat, _ = _lib()
    sps, M, n = 2, 25, 8
    fam = "dp" if fn_name.startswith("vaeq_dp") else "awgn"
    top = _largest(fn_name, CEIL[fam], sps, M)
    assert LDS[fn_name](top, sps, M) > DYN[fam] and LDS[fn_name](top + 1, sps, M) > CEIL[fam]
    rng = np.random.default_rng(7000 + CEILING.index(fn_name))
    if fn_name == "vaeq_dp_forward_bwd":
        _dp_fwd_case(rng, n, sps, M, top, gy_null=False)
    elif fn_name == "vaeq_awgn_forward_bwd":
        _awgn_fwd_case(rng, n, sps, M, top, gy_null=False)
    elif fam == "dp":
        _dp_loss_case(rng, n, sps, M, top, which=(fn_name,))
    else:
        _awgn_loss_case(rng, n, sps, M, top, True, which=(fn_name,))
    B = top + 1                                                # refused: buffers sized for B anyway, nothing may touch them
    e = lambda *s: torch.zeros(*s, device=DEV)
    if fn_name == "vaeq_dp_loss":
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2, 2 * n, B), e(1, 2, 2, B * sps), e(1, 2, 2, 2, M), e(n), e(1, n), e(1), e(1, 2))
    elif fn_name == "vaeq_dp_loss_bwd":
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2, 2 * n, B), e(1, 2, 2, B * sps), e(1, 2, 2, 2, M), e(n), e(1, n), e(1),
                   e(1, 2, 2 * n, B), e(1, 2, 2, 2, M))
    elif fn_name == "vaeq_dp_forward_bwd":
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2, 2, B * sps), e(1, 2, 2 * n, B), e(1, 2, 2, B), e(1, 2, 2 * n, B), None, e(n), e(1, 2),
                   e(1, 2, 4, M))
    elif fn_name == "vaeq_awgn_loss":
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2 * n, B), e(1, 2, B * sps), e(1, 2, M), e(n), e(1, n), e(1))
    elif fn_name == "vaeq_awgn_loss_bwd":
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2 * n, B), e(1, 2, B * sps), e(1, 2, M), e(n), e(1, n), e(1), e(1, 2 * n, B), e(1, 2, M))
    else:
        rc = _call(fn_name, 1, B, sps, M, n, e(1, 2, B * sps), e(1, 2, M), e(n), e(1), e(1), e(1, 2 * n, B), None, e(1, 2, M))
    assert rc == VAEQ_ERR_LDS
    with pytest.raises(nat.VaeqError):
        nat.check(rc, fn_name)


# ------------------------------------------------------------------ the batched ABI
HEAVY = load_golden("G1_dp_step_64qam_nu1222")                # config 5's heavy shaping: nu = 0.1222 (Eval_run_DP.py:24)


def _runs():
    amp = HEAVY["amp_levels"].astype(np.float32)
    P = np.stack([np.full(8, 1 / 8), _prior(np.random.default_rng(5), 8), HEAVY["P"]]).astype(np.float32)
    var = np.array([[0.02, 0.03], [0.0025, 0.004], list(HEAVY["var"])], np.float32)
    nu = np.array([0.0, 0.8724, float(HEAVY["nu_sc"])], np.float32)
    up = np.array([1.0, -0.7, 2.9], np.float32)
    return amp, P, var, nu, up


def _rows(t, r):
    return t[r:r + 1].contiguous()


def test_dp_batched_abi_per_run_parameters():
    rng = np.random.default_rng(11)
    amp, P, var, nu, up = _runs()
    R, n, sps, M, B = 3, 8, 2, 13, 128
    sym = rng.choice(amp, (R, 2, 2, B))
    x = np.repeat(sym, sps, -1) + rng.standard_normal((R, 2, 2, B * sps)) * np.sqrt(var)[:, :, None, None]
    x = x.astype(np.float32)
    W = np.concatenate([_taps(rng, (1, 2, 4, M), M, [(0, 0, 0), (0, 1, 1)]) for _ in range(R)])
    W = (np.round(W) + 0.01 * (W - np.round(W))).astype(np.float32)   # near-Dirac taps: the heavy run keeps a readable constellation
    h = (0.3 * rng.standard_normal((R, 2, 2, 2, M))).astype(np.float32)
    gq_up = rng.standard_normal((R, 2, 2 * n, B)).astype(np.float32)
    gy_up = rng.standard_normal((R, 2, 2, B)).astype(np.float32)
    xg, Wg, hg, ag, Pg, vg, ng, ug = _g(x), _g(W), _g(h), _g(amp), _g(P), _g(var), _g(nu), _g(up)
    e = lambda *s: torch.empty(*s, device=DEV)

    def launch(sel):
        o = dict(q=e(len(sel), 2, 2 * n, B), y=e(len(sel), 2, 2, B), qs=e(len(sel), 2, 2 * n, B), loss=e(len(sel)), ve=e(len(sel), 2),
                 gq=e(len(sel), 2, 2 * n, B), gh=e(len(sel), 2, 2, 2, M), gW=e(len(sel), 2, 4, M))
        k = len(sel)
        X, Wt, Ht, Pt, Vt, Nt, Ut = (sel(t) for t in (xg, Wg, hg, Pg, vg, ng, ug))
        _run("vaeq_dp_forward", k, B, sps, M, n, X, Wt, ag, Vt, Nt, o["q"], o["y"])
        _run("vaeq_soft_demap", k, B, n, o["y"], ag, Vt, Nt, o["qs"])
        _run("vaeq_dp_loss", k, B, sps, M, n, o["q"], X, Ht, ag, Pt, o["loss"], o["ve"])
        _run("vaeq_dp_loss_bwd", k, B, sps, M, n, o["q"], X, Ht, ag, Pt, Ut, o["gq"], o["gh"])
        _run("vaeq_dp_forward_bwd", k, B, sps, M, n, X, o["q"], o["y"], sel(_g(gq_up)), sel(_g(gy_up)), ag, Vt, o["gW"])
        return o

    class _All:
        def __call__(self, t):
            return t

        def __len__(self):
            return R

    full = launch(_All())
    for r in range(R):
        class _One:
            def __call__(self, t):
                return _rows(t, r)

            def __len__(self):
                return 1

        one = launch(_One())
        for k in full:
            assert torch.equal(full[k][r:r + 1], one[k]), (r, k)       # run r of the batch == run r alone, bit for bit
        W64, h64 = _d(W[r]).requires_grad_(True), _d(h[r]).requires_grad_(True)
        qr, yr = ref.dp_forward(_d(x[r]), W64, _d(amp), _d(var[r]), float(nu[r]), sps)
        ctx = ("run", r)
        _ok("y", _rel(_h(full["y"])[r], _h(yr)), ctx)
        _ok("q", _maxabs(_h(full["q"])[r], _h(qr)), ctx)
        _ok("q", _maxabs(_h(full["qs"])[r], _h(ref.soft_dec(_d(_h(full["y"])[r]), _d(var[r]), _d(amp), float(nu[r])))), ctx)
        q64 = _d(_h(full["q"])[r]).requires_grad_(True)
        lr_, ver = ref.dp_loss(q64, _d(x[r]), h64, _d(amp), _d(P[r]))
        _ok("loss", abs(float(_h(full["loss"])[r]) - float(lr_.detach())) / abs(float(lr_.detach())), ctx)
        _ok("var_est", _rel(_h(full["ve"])[r], _h(ver)), ctx)
        gqr, ghr = torch.autograd.grad(float(up[r]) * lr_, (q64, h64))
        _ok("gq", _rel(_h(full["gq"])[r], _h(gqr)), ctx)
        _ok("gh", _rel(_h(full["gh"])[r], _h(ghr)), ctx)
        (gWr,) = torch.autograd.grad((qr * _d(gq_up[r])).sum() + (yr * _d(gy_up[r])).sum(), (W64,))
        _ok("gW_dp", _rel(_h(full["gW"])[r], _h(gWr)), ctx)


def test_awgn_batched_abi_per_run_parameters():
    rng = np.random.default_rng(12)
    amp, P, var, nu, up = _runs()
    R, n, sps, M, B = 3, 8, 2, 13, 128
    am = np.array([np.mean(np.abs(amp))] * 2 + [float(np.sum(HEAVY["P"] * np.abs(amp)))], np.float32)
    va = np.array([0.05, 0.01, 0.004], np.float32)
    x = (np.repeat(rng.choice(amp, (R, 2, B)), sps, -1) + 0.05 * rng.standard_normal((R, 2, B * sps))).astype(np.float32)
    W = np.concatenate([_taps(rng, (1, 2, M), M, [(0, 0)]) for _ in range(R)])
    h = (0.3 * rng.standard_normal((R, 2, M))).astype(np.float32)
    gq_up = rng.standard_normal((R, 2 * n, B)).astype(np.float32)
    gy_up = rng.standard_normal((R, 2, B)).astype(np.float32)
    xg, Wg, hg, ag, Pg, amg, vg, ug = _g(x), _g(W), _g(h), _g(amp), _g(P), _g(am), _g(va), _g(up)
    e = lambda *s: torch.empty(*s, device=DEV)

    def launch(sl):
        k = sl.stop - sl.start
        X, Wt, Ht, Pt, At, Vt, Ut = (t[sl].contiguous() for t in (xg, Wg, hg, Pg, amg, vg, ug))
        o = dict(q=e(k, 2 * n, B), y=e(k, 2, B), loss=e(k), lossnn=e(k), gq=e(k, 2 * n, B), gh=e(k, 2, M), gqnn=e(k, 2 * n, B),
                 ghnn=e(k, 2, M), gW=e(k, 2, M))
        _run("vaeq_awgn_forward", k, B, sps, M, n, X, Wt, ag, At, Vt, o["q"], o["y"])
        _run("vaeq_awgn_loss", k, B, sps, M, n, o["q"], X, Ht, ag, Pt, o["loss"])
        _run("vaeq_awgn_loss", k, B, sps, M, n, o["q"], X, Ht, ag, None, o["lossnn"])
        _run("vaeq_awgn_loss_bwd", k, B, sps, M, n, o["q"], X, Ht, ag, Pt, Ut, o["gq"], o["gh"])
        _run("vaeq_awgn_loss_bwd", k, B, sps, M, n, o["q"], X, Ht, ag, None, Ut, o["gqnn"], o["ghnn"])
        _run("vaeq_awgn_forward_bwd", k, B, sps, M, n, X, Wt, ag, At, Vt, _g(gq_up)[sl].contiguous(), _g(gy_up)[sl].contiguous(), o["gW"])
        return o

    full = launch(slice(0, R))
    for r in range(R):
        one = launch(slice(r, r + 1))
        for k in full:
            assert torch.equal(full[k][r:r + 1], one[k]), (r, k)
        W64, h64 = _d(W[r:r + 1]).requires_grad_(True), _d(h[r]).requires_grad_(True)
        qr, yr = ref.awgn_forward(_d(x[r]), W64, _d(amp), float(am[r]), float(va[r]), sps)
        ctx = ("run", r)
        _ok("y", _rel(_h(full["y"])[r], _h(yr)), ctx)
        _ok("q", _maxabs(_h(full["q"])[r], _h(qr)), ctx)
        for Pr, lk, gqk, ghk in ((_d(P[r]), "loss", "gq", "gh"), (None, "lossnn", "gqnn", "ghnn")):
            q64 = _d(_h(full["q"])[r]).requires_grad_(True)
            lr_ = ref.awgn_loss(q64, _d(x[r]), h64, _d(amp), Pr)
            _ok("loss", abs(float(_h(full[lk])[r]) - float(lr_.detach())) / abs(float(lr_.detach())), ctx)
            gqr, ghr = torch.autograd.grad(float(up[r]) * lr_, (q64, h64))
            _ok("gq", _rel(_h(full[gqk])[r], _h(gqr)), ctx)
            _ok("gh", _rel(_h(full[ghk])[r], _h(ghr)), ctx)
        (gWr,) = torch.autograd.grad((qr * _d(gq_up[r])).sum() + (yr * _d(gy_up[r])).sum(), (W64,))
        _ok("gW_awgn", _rel(_h(full["gW"])[r], _h(gWr)), ctx)


# ------------------------------------------------------------------ numeric edges
@pytest.mark.parametrize("n,sps,M", [(2, 1, 1), (4, 2, 9), (8, 3, 25)])
def test_one_hot_and_exact_zero_q(n, sps, M):
    rng = np.random.default_rng(13 + n)
    _dp_loss_case(rng, n, sps, M, 97, zeros=True)
    _awgn_loss_case(rng, n, sps, M, 97, True, zeros=True)
    _awgn_loss_case(rng, n, sps, M, 97, False, zeros=True)


def test_soft_demap_near_zero_var():
    rng = np.random.default_rng(14)
    n, N = 8, 4096
    amp = _levels(n)
    y = (rng.choice(amp, (1, 2, 2, N)) + 0.02 * rng.standard_normal((1, 2, 2, N))).astype(np.float32)
    var, nu = np.array([[1e-6, 3e-6]], np.float32), np.array([0.5], np.float32)
    q = torch.empty(1, 2, 2 * n, N, device=DEV)
    _run("vaeq_soft_demap", 1, N, n, _g(y), _g(amp), _g(var), _g(nu), q)
    assert torch.isfinite(q).all()
    _ok("q", _maxabs(_h(q)[0], _h(ref.soft_dec(_d(y[0]), _d(var[0]), _d(amp), float(nu[0])))), "var 1e-6")


@pytest.mark.parametrize("N", [1, 4096 * 256 + 37])
def test_soft_demap_and_dp_forward_at_n1_and_past_the_grid_stride(N):
    """The grids are capped at 4096 blocks of 256 threads: past 4096 * 256 symbols the kernels loop."""
    rng = np.random.default_rng(15)
    n, sps, M = 2, 2, 9
    amp = _levels(n)
    var, nu = np.array([[0.02, 0.03]], np.float32), np.array([0.3], np.float32)
    x = (0.5 * rng.standard_normal((1, 2, 2, N * sps))).astype(np.float32)
    W = _taps(rng, (1, 2, 4, M), M, [(0, 0, 0), (0, 1, 1)])
    q, y, qs = torch.empty(1, 2, 2 * n, N, device=DEV), torch.empty(1, 2, 2, N, device=DEV), torch.empty(1, 2, 2 * n, N, device=DEV)
    _run("vaeq_dp_forward", 1, N, sps, M, n, _g(x), _g(W), _g(amp), _g(var), _g(nu), q, y)
    _run("vaeq_soft_demap", 1, N, n, y, _g(amp), _g(var), _g(nu), qs)
    with torch.no_grad():
        qr, yr = ref.dp_forward(_d(x[0]), _d(W[0]), _d(amp), _d(var[0]), float(nu[0]), sps)
        qsr = ref.soft_dec(_d(_h(y)[0]), _d(var[0]), _d(amp), float(nu[0]))
    _ok("y", _rel(_h(y)[0], yr.numpy()), N)
    _ok("q", _maxabs(_h(q)[0], qr.numpy()), N)
    _ok("q", _maxabs(_h(qs)[0], qsr.numpy()), N)


# ------------------------------------------------------------------ the autograd wrappers through the mirrors
def _nc(t):
    """Same values and shape, dense but not contiguous (a permuted layout)."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def _leaf(a, nc):
    t = _g(a)
    return (_nc(t) if nc else t).detach().requires_grad_(True)


COMBOS = [(False, False, False, False), (True, False, False, False), (False, True, False, False), (True, True, False, False),
          (False, False, True, True), (True, True, True, True)]   # (q, h, x, W) non-contiguous; (True, True, ...) = the aliasing case


def _dp_mirror_grads(g, nc_q, nc_h, nc_x, nc_W):
    from vae_equalizer_amd import shared_funcs as sfun
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    net = sfun.twoXtwoFIR(M, sps).to(DEV)
    net.conv_w.weight = torch.nn.Parameter(_nc(_g(g["W0"])) if nc_W else _g(g["W0"]))
    assert net.conv_w.weight.is_contiguous() != nc_W
    h = _leaf(g["h0"], nc_h)
    x = _g(g["rx"][:, :, :B * sps])
    x = _nc(x) if nc_x else x
    amp, P, var = (_g(g[k]) for k in ("amp_levels", "P", "var"))
    q, out = net(x, amp, var, float(g["nu_sc"]))
    loss, _ = sfun.loss_function_shaping(_nc(q) if nc_q else q, x, h, amp, P)
    ((3.7 * loss) + (loss + loss)).backward()
    return net.conv_w.weight.grad.clone(), h.grad.clone()


def test_dp_mirrors_with_non_contiguous_inputs():
    g = load_golden("G1_dp_step_16qam")
    B, sps = int(g["B"]), int(g["sps"])
    gW0, gh0 = _dp_mirror_grads(g, *COMBOS[0])
    W64, h64 = _d(g["W0"]).requires_grad_(True), _d(g["h0"]).requires_grad_(True)
    x64 = _d(g["rx"][:, :, :B * sps])
    qr, _ = ref.dp_forward(x64, W64, _d(g["amp_levels"]), _d(g["var"]), float(g["nu_sc"]), sps)
    lr_, _ = ref.dp_loss(qr, x64, h64, _d(g["amp_levels"]), _d(g["P"]))
    gWr, ghr = torch.autograd.grad(5.7 * lr_, (W64, h64))
    _ok("gW_dp", _rel(_h(gW0), _h(gWr)), "mirror")
    _ok("gh", _rel(_h(gh0), _h(ghr)), "mirror")
    for combo in COMBOS[1:]:
        gW, gh = _dp_mirror_grads(g, *combo)
        assert torch.equal(gW, gW0) and torch.equal(gh, gh0), combo


def _awgn_mirror_grads(g, nc_q, nc_h, nc_x, nc_W, vaenn):
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw
    from vae_equalizer_amd import func_VAENN_MQAM as nn_
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    net = aw.twoFIR(M, sps).to(DEV)
    net.conv_w.weight = torch.nn.Parameter(_nc(_g(g["W0"]).reshape(1, 2, M)) if nc_W else _g(g["W0"]).reshape(1, 2, M))
    h = _leaf(g["h0"], nc_h)
    x = _g(g["rx"][:, :B * sps])
    x = _nc(x) if nc_x else x
    amp, P = _g(g["amp_levels"]), _g(g["P"])
    q, out = net(x, amp, float(g["amp_mean"]), float(g["var"]))
    qq = _nc(q) if nc_q else q
    loss = nn_.loss_function(qq, x, h, DEV, amp) if vaenn else aw.loss_function(qq, x, h, DEV, amp, P)
    ((3.7 * loss) + (loss + loss)).backward()
    return net.conv_w.weight.grad.clone(), h.grad.clone()


@pytest.mark.parametrize("vaenn", [False, True])
def test_awgn_mirrors_with_non_contiguous_inputs(vaenn):
    g = load_golden("G4_awgn_16qam_cfg1")
    B, sps = int(g["B"]), int(g["sps"])
    gW0, gh0 = _awgn_mirror_grads(g, *COMBOS[0], vaenn)
    W64, h64 = _d(g["W0"]).requires_grad_(True), _d(g["h0"]).requires_grad_(True)
    x64 = _d(g["rx"][:, :B * sps])
    qr, _ = ref.awgn_forward(x64, W64, _d(g["amp_levels"]), float(g["amp_mean"]), float(g["var"]), sps)
    lr_ = ref.awgn_loss(qr, x64, h64, _d(g["amp_levels"]), None if vaenn else _d(g["P"]))
    gWr, ghr = torch.autograd.grad(5.7 * lr_, (W64, h64))
    _ok("gW_awgn", _rel(_h(gW0), _h(gWr)), ("mirror", vaenn))
    _ok("gh", _rel(_h(gh0), _h(ghr)), ("mirror", vaenn))
    for combo in COMBOS[1:]:
        gW, gh = _awgn_mirror_grads(g, *combo, vaenn)
        assert torch.equal(gW, gW0) and torch.equal(gh, gh0), combo


def test_vaenn_loss_with_non_contiguous_q_and_h():
    """func_VAENN_MQAM.loss_function on q from the encoder: both leaves permuted (the aliasing case) == contiguous, bit for bit."""
    from vae_equalizer_amd import func_VAENN_MQAM as nn_
    g = load_golden("G8_vaenn_16qam_small")
    B, sps, M = int(g["B"]), int(g["sps"]), int(g["M_est"])
    x = _g(g["rx"][:, :B * sps])
    amp = _g(g["amp_levels"])
    h0 = g["theta0"][-2 * M:].reshape(2, M)
    res = []
    for nc in (False, True):
        q, h = _leaf(g["q0"], nc), _leaf(h0, nc)
        loss = nn_.loss_function(q, x, h, DEV, amp)
        ((3.7 * loss) + (loss + loss)).backward()
        res.append((q.grad.contiguous(), h.grad.contiguous()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    q64, h64 = _d(g["q0"]).requires_grad_(True), _d(h0).requires_grad_(True)
    gqr, ghr = torch.autograd.grad(5.7 * ref.awgn_loss(q64, _d(g["rx"][:, :B * sps]), h64, _d(g["amp_levels"]), None), (q64, h64))
    _ok("gq", _rel(_h(res[1][0]), _h(gqr)), "vaenn mirror")
    _ok("gh", _rel(_h(res[1][1]), _h(ghr)), "vaenn mirror")


# ------------------------------------------------------------------ ragged input length
@pytest.mark.parametrize("sps,L", [(2, 201), (3, 301), (4, 402)])
def test_ragged_length_dp_mirror(sps, L):
    """Conv1d(padding=M//2, stride=sps) yields ceil(L/sps) outputs; the mirror must too, with the values and W.grad of the reference."""
    from vae_equalizer_amd import shared_funcs as sfun
    rng = np.random.default_rng(16 + sps)
    n, M = 4, 9
    amp, var, nu = _levels(n), np.array([0.02, 0.03], np.float32), 0.4
    x = (0.5 * rng.standard_normal((2, 2, L))).astype(np.float32)
    W = _taps(rng, (2, 4, M), M, [(0, 0), (1, 1)])
    net = sfun.twoXtwoFIR(M, sps).to(DEV)
    with torch.no_grad():
        net.conv_w.weight.copy_(_g(W))
    N = -(-L // sps)
    with torch.no_grad():
        qe, ye = net(_g(x), _g(amp), _g(var), nu)
    q, y = net(_g(x), _g(amp), _g(var), nu)
    assert q.shape[-1] == N and y.shape[-1] == N and qe.shape[-1] == N
    W64 = _d(W).requires_grad_(True)
    qr, yr = ref.dp_forward(_d(x), W64, _d(amp), _d(var), nu, sps)
    assert qr.shape[-1] == N
    for qq, yy in ((q, y), (qe, ye)):
        _ok("y", _rel(_h(yy), _h(yr)), ("ragged", sps, L))
        _ok("q", _maxabs(_h(qq), _h(qr)), ("ragged", sps, L))
    gq = rng.standard_normal((2, 2 * n, N)).astype(np.float32)
    gy = rng.standard_normal((2, 2, N)).astype(np.float32)
    ((q * _g(gq)).sum() + (y * _g(gy)).sum()).backward()
    (gWr,) = torch.autograd.grad((qr * _d(gq)).sum() + (yr * _d(gy)).sum(), (W64,))
    _ok("gW_dp", _rel(_h(net.conv_w.weight.grad), _h(gWr)), ("ragged", sps, L))


@pytest.mark.parametrize("sps,L", [(2, 201), (3, 301), (4, 402)])
def test_ragged_length_awgn_mirror(sps, L):
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw
    rng = np.random.default_rng(17 + sps)
    n, M = 4, 9
    amp = _levels(n)
    am, var = float(np.mean(np.abs(amp))), 0.05
    x = (0.5 * rng.standard_normal((2, L))).astype(np.float32)
    W = _taps(rng, (1, 2, M), M, [(0, 0)])
    net = aw.twoFIR(M, sps).to(DEV)
    with torch.no_grad():
        net.conv_w.weight.copy_(_g(W))
    N = -(-L // sps)
    with torch.no_grad():
        qe, ye = net(_g(x), _g(amp), am, var)
    q, y = net(_g(x), _g(amp), am, var)
    assert q.shape[-1] == N and y.shape[-1] == N and qe.shape[-1] == N
    W64 = _d(W).requires_grad_(True)
    qr, yr = ref.awgn_forward(_d(x), W64, _d(amp), am, var, sps)
    for qq, yy in ((q, y), (qe, ye)):
        _ok("y", _rel(_h(yy), _h(yr)), ("ragged", sps, L))
        _ok("q", _maxabs(_h(qq), _h(qr)), ("ragged", sps, L))
    gq = rng.standard_normal((2 * n, N)).astype(np.float32)
    gy = rng.standard_normal((2, N)).astype(np.float32)
    ((q * _g(gq)).sum() + (y * _g(gy)).sum()).backward()
    (gWr,) = torch.autograd.grad((qr * _d(gq)).sum() + (yr * _d(gy)).sum(), (W64,))
    _ok("gW_awgn", _rel(_h(net.conv_w.weight.grad), _h(gWr)), ("ragged", sps, L))

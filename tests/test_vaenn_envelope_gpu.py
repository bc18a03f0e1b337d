"""vaeq_nn_train / vaeq_nn_forward / vaeq_nn_validate over their whole envelope, against the float64 restatement of tests/_ref_vaenn.py:
every n_lev, `Net` and `Net_BN`, 1 to 8 samples per symbol, tap counts 1 to 63, ragged minibatches on both sides of BatchNorm's 640-sample
register rows, the sweep shapes (BK = 1 / 2) and the LDS ceiling, free AMSGrad steps with per-run step sizes, the state invariants of a
call, eval forward across tile boundaries with random running statistics, the fused validation pass, and the dispatch edges.

Tolerances follow the float32 C oracle: the kernel's error against float64 may be a small multiple of the oracle's own, with an absolute
floor.  The largest error of each quantity and its ratio to the oracle's is printed at the end of the module (-s)."""
import numpy as np
import pytest
import torch

import oracle
import _ref_vaenn as ref
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = {}
SEEN = set()
FACTOR = 4.0


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


def _train_name(n, bn, sps, bk=0, nt=512):
    return f"vaeq::nn_train_kernel<{nt}, {n}, {'true' if bn else 'false'}, {2 if sps == 2 else 0}, {bk}>"


def _check(tag, err, base, floor):
    """err (kernel vs float64) within FACTOR x base (float32 oracle vs float64) or the floor."""
    _note(f"{tag} err", err)
    _note(f"{tag} err / f32-oracle err", err / max(base, 1e-30))
    _note(f"{tag} err / tolerance", err / max(FACTOR * base, floor))
    assert err <= max(FACTOR * base, floor), (tag, err, base)


def _engine(n, bn, k1, k2, M, sps, thetas, bns=None):
    from vae_equalizer_amd.engine import NNEngine
    eng = NNEngine(len(thetas), M, k1, k2, ref.levels(n), DEV, sps, batch_norm=bn)
    assert eng.NP == thetas[0].size and eng.offsets() == ref.offsets(n, k1, k2, M, bn)
    eng.theta.copy_(torch.from_numpy(np.stack(thetas)).to(DEV))
    if bn:
        eng.bn.copy_(torch.from_numpy(np.stack(bns)).to(DEV))
    return eng


def _case(seed, n, bn, B, sps, k1, k2, M, steps=1, R=1, extra=0):
    rng = np.random.default_rng(seed)
    thetas = [ref.init_theta(rng, n, k1, k2, M, bn) for _ in range(R)]
    bns = [ref.random_bn(rng, n) for _ in range(R)] if bn else None
    x = (0.5 * rng.standard_normal((R, 2, steps * B * sps + extra))).astype(np.float32)
    return thetas, bns, x


def _f32_grads(x, theta, bn0, amp, n, bn, k1, k2, M, sps):
    return (oracle.nnbn_step_grads(x, theta, bn0, amp, k1, k2, M, sps, np.float32) if bn else
            oracle.nn_step_grads(x, theta, amp, k1, k2, M, sps, np.float32))


def teacher_forced(n, bn, B, sps, k1, k2, M, seed=0):
    """One teacher-forced step (no_update, want_q, debug_grads): q, loss and each parameter tensor's gradient against float64."""
    thetas, bns, x = _case(seed or (B * 131 + sps * 17 + k1 * 5 + k2 + M + n + bn), n, bn, B, sps, k1, k2, M)
    eng = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    r = eng.train(torch.from_numpy(x).to(DEV), B, 1, 1e-3, want_q=True, debug_grads=True, no_update=True)
    torch.cuda.synchronize()
    name = _last()
    amp = ref.levels(n)
    t64 = ref.step_grads(x[0], thetas[0], amp, n, k1, k2, M, sps, bn, bns[0] if bn else None)
    t32 = _f32_grads(x[0], thetas[0], bns[0] if bn else None, amp, n, bn, k1, k2, M, sps)
    tag = (n, bn, B, sps, k1, k2, M)
    q = _np(r["q"])[0]
    _check("tf q", np.abs(q - t64["q"]).max(), np.abs(t32["q"] - t64["q"]).max(), 2e-5)
    lo = float(_np(r["loss"])[0, 0])
    _check("tf loss", abs(lo - t64["loss"]) / abs(t64["loss"]), abs(float(t32["loss"]) - t64["loss"]) / abs(t64["loss"]), 1e-5)
    o = eng.offsets()
    names = ["w1", "b1", "w2", "b2"] + (["gamma", "beta"] if bn else []) + ["h"]
    g = _np(r["g"])[0]
    for nm, a, b in zip(names, o[:-1], o[1:]):
        err, base = relerr(g[a:b], t64["g"][a:b]), relerr(t32["g"][a:b], t64["g"][a:b])
        try:
            _check(f"tf grad {nm}", err, base, 5e-5)
        except AssertionError:
            raise AssertionError((tag, nm, err, base))
    return name


# ------------------------------------------------------------------ a. teacher-forced step over the index grid
def _grid():
    SPS, K1, K2, MS = (1, 2, 3, 4, 8), (1, 3, 11, 25, 63), (1, 3, 5, 9), (1, 3, 13, 25, 63)
    cases = []
    for i in range(30):                        # every (n_lev, sps, Net / Net_BN) triple once
        n, sps, bn = (2, 4, 8)[i % 3], SPS[i % 5], (i // 3) % 2 == 1
        k1, k2, M = K1[(2 * i + 1) % 5], K2[(i // 2) % 4], MS[(3 * i + 2) % 5]
        lo = 2 * (M // 2)
        B = [lo + 1, lo + 39, 640 // sps + 1, 640 // sps][i % 4]   # just above the halo, odd, L just past / at most 640
        B = max(B, lo + 1, 2 if bn else 1)
        cases.append((n, bn, B, sps, k1, k2, M))
    return cases


SWEEP = {8: (300, 2, 25, 3, 25), 4: (60, 2, 11, 3, 9), 2: (41, 2, 7, 5, 13)}


@pytest.mark.parametrize("n,bn,B,sps,k1,k2,M", _grid())
def test_teacher_forced_grid(n, bn, B, sps, k1, k2, M):
    from vae_equalizer_amd import _native as nat
    if _lds(2 * (M // 2) + 1, sps, M, n, k1, k2, bn) > 160 * 1024:      # not even the smallest minibatch fits: refused before any launch
        thetas, bns, x = _case(1, n, bn, B, sps, k1, k2, M)
        with pytest.raises(nat.VaeqError, match="code -3"):
            _engine(n, bn, k1, k2, M, sps, thetas, bns).train(torch.from_numpy(x).to(DEV), B, 1, 1e-3)
        return
    B = min(B, _ceiling(sps, M, n, k1, k2, bn))                          # (the few grid points past 160 KiB: the largest B that fits)
    assert teacher_forced(n, bn, B, sps, k1, k2, M) == _train_name(n, bn, sps)


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_teacher_forced_sweep_shapes(n, bn):
    """The sweep script's shape (B 300, M 25, k1 25, k2 3, sps 2): BK = 1 for 64-QAM, BK = 2 for 16-QAM, generic for 4-QAM; and each
    n_lev's own sweep shape."""
    name = teacher_forced(n, bn, 300, 2, 25, 3, 25)
    assert name == _train_name(n, bn, 2, {8: 1, 4: 2, 2: 0}[n])
    B, sps, k1, k2, M = SWEEP[n]
    assert teacher_forced(n, bn, B, sps, k1, k2, M) == _train_name(n, bn, sps, 1 if (n, B) == (8, 300) else 0)


def _lds(B, sps, M, n, k1, k2, bn):
    from vae_equalizer_amd import _native as nat
    return int(nat.lib().vaeq_nn_lds_bytes(B, sps, M, n, k1, k2, int(bn)))


def _ceiling(sps, M, n, k1, k2, bn):
    lo, hi = 2 * (M // 2) + 1, 1 << 14
    assert _lds(lo, sps, M, n, k1, k2, bn) <= 160 * 1024 < _lds(hi, sps, M, n, k1, k2, bn)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _lds(mid, sps, M, n, k1, k2, bn) <= 160 * 1024 else (lo, mid)
    return lo


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_teacher_forced_at_the_lds_ceiling(n, bn):
    """k1 = 63, k2 = 9, M = 63 at the largest B whose working set fits 160 KiB (found from vaeq_nn_lds_bytes); one more is refused."""
    from vae_equalizer_amd import _native as nat
    B = _ceiling(2, 63, n, 63, 9, bn)
    assert teacher_forced(n, bn, B, 2, 63, 9, 63) == _train_name(n, bn, 2)
    thetas, bns, x = _case(5, n, bn, B + 1, 2, 63, 9, 63)
    eng = _engine(n, bn, 63, 9, 63, 2, thetas, bns)
    with pytest.raises(nat.VaeqError, match="code -3"):
        eng.train(torch.from_numpy(x).to(DEV), B + 1, 1, 1e-3)


# ------------------------------------------------------------------ b. free steps against the float64 loop
FREE = [  # n, bn, B, sps, k1, k2, M
    (8, True, 330, 2, 11, 3, 13), (8, True, 320, 2, 5, 3, 9), (8, True, 641, 1, 3, 1, 3), (4, True, 350, 2, 7, 3, 9),
    (2, True, 41, 2, 7, 5, 13), (2, True, 230, 3, 3, 1, 5), (2, True, 213, 3, 5, 3, 7), (4, False, 60, 2, 11, 3, 9),
    (4, True, 300, 2, 25, 3, 25), (4, False, 300, 2, 25, 3, 25), (8, False, 300, 2, 25, 3, 25), (8, True, 300, 2, 25, 3, 25),
    (2, False, 37, 1, 1, 1, 1), (8, True, 97, 3, 9, 5, 13), (4, True, 90, 8, 3, 9, 3), (2, False, 300, 2, 25, 3, 25),
]


def _sensitive(st, o):
    """Parameters whose gradient was rounding-level (per tensor) at some step: AMSGrad moves them by +-lr on the sign of rounding."""
    bad = np.zeros(o[-1], bool)
    for g in st.grads:
        for a, b in zip(o[:-1], o[1:]):
            bad[a:b] |= np.abs(g[a:b]) <= 1e-4 * np.abs(g[a:b]).max()
    return bad


def _f32_loop(theta, bn0, x, steps, B, amp, n, bn, k1, k2, M, lr, sps):
    if bn:
        so = oracle.NNBNState(theta, n, np.float32)
        so.bn = np.array(bn0, np.float32)
        lo = oracle.nnbn_train(so, x, steps, B, amp, k1, k2, M, lr, sps, np.float32)
    else:
        so = oracle.NNState(theta, np.float32)
        lo = oracle.nn_train(so, x, steps, B, amp, k1, k2, M, lr, sps, np.float32)
    return so, lo


@pytest.mark.parametrize("n,bn,B,sps,k1,k2,M", FREE)
def test_free_steps_against_float64(n, bn, B, sps, k1, k2, M):
    """Two runs with their own parameters, running statistics, data and step size, five AMSGrad steps, rx rows longer than the five
    minibatches: losses, theta, m, v, vmax, step and the running statistics against the float64 loop."""
    steps, lrs = 5, (2e-3, 3.5e-3)
    thetas, bns, x = _case(B * 7 + k1 + M + n + sps * 3 + bn, n, bn, B, sps, k1, k2, M, steps, R=2, extra=37)
    eng = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    r = eng.train(torch.from_numpy(x).to(DEV), B, steps, torch.tensor(lrs, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    _last()
    amp, o = ref.levels(n), eng.offsets()
    for i in range(2):
        st = ref.State(thetas[i], n, bn, bns[i] if bn else None)
        l64, _, _ = ref.train(st, x[i], steps, B, amp, n, k1, k2, M, sps, lrs[i], bn)
        so, l32 = _f32_loop(thetas[i], bns[i] if bn else None, x[i], steps, B, amp, n, bn, k1, k2, M, lrs[i], sps)
        ok = ~_sensitive(st, o)
        _check("free loss", np.max(np.abs(_np(r["loss"])[i] - l64) / np.abs(l64)), np.max(np.abs(l32 - l64) / np.abs(l64)), 2e-5)
        th = _np(eng.theta)[i]
        _check("free theta", np.abs(th - st.theta)[ok].max(), np.abs(so.theta - st.theta)[ok].max(), 2e-5)
        assert np.abs(th - st.theta).max() <= 2.01 * steps * lrs[i]
        for nm, ours, theirs, mine in (("m", eng.m, so.m, st.m), ("v", eng.v, so.v, st.v), ("vmax", eng.vmax, so.vmax, st.vmax)):
            _check(f"free {nm}", relerr(_np(ours)[i], mine), relerr(theirs, mine), 1e-4)
        if bn:
            _check("free bn_running", relerr(_np(eng.bn)[i], st.bn), relerr(so.bn, st.bn), 1e-5)
        assert int(eng.step[i]) == steps


# ------------------------------------------------------------------ c. state invariants, bit for bit
INV = [(8, False, 300, 2, 25, 3, 25), (4, True, 300, 2, 25, 3, 25), (8, True, 150, 2, 11, 3, 13), (2, True, 90, 3, 7, 3, 9),
       (4, False, 60, 2, 11, 3, 9), (8, True, 330, 1, 3, 5, 5)]


def _state(eng):
    return [t.clone() for t in (eng.theta, eng.m, eng.v, eng.vmax, eng.step)] + ([eng.bn.clone()] if eng.batch_norm else [])


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("n,bn,B,sps,k1,k2,M", INV)
def test_two_calls_equal_one(n, bn, B, sps, k1, k2, M):
    """k steps, then k more from where the first call stopped == 2k steps in one call."""
    thetas, bns, x = _case(B + 3, n, bn, B, sps, k1, k2, M, 4, R=2)
    xt = torch.from_numpy(x).to(DEV)
    a = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    a.train(xt, B, 4, 3e-3)
    b = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    b.train(xt, B, 2, 3e-3)
    b.train(xt[..., 2 * B * sps:].contiguous(), B, 2, 3e-3)
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))
    assert int(a.step[0]) == 4


@pytest.mark.parametrize("n,bn,B,sps,k1,k2,M", INV)
def test_runs_are_independent(n, bn, B, sps, k1, k2, M):
    """R = 3 runs with their own theta, running statistics, lr and data from rows of S > steps B sps samples == each run alone, both from
    the same long row and from a row cut to exactly steps B sps samples."""
    steps, R, lrs = 3, 3, [2e-3, 3e-3, 5e-3]
    thetas, bns, x = _case(B * 5 + 1, n, bn, B, sps, k1, k2, M, steps, R=R, extra=101)
    xt = torch.from_numpy(x).to(DEV)
    e = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    r = e.train(xt, B, steps, torch.tensor(lrs, device=DEV))
    torch.cuda.synchronize()
    for i in range(R):
        for xi in (xt[i:i + 1].contiguous(), xt[i:i + 1, :, :steps * B * sps].contiguous()):
            s = _engine(n, bn, k1, k2, M, sps, thetas[i:i + 1], bns[i:i + 1] if bn else None)
            r1 = s.train(xi, B, steps, lrs[i])
            torch.cuda.synchronize()
            assert torch.equal(r["loss"][i:i + 1], r1["loss"]), i
            assert all(torch.equal(u[i:i + 1], v) for u, v in zip(_state(e), _state(s))), i


@pytest.mark.parametrize("n,bn,B,sps,k1,k2,M", INV[:4])
def test_no_update_and_zero_lr(n, bn, B, sps, k1, k2, M):
    """no_update = 1 leaves theta, m, v, vmax, step and the running statistics untouched; lr = 0 keeps theta bit for bit while m, v, vmax,
    step and the running statistics advance as float64 says."""
    thetas, bns, x = _case(B * 9 + 2, n, bn, B, sps, k1, k2, M, 5, R=2)
    xt = torch.from_numpy(x).to(DEV)
    e = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    e.train(xt, B, 2, 3e-3)                                              # a state that is not the initial one
    before = _state(e)
    e.train(xt[..., 2 * B * sps:].contiguous(), B, 3, 3e-3, no_update=True)
    torch.cuda.synchronize()
    assert _same(before, _state(e))
    z = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    z.train(xt, B, 3, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(z.theta, torch.from_numpy(np.stack(thetas)).to(DEV))
    for i in range(2):
        st = ref.State(thetas[i], n, bn, bns[i] if bn else None)
        ref.train(st, x[i], 3, B, ref.levels(n), n, k1, k2, M, sps, 0.0, bn)
        for nm, ours, mine in (("m", z.m, st.m), ("v", z.v, st.v), ("vmax", z.vmax, st.vmax)):
            err = relerr(_np(ours)[i], mine)
            _note(f"lr0 {nm} relerr", err)
            assert err < 1e-4, (nm, err)
        if bn:
            assert relerr(_np(z.bn)[i], st.bn) < 1e-5
        assert int(z.step[i]) == 3


# ------------------------------------------------------------------ d. BatchNorm edges
def test_batchnorm_one_sample_is_refused():
    """L = B sps = 1 has no batch variance (BatchNorm1d raises); the kernel refuses it with VAEQ_ERR_SHAPE, Net takes it."""
    from vae_equalizer_amd import _native as nat
    for n in (2, 4, 8):
        thetas, bns, x = _case(n, n, True, 1, 1, 3, 1, 1)
        e = _engine(n, True, 3, 1, 1, 1, thetas, bns)
        with pytest.raises(nat.VaeqError, match="code -2"):
            e.train(torch.from_numpy(x).to(DEV), 1, 1, 1e-3)
    assert teacher_forced(4, False, 1, 1, 3, 1, 1) == _train_name(4, False, 1)


@pytest.mark.parametrize("n,B,sps,k1,k2,M", [(8, 320, 2, 5, 3, 7), (8, 641, 1, 3, 1, 3), (4, 320, 2, 5, 3, 7), (4, 321, 2, 5, 3, 7),
                                             (4, 641, 1, 1, 1, 1), (2, 320, 2, 5, 3, 7), (2, 641, 1, 5, 3, 7), (2, 640, 1, 3, 3, 3),
                                             (8, 1, 2, 3, 1, 1), (4, 1, 2, 1, 3, 1), (2, 1, 2, 5, 1, 1)])
def test_batchnorm_row_edges(n, B, sps, k1, k2, M):
    """L = 640 (the last row held in registers), L = 641 / 642 (the first that are not) and L = 2, teacher-forced."""
    assert teacher_forced(n, True, B, sps, k1, k2, M) == _train_name(n, True, sps)


# ------------------------------------------------------------------ e. eval forward
EVAL_N = [1, 2, 254, 255, 256, 509, 510, 511, 766, 3000]


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("bn,sps,k1,k2,M", [(True, 1, 63, 9, 5), (False, 3, 11, 3, 9), (True, 2, 25, 3, 25)])
def test_eval_forward(n, bn, sps, k1, k2, M):
    """Three runs with their own parameters (and random running statistics, gamma, beta) over blocks of 1 to 3000 symbols, computed in
    255-symbol tiles whose halos reach into the neighbouring tiles == the float64 whole-block forward."""
    for N in EVAL_N:
        thetas, bns, x = _case(N * 3 + k1 + n, n, bn, N, sps, k1, k2, M, R=3)
        e = _engine(n, bn, k1, k2, M, sps, thetas, bns)
        q = _np(e.forward(torch.from_numpy(x).to(DEV)))
        torch.cuda.synchronize()
        assert _last() == f"vaeq::nn_forward_kernel<1024, {n}>"
        for i in range(3):
            q64 = ref.eval_forward(x[i], thetas[i], n, k1, k2, sps, M, bn, bns[i] if bn else None)
            q32 = (oracle.nnbn_forward_eval(x[i], thetas[i], bns[i], n, k1, k2, sps, np.float32) if bn else
                   oracle.nn_forward(x[i], thetas[i], n, k1, k2, sps, np.float32))
            _check("eval q", np.abs(q[i] - q64).max(), np.abs(q32 - q64).max(), 2e-5)


# ------------------------------------------------------------------ f. validate
def _validate_case(n, bn, N, sps, k1, k2, M, n_shift, shifts, seed):
    """R = len(shifts) runs: data = the float64 decisions of each run's own q with ~2 % flips, delayed by shifts[r] and rotated by r
    quadrants -> (ser, shift) of the kernel and the float64 (shift, SER, low-margin symbols of the SER window)."""
    R = len(shifts)
    rng = np.random.default_rng(seed)
    thetas, bns, x = _case(seed, n, bn, N, sps, k1, k2, M, R=R)
    x *= 2
    o = ref.offsets(n, k1, k2, M, bn)
    for t in thetas:
        t[o[2]:o[3]] *= 4                                                   # confident decisions: E_q[x] follows them
    e = _engine(n, bn, k1, k2, M, sps, thetas, bns)
    amp = ref.levels(n)
    datas, refs = [], []
    for r, k in enumerate(shifts):
        q64 = ref.eval_forward(x[r], thetas[r], n, k1, k2, sps, M, bn, bns[r] if bn else None)
        dec, margin = ref.decisions(q64, n)
        dec = np.where(rng.random(dec.shape) < 0.02, (dec + 1) % n, dec)
        d = np.roll(dec, -k, axis=1)
        K = n - 1
        d = [d, np.stack([K - d[0], K - d[1]]), np.stack([d[1], K - d[0]]), np.stack([K - d[1], d[0]])][r % 4]
        tx = amp[d].astype(np.float16)
        datas.append(tx)
        sh, ser = ref.validate(q64, tx, n_shift, amp, n)
        low = int(np.sum(margin[11 + sh:N - 11] < 1e-5)) if 11 + sh >= 0 else 0
        refs.append((sh, ser, low))
    ser, shv = e.validate(torch.from_numpy(x).to(DEV), torch.from_numpy(np.stack(datas)).to(DEV), n_shift)
    torch.cuda.synchronize()
    return _np(ser), _np(shv), refs, _last()


def _check_validate(ser, shv, refs, N):
    for i, (sh, s64, low) in enumerate(refs):
        assert int(shv[i]) == sh, (i, int(shv[i]), sh)
        if np.isnan(s64):                                                   # a shift of -11 or less (see test_validate_shift_below_minus_10)
            assert np.isnan(ser[i]), (i, sh, float(ser[i]))
            continue
        ln = N - 22 - sh
        err = abs(float(ser[i]) - s64)
        _note("validate SER err", err)
        _note("validate low-margin symbols", low)
        assert err <= 1.0 / N + low / ln + 1e-6, (i, float(ser[i]), s64, low)


def _val_nmax(n, bn, sps, k1, k2, M):
    """The largest N the validation kernel's LDS admits (<= 65536): its refusal (VAEQ_ERR_LDS) comes before any launch."""
    from vae_equalizer_amd import _native as nat
    thetas, bns, _ = _case(1, n, bn, 1, sps, k1, k2, M)
    e = _engine(n, bn, k1, k2, M, sps, thetas, bns)

    def fits(N):
        x = torch.zeros(1, 2, N * sps, device=DEV)
        d = torch.zeros(1, 2, N, dtype=torch.float16, device=DEV)
        try:
            e.validate(x, d, 21)
            torch.cuda.synchronize()
            return True
        except nat.VaeqError as err:
            assert "code -3" in str(err)
            return False

    if fits(65536):
        return 65536
    lo, hi = 64, 65536
    assert fits(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


SHIFTS = {1: [0, 0, 0, 0], 21: [0, 4, -7, 9], 32: [0, 16, -10, 5]}


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_validate(n, bn):
    """Fused eval forward + find_shift + SER_q at the sweep shape (BK = 1 for 64-QAM) for N = 64, 1000, 8192 and the largest N the LDS
    admits, n_shift 1, 21 and 32: the shift exactly, the SER within 1 / N of float64 (symbols whose float64 decision margin is below 1e-5
    may go either way and are counted)."""
    sps, k1, k2, M = 2, 25, 3, 25
    nmax = _val_nmax(n, bn, sps, k1, k2, M)
    _note(f"validate N max (n_lev {n}, bn {int(bn)})", nmax)
    for N in (64, 1000, 8192, nmax):
        for n_shift in (1, 21, 32):
            ser, shv, refs, name = _validate_case(n, bn, N, sps, k1, k2, M, n_shift, SHIFTS[n_shift], N + n_shift + n)
            assert name == f"vaeq::nn_validate_kernel<1024, {n}, {1 if n == 8 else 0}>"
            _check_validate(ser, shv, refs, N)


@pytest.mark.parametrize("n,bn", [(8, True), (4, False), (2, True)])
def test_validate_generic_shape(n, bn):
    ser, shv, refs, name = _validate_case(n, bn, 3000, 3, 11, 5, 9, 21, SHIFTS[21], 77 + n)
    assert name == f"vaeq::nn_validate_kernel<1024, {n}, 0>"
    _check_validate(ser, shv, refs, 3000)


@pytest.mark.parametrize("n", [2, 8])
def test_validate_shift_below_minus_10(n):
    """n_shift = 32 admits shifts down to -15.  From -11 down the reference's data[:, 11:-11-shift] is empty (below -11 its
    q[:, 11+shift:-11] too) and SER_q's mean over no symbols is NaN; the kernel returned a number there, below -11 from decisions read in
    front of its decision array."""
    ser, shv, refs, _ = _validate_case(n, False, 1000, 2, 25, 3, 25, 32, [-13, -15, -11, -10, -12], 5)
    for i, (sh, s64, _) in enumerate(refs):
        assert int(shv[i]) == sh
        if sh <= -11:
            assert np.isnan(s64) and np.isnan(ser[i]), (i, sh, float(ser[i]))
        else:
            assert abs(float(ser[i]) - s64) <= 1.0 / 1000 + 1e-6


def test_validate_refusals():
    from vae_equalizer_amd import _native as nat
    thetas, bns, _ = _case(1, 8, False, 1, 2, 25, 3, 25)
    e = _engine(8, False, 25, 3, 25, 2, thetas, bns)
    for N, n_shift in ((1000, 33), (1000, 0), (63, 21), (65537, 21)):
        x = torch.zeros(1, 2, N * 2, device=DEV)
        d = torch.zeros(1, 2, N, dtype=torch.float16, device=DEV)
        with pytest.raises(nat.VaeqError, match="code -2"):
            e.validate(x, d, n_shift)


# ------------------------------------------------------------------ g. dispatch edges
def _raw_train(n, bn, B, sps, k1, k2, M, steps=1, S=None):
    """vaeq_nn_train on buffers sized for the given shape by formula (so that no shape, refused or not, can reach past them)."""
    from vae_equalizer_amd import _native as nat
    C_ = 2 * n
    NP = ref.offsets(n, max(k1, 1), max(k2, 1), max(M, 1), bn)[-1]
    L = max(steps * B * sps, 1)
    S = L if S is None else S
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    rx, th, m, v, vx = f(2 * max(S, L) + 64), f(NP), f(NP), f(NP), f(NP)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    amp, lr, loss, bnr = f(max(n, 8)), f(1), f(max(steps, 1)), f(2 * max(C_, 16))
    a = nat.NNArgs(R=1, steps=steps, B=B, sps=sps, M=M, n_lev=n, k1=k1, k2=k2, S=S, rx=nat.ptr(rx), theta=nat.ptr(th), adam_m=nat.ptr(m),
                   adam_v=nat.ptr(v), adam_x=nat.ptr(vx), step=nat.ptr(step, torch.int32), amp=nat.ptr(amp), lr=nat.ptr(lr), loss=nat.ptr(loss),
                   q_out=None, dbg_g=None, no_update=1, batch_norm=int(bn), bn_running=nat.ptr(bnr))
    import ctypes as C
    with torch.cuda.device(DEV):
        code = int(nat.lib().vaeq_nn_train(C.byref(a), nat.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return code


def test_dispatch_shape_bounds():
    """Every bound of nn_shape_ok runs, one past it returns VAEQ_ERR_SHAPE; so does a window past S."""
    base = dict(n=8, bn=False, B=100, sps=2, k1=25, k2=3, M=25)
    for good, bad in ((dict(sps=8), dict(sps=9)), (dict(M=63), dict(M=65)), (dict(M=25), dict(M=24)), (dict(k1=63), dict(k1=65)),
                      (dict(k2=9), dict(k2=11)), (dict(n=2), dict(n=3)), (dict(B=49, M=49), dict(B=48, M=49))):
        assert _raw_train(**dict(base, **good)) == 0, good
        assert _raw_train(**dict(base, **bad)) == -2, bad
    assert _raw_train(**dict(base, steps=2, S=400)) == 0
    assert _raw_train(**dict(base, steps=2, S=399)) == -2


@pytest.mark.parametrize("env,value,name", [("VAEQ_NN_HALF", "1", "vaeq::nn_train_half_kernel<256, 1>"),
                                            ("VAEQ_NN_NT", "256", _train_name(8, False, 2, 1, 256)),
                                            ("VAEQ_NN_NT", "1024", _train_name(8, False, 2, 1, 1024))])
def test_experiment_knobs(monkeypatch, env, value, name):
    """The half-minibatch kernel and the 256 / 1024-thread variants of the baked 64-QAM `Net` kernel: one teacher-forced step and five
    free steps against float64, and last_kernel() names them."""
    monkeypatch.setenv(env, value)
    assert teacher_forced(8, False, 300, 2, 25, 3, 25) == name
    thetas, _, x = _case(21, 8, False, 300, 2, 25, 3, 25, 5, R=2)
    eng = _engine(8, False, 25, 3, 25, 2, thetas)
    r = eng.train(torch.from_numpy(x).to(DEV), 300, 5, 3e-3)
    torch.cuda.synchronize()
    assert _last() == name
    o = eng.offsets()
    for i in range(2):
        st = ref.State(thetas[i])
        l64, _, _ = ref.train(st, x[i], 5, 300, ref.levels(8), 8, 25, 3, 25, 2, 3e-3)
        so, l32 = _f32_loop(thetas[i], None, x[i], 5, 300, ref.levels(8), 8, False, 25, 3, 25, 3e-3, 2)
        ok = ~_sensitive(st, o)
        _check("knob loss", np.max(np.abs(_np(r["loss"])[i] - l64) / np.abs(l64)), np.max(np.abs(l32 - l64) / np.abs(l64)), 2e-5)
        _check("knob theta", np.abs(_np(eng.theta)[i] - st.theta)[ok].max(), np.abs(so.theta - st.theta)[ok].max(), 2e-5)
        _check("knob vmax", relerr(_np(eng.vmax)[i], st.vmax), relerr(so.vmax, st.vmax), 1e-4)


# ------------------------------------------------------------------ coverage (runs last)
def test_every_instantiation_is_reached():
    want = {_train_name(n, bn, sps) for n in (2, 4, 8) for bn in (False, True) for sps in (1, 2)}
    want |= {_train_name(8, bn, 2, 1) for bn in (False, True)} | {_train_name(4, bn, 2, 2) for bn in (False, True)}
    want |= {"vaeq::nn_train_half_kernel<256, 1>", _train_name(8, False, 2, 1, 256), _train_name(8, False, 2, 1, 1024)}
    want |= {f"vaeq::nn_forward_kernel<1024, {n}>" for n in (2, 4, 8)}
    want |= {f"vaeq::nn_validate_kernel<1024, {n}, 0>" for n in (2, 4, 8)} | {"vaeq::nn_validate_kernel<1024, 8, 1>"}
    print("  reached:", len(SEEN), "instantiations")
    assert want <= SEEN, sorted(want - SEEN)

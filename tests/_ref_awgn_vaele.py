"""Float64 model of the fused AWGN VAE-LE training loop (vaeq_awgn_train), written for the tests from the math alone: numpy and torch on the
CPU, neither the package nor the C oracle is imported.

One step is _ref_operators.awgn_forward followed by awgn_loss with the prior P, on the float32 inputs exactly as the kernel sees them, widened to
float64; the gradients come from torch.autograd.grad (no hand-derived backward).  The optimiser is Adam(amsgrad=True) with beta = (0.9, 0.999),
eps = 1e-8, written out by hand so that a state (moments, maxima, step count) can be injected; tests/test_ref_awgn_vaele_host.py holds it to
torch.optim.Adam.

cases() is the one list of envelope cases that the host test (conditioning) and the GPU test (kernels against the model) both iterate.
"""
import functools

import numpy as np
import torch

import _ref_operators as ref

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
STATE_KEYS = ("mW", "vW", "xW", "mh", "vh", "xh")


def _t(a, dtype=np.float64):
    """float32 as the kernel sees it, widened to float64 (or kept, for the float32 evaluation of the model)."""
    return torch.from_numpy(np.asarray(a, np.float32).astype(dtype))


def amsgrad_step(p, g, m, v, x, t, lr):
    """One torch.optim.Adam(amsgrad=True) step, in place on the float64 arrays p, m, v, x; t is the step count AFTER this step.
    The maximum is taken over the raw second moment, the bias corrections divide sqrt(max) and the step size (torch/optim/adam.py,
    _single_tensor_adam)."""
    m *= BETA1
    m += (1 - BETA1) * g
    v *= BETA2
    v += (1 - BETA2) * g * g
    np.maximum(x, v, out=x)
    denom = np.sqrt(x) / np.sqrt(1 - BETA2 ** t) + EPS
    p -= (lr / (1 - BETA1 ** t)) * m / denom


def adam_travel_bound(b1, b2, t0, t):
    """Bound on |p_t - p_t0| / lr of one entry under bias-corrected Adam / AMSGrad between the step counts t0 and t, whatever its gradients
    were, for moments that are zero at count 0 (t0 = 0) or that came from t0 earlier steps of the same recursion.

    At count s the first moment is m_s = (1 - b1) sum_{i<=s} b1^(s-i) g_i, so m_s / (1 - b1^s) = sum_i w_i g_i with the normalised weights
    w_i = (1 - b1) b1^(s-i) / (1 - b1^s), sum_i w_i = 1; likewise v_s / (1 - b2^s) = sum_i u_i g_i^2 with u_i = (1 - b2) b2^(s-i) / (1 - b2^s).
    By Jensen (the w_i are a probability vector) (sum_i w_i g_i)^2 <= sum_i w_i g_i^2 = sum_i (w_i / u_i) u_i g_i^2 <= max_i (w_i / u_i) sum_i u_i g_i^2,
    hence |mhat_s| <= sqrt(max_i w_i / u_i) sqrt(vhat_s).  The step divides by sqrt(max(x, v)_s / (1 - b2^s)) + eps >= sqrt(vhat_s), so it moves
    the entry by at most lr sqrt(max_i w_i / u_i); the travel is the sum over s = t0 + 1 .. t.  From a fresh state the factor is 1, 1.04, 1.06, 1.08
    at s = 1 .. 4; for an old run it tends to sqrt((1 - b1) / (1 - b2)) = 10."""
    total = 0.0
    for s in range(t0 + 1, t + 1):
        i = np.arange(1, s + 1, dtype=np.float64)
        w = (1 - b1) * b1 ** (s - i) / (1 - b1 ** s)
        u = (1 - b2) * b2 ** (s - i) / (1 - b2 ** s)
        total += float(np.sqrt(np.max(w / u)))
    return total


def step_grads(x, W, h, amp, P, amp_mean, var, sps):
    """One minibatch x[2,B*sps] at the taps W[2,M], h[2,M] (float64 arrays; float32 arrays evaluate the model in float32) -> (loss, y[2,B] un-normalised, q[2n,B], gW[2,M], gh[2,M])."""
    M, dt = W.shape[-1], W.dtype
    Wt, ht = torch.tensor(W.reshape(1, 2, M), requires_grad=True), torch.tensor(h, requires_grad=True)
    xt = _t(x, dt)
    q, out = ref.awgn_forward(xt, Wt, _t(amp, dt), float(np.float32(amp_mean)), float(np.float32(var)), sps)
    loss = ref.awgn_loss(q, xt, ht, _t(amp, dt), _t(P, dt))
    gW, gh = torch.autograd.grad(loss, (Wt, ht))
    return float(loss.detach()), out.detach().numpy(), q.detach().numpy(), gW.numpy().reshape(2, M), gh.numpy()


def train(rx, W, h, state, steps, B, amp, P, amp_mean, var, lr, sps, dtype=np.float64):
    """The training loop of one run: rx[2,S] float32, W[2,M] (or [1,2,M]) and h[2,M] float32, state None (fresh) or a dict with mW, vW, xW, mh, vh,
    xh [2,M] and step -> dict(loss[steps], y[2,steps*B], q[2n,steps*B], gW[steps,2,M], gh[steps,2,M], W_hist / h_hist [steps,2,M] (taps after each
    step), st_hist (the six optimiser arrays after each step), W, h, mW, vW, xW, mh, vh, xh, step), all float64.
    dtype = np.float32 evaluates the same loop with float32 tensors and float32 state: not a reference for anything, but the measure of how far the
    number format alone takes a float32 implementation from the model (float32_gap)."""
    M = np.asarray(W).shape[-1]
    W = np.asarray(W, np.float32).astype(dtype).reshape(2, M).copy()
    h = np.asarray(h, np.float32).astype(dtype).reshape(2, M).copy()
    st = {k: np.zeros((2, M), dtype) for k in STATE_KEYS}
    t = 0
    if state is not None:
        for k in STATE_KEYS:
            st[k] = np.asarray(state[k], np.float32).astype(dtype).reshape(2, M).copy()
        t = int(state["step"])
    lr = float(np.float32(lr))
    L = B * sps
    out = {k: [] for k in ("loss", "y", "q", "gW", "gh", "W_hist", "h_hist", "st_hist")}
    for s in range(steps):
        loss, y, q, gW, gh = step_grads(np.asarray(rx)[:, s * L:(s + 1) * L], W, h, amp, P, amp_mean, var, sps)
        t += 1
        amsgrad_step(W, gW, st["mW"], st["vW"], st["xW"], t, lr)
        amsgrad_step(h, gh, st["mh"], st["vh"], st["xh"], t, lr)
        for k, v in zip(out, (loss, y, q, gW, gh, W.copy(), h.copy(), {k: v.copy() for k, v in st.items()})):
            out[k].append(v)
    res = {"loss": np.array(out["loss"]), "y": np.concatenate(out["y"], 1), "q": np.concatenate(out["q"], 1)}
    res.update({k: np.stack(out[k]) for k in ("gW", "gh", "W_hist", "h_hist")})
    res.update(W=W, h=h, step=t, st_hist=out["st_hist"], **st)
    return res


def prefix(m, k, B):
    """The first k steps of a model run m, as train() would have returned them for steps = k."""
    res = {"loss": m["loss"][:k], "y": m["y"][:, :k * B], "q": m["q"][:, :k * B], "gW": m["gW"][:k], "gh": m["gh"][:k],
           "W": m["W_hist"][k - 1], "h": m["h_hist"][k - 1], "step": m["step"] - (len(m["loss"]) - k)}
    res.update(m["st_hist"][k - 1])
    return res


def conditioned(grads, floor=1e-2):
    """grads[steps,2,M] of one group -> bool[2,M]: the entries whose gradient is, at EVERY step, at least `floor` of the largest gradient
    magnitude of the group at that step.  Adam divides by sqrt(v): an entry whose gradient is rounding noise moves by +-lr on a coin flip, so only
    the conditioned entries are compared tightly; the others are held to adam_travel_bound."""
    g = np.abs(np.asarray(grads, np.float64))
    return np.all(g >= floor * g.max(axis=(1, 2), keepdims=True), axis=0)


# ------------------------------------------------------------------ the envelope
def levels(n):
    a = np.arange(-(n - 1), n, 2).astype(np.float32)
    return (a / np.sqrt(2 * np.mean(a ** 2))).astype(np.float32)


def wave_kernel_name(B, M, n):
    """The instantiation vaeq_awgn_train documents for a wave-eligible call (sps = 2, B even, 2 (M / 2) + 2 <= B <= 1024, M in 9 / 17 / 25):
    rounds of 64 symbol pairs per lane, up to three in one wavefront, two per wavefront above 384 symbols; B = 350 at M = 25 is baked."""
    if M == 25 and B == 350:
        return f"vaeq::awgn_wave_kernel<25, {n}, 3, 1, 350>"
    rounds = (B // 2 + 63) // 64
    NR, NW = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (2, 3), 6: (2, 3), 7: (2, 4), 8: (2, 4)}[rounds]
    return f"vaeq::awgn_wave_kernel<{M}, {n}, {NR}, {NW}, 0>"


def generic_kernel_name(threads, n):
    return f"vaeq::awgn_train_kernel<{threads or 256}, {n}>"


def generic_lds_bytes(B, sps, M):
    """Restatement of vaeq_awgn_lds_bytes: the generic kernel's LDS arrays, each padded to four floats."""
    p4 = lambda k: (k + 3) // 4 * 4
    mh = M // 2
    L = B * sps
    nm = L - 2 * mh
    return 4 * (p4(2 * p4(L + 2 * mh)) + 10 * p4(2 * M) + 6 * p4(2 * B) + p4(2 * nm) + p4(M) + 64)


LDS_MAX = 160 * 1024                                           # LDS_MAX of csrc/vaeq_launch.h (tests/test_ref_awgn_vaele_host.py reads it there)


def largest_generic_B(sps, M):
    B = 2 * (M // 2) + 1
    while generic_lds_bytes(B + 1, sps, M) <= LDS_MAX:
        B += 1
    return B


LDS_CASE = dict(sps=2, M=25, n_lev=8)

WAVE_GRID = [  # (B, M, n_lev): both sides of every class edge, both residues of B mod 4, every (M, class) pair, every n_lev in every class
    (10, 9, 4), (18, 17, 2), (26, 25, 8), (126, 25, 2), (128, 17, 8),                     # one round
    (130, 9, 8), (254, 17, 4), (256, 25, 2),                                             # two rounds
    (258, 9, 2), (348, 25, 4), (350, 25, 2), (350, 25, 4), (350, 25, 8), (352, 25, 8), (350, 17, 8), (382, 17, 4), (384, 9, 8),   # three rounds; baked
    (386, 25, 8), (510, 17, 2), (512, 9, 4),                                             # two wavefronts
    (514, 25, 4), (766, 9, 8), (768, 17, 2),                                             # three wavefronts
    (770, 17, 8), (1022, 25, 2), (1024, 9, 4),                                           # four wavefronts
]
GENERIC_GRID = [  # (threads, B, sps, M, n_lev)
    (64, 41, 2, 9, 2), (128, 351, 2, 25, 8), (256, 41, 1, 13, 4), (64, 60, 3, 31, 8), (128, 50, 4, 3, 2), (256, 100, 2, 63, 4),
    (64, 33, 1, 1, 8), (128, 40, 3, 1, 4),
    # B at the minimum 2 (M / 2) + 1 the entry point accepts; (M = 1, B = 1) is left out: with one symbol the normalised output is
    # +-amp_mean whatever W is, so dL/dW is identically zero and every W entry is a coin flip
    (256, 13, 1, 13, 4), (64, 31, 3, 31, 2), (128, 3, 4, 3, 8), (256, 63, 2, 63, 2), (64, 3, 1, 3, 4),
]
# seeds changed where the first choice left under two thirds of a group conditioned (tests/test_ref_awgn_vaele_host.py)
SEED_OVERRIDE = {
    "wave-B130-M9-n8": 138019, "wave-B766-M9-n8": 774019, "generic-T64-B41-s2-M9-n2": 49013, "generic-T64-B33-s1-M1-n8": 48857,
    "generic-ldsmax-B2016": 2024179, "edge-onehot-generic-B41": 72770,
    # ... or left the float32 evaluation of the model further from the float64 one than GAP_LIMIT (a tap group whose whole gradient vanishes)
    "wave-B18-M17-n2": 342853, "wave-B254-M17-n4": 262095, "wave-B258-M9-n2": 273932, "generic-T128-B50-s4-M3-n2": 208416,
    "generic-T256-B100-s2-M63-n4": 108555, "generic-T128-B40-s3-M1-n4": 119207, "generic-T256-B13-s1-M13-n4": 44811, "generic-T64-B3-s1-M3-n4": 90144,
    "edge-steep-wave-B130": 145938, "edge-steep-wave-B386": 402094, "edge-steep-generic-B41": 72770,
}


def _case(kind, name, B, M, n_lev, sps, threads, kernel, **extra):
    c = dict(kind=kind, id=name, B=B, M=M, n_lev=n_lev, sps=sps, threads=threads, kernel=kernel, R=3, steps=4, edge=None)
    c.update(extra)
    c["seed"] = SEED_OVERRIDE.get(name, 1000 * B + 10 * M + n_lev + sps)
    return c


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for B, M, n in WAVE_GRID:
        out.append(_case("wave", f"wave-B{B}-M{M}-n{n}", B, M, n, 2, 1, wave_kernel_name(B, M, n)))
    for T, B, sps, M, n in GENERIC_GRID:
        out.append(_case("generic", f"generic-T{T}-B{B}-s{sps}-M{M}-n{n}", B, M, n, sps, T, generic_kernel_name(T, n)))
    Bmax = largest_generic_B(LDS_CASE["sps"], LDS_CASE["M"])
    out.append(_case("generic", f"generic-ldsmax-B{Bmax}", Bmax, LDS_CASE["M"], LDS_CASE["n_lev"], LDS_CASE["sps"], 256, generic_kernel_name(256, 8)))
    # dispatch: wave-eligible shapes that threads = 0 hands to the generic kernel
    out.append(_case("dispatch", "dispatch-S-mod4-is-2", 128, 25, 8, 2, 0, generic_kernel_name(0, 8), fallback="S%4"))
    out.append(_case("dispatch", "dispatch-rx-off-8-bytes", 130, 17, 4, 2, 0, generic_kernel_name(0, 4), fallback="offset"))
    # numeric edges, on a one-wave, a multi-wave and a generic shape each
    # (the steep demapper on 8 levels: with 2 or 4 every symbol of these frames sits so far from a decision boundary that q is one-hot and
    # the whole gradient of W is rounding noise)
    for edge, n386, n41 in (("onehot", 4, 2), ("steep", 8, 8)):
        out.append(_case("wave", f"edge-{edge}-wave-B130", 130, 9, 8, 2, 1, wave_kernel_name(130, 9, 8), edge=edge))
        out.append(_case("wave", f"edge-{edge}-wave-B386", 386, 25, n386, 2, 1, wave_kernel_name(386, 25, n386), edge=edge))
        out.append(_case("generic", f"edge-{edge}-generic-B41", 41, 9, n41, 2, 128, generic_kernel_name(128, n41), edge=edge))
    return tuple(out)


def cases(kind=None):
    """Every envelope case (dicts; seeded and deterministic), optionally of one kind ("wave", "generic", "dispatch")."""
    return [dict(c) for c in _cases() if kind is None or c["kind"] == kind]


def case_by_id(name):
    return next(dict(c) for c in _cases() if c["id"] == name)


def build(case):
    """The float32 inputs of a case: R runs with their own P, amp_mean, var in 0.005 .. 0.05 and lr in 5e-4 .. 4e-3, `steps` minibatches of ISI +
    noise on random symbols, and a non-Dirac start (Dirac + 0.05 N(0, 1) on both tap sets).  Edges: "onehot" puts one level's prior at 1e-6,
    "steep" sets var = 1e-3.  At var = 1e-3 the gradients of the later steps are 1 / var times as sensitive to the rounding of y as at the
    default var: float32_gap shows the float32 evaluation of the model itself 3 to 80 times GAP_LIMIT away in the moments after 4 steps, for every
    seed tried, while the first step, the losses and the conditioned taps stay inside it.  held() names what a steep case must be conditioned
    on; the kernels are compared on every quantity there too, the later steps' in a bound group of their own.

    The edge "one minibatch of exact zeros" is not built: there the mean |y| that normalises the equaliser output is 0, the model's y / mean|y| is
    0 / 0 and its loss is NaN (tests/test_ref_awgn_vaele_host.py shows it), so there is nothing finite to compare a kernel with."""
    rng = np.random.default_rng(case["seed"])
    R, steps, B, M, n, sps = case["R"], case["steps"], case["B"], case["M"], case["n_lev"], case["sps"]
    amp = levels(n)
    P = rng.uniform(0.5, 1.5, (R, n))
    if case["edge"] == "onehot":
        P[np.arange(R), rng.integers(0, n, R)] = 0.0
        P = P / P.sum(1, keepdims=True) * (1 - 1e-6)
        P[P == 0.0] = 1e-6
    else:
        P /= P.sum(1, keepdims=True)
    P = P.astype(np.float32)
    amp_mean = (np.mean(np.abs(amp)) * rng.uniform(0.9, 1.1, R)).astype(np.float32)
    var = np.exp(rng.uniform(np.log(0.005), np.log(0.05), R)).astype(np.float32)
    if case["edge"] == "steep":
        var[:] = 1e-3
    lr = np.exp(rng.uniform(np.log(5e-4), np.log(4e-3), R)).astype(np.float32)
    sym = rng.choice(amp, (R, 2, steps * B))
    rx = np.repeat(sym, sps, axis=-1).astype(np.float32)
    rx = (0.5 * rx + 0.3 * np.roll(rx, 1, -1) + 0.05 * rng.standard_normal(rx.shape)).astype(np.float32)
    W0 = (0.05 * rng.standard_normal((R, 2, M))).astype(np.float32)
    W0[:, 0, M // 2] += 1.0
    h0 = (0.05 * rng.standard_normal((R, 2, M))).astype(np.float32)
    h0[:, 0, M // 2] += 1.0
    return dict(rx=rx, W0=W0, h0=h0, amp=amp, P=P, amp_mean=amp_mean, var=var, lr=lr)


def run_model(case, data, state=None, steps=None, runs=None, dtype=np.float64):
    """train() for every run of a case -> list of result dicts; state: None or a list of per-run state dicts."""
    runs = range(case["R"]) if runs is None else runs
    steps = case["steps"] if steps is None else steps
    return [train(data["rx"][r], data["W0"][r], data["h0"][r], None if state is None else state[r], steps, case["B"], data["amp"], data["P"][r],
                  data["amp_mean"][r], data["var"][r], data["lr"][r], case["sps"], dtype) for r in runs]


_MODEL = {}


def model(case):
    """(inputs, fresh-start model of every run) of a case, computed once per process and shared; callers leave both unchanged."""
    if case["id"] not in _MODEL:
        data = build(case)
        _MODEL[case["id"]] = (data, run_model(case, data))
    return _MODEL[case["id"]]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), 1e-300))


# A quarter of what the suite allows each quantity against the reference (tests/test_awgn_kernel_gpu.py): a case is float32-conditioned when the
# float32 evaluation of the model itself stays within these of the float64 model, which leaves a float32 kernel room below the same ceilings.
GAP_LIMIT = {"first y": 5e-7, "first q": 1.25e-4, "first loss": 2.5e-6, "first gW": 5e-5, "first gh": 5e-6,
             "loss": 5e-6, "taps": 5e-6, "m": 2.5e-5, "v": 2.5e-5, "x": 2.5e-5, "q": 1.25e-4, "gW": 5e-5, "gh": 5e-6}


def held(case):
    """The quantities of GAP_LIMIT in which a case must be float32-conditioned: all of them, but for the steep demapper (see build) neither the
    moments nor q and the gradients of the later steps."""
    return [k for k in GAP_LIMIT if not (case["edge"] == "steep" and k in ("m", "v", "x", "q", "gW", "gh"))]


def loss_err(got, want):
    """The largest relative error of the per-step losses; a loss within 1 of zero is taken absolutely.  The loss nm log C + KL is a difference of
    terms of either sign, and at the shortest minibatches (B = M at one sample per symbol: one residual sample, nm = 1) it is of order 1 and
    crosses zero from step to step and seed to seed, where an error relative to the loss itself measures nothing."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1.0)))


def float32_gap(case, data, models):
    """How far float32 arithmetic alone takes the training loop of a case from its float64 model: the largest error, over the runs, of the
    float32 evaluation of the model (same code, float32 tensors and state) per quantity, measured as the kernels are (relerr of y and the
    gradients at the first step, max abs error of q, relative error of the losses, max abs error of the conditioned taps, relerr of the moments and
    of the last step's gradients).
    Where the loop amplifies rounding noise (a tap group whose whole gradient vanishes, a demapper so steep that the trajectory forks), this
    gap is large whatever the implementation, and the case cannot tell a right kernel from a wrong one."""
    B = case["B"]
    gap = {k: 0.0 for k in GAP_LIMIT}
    up = lambda k, v: gap.__setitem__(k, max(gap[k], float(v)))
    for m, f in zip(models, run_model(case, data, dtype=np.float32)):
        up("first y", _rel(f["y"][:, :B], m["y"][:, :B]))
        up("first q", np.max(np.abs(f["q"][:, :B] - m["q"][:, :B])))
        up("first loss", loss_err(f["loss"][:1], m["loss"][:1]))
        up("first gW", _rel(f["gW"][0], m["gW"][0]))
        up("first gh", _rel(f["gh"][0], m["gh"][0]))
        up("loss", loss_err(f["loss"], m["loss"]))
        up("q", np.max(np.abs(f["q"] - m["q"])))
        up("gW", _rel(f["gW"][-1], m["gW"][-1]))
        up("gh", _rel(f["gh"][-1], m["gh"][-1]))
        for grp in ("W", "h"):
            up("taps", np.abs(f[grp] - m[grp])[conditioned(m["g" + grp])].max())
            for k in ("m", "v", "x"):
                up(k, _rel(f[k + grp], m[k + grp]))
    return gap


def old_state(case, data, step, seed=0):
    """A plausible old optimiser state per run (for a run whose step counter stands at `step`): the moments the recursion leaves after `step`
    steps on gradients of the magnitude the case's first minibatch gives, g_i = g (0.6 + 0.4 N(0, 1)) per entry, with the AMSGrad maximum kept
    along the way (so x >= v, and x > v where v has fallen since)."""
    rng = np.random.default_rng(seed + step)
    fresh = model(case)[1]
    out = []
    for r in range(case["R"]):
        st = {"step": step}
        for grp, key in (("W", "gW"), ("h", "gh")):
            g0 = fresh[r][key][0]
            m, v, x = np.zeros_like(g0), np.zeros_like(g0), np.zeros_like(g0)
            for i in range(step):
                g = g0 * (0.6 + 0.4 * rng.standard_normal(g0.shape)) * (1.5 if i < step // 2 else 1.0)
                m = BETA1 * m + (1 - BETA1) * g
                v = BETA2 * v + (1 - BETA2) * g * g
                x = np.maximum(x, v)
            st["m" + grp], st["v" + grp], st["x" + grp] = m.astype(np.float32), v.astype(np.float32), x.astype(np.float32)
        out.append(st)
    return out


def binding_state(case, data, step=50):
    """A state whose AMSGrad maximum binds on half of the entries: m = g / 2, v = g^2 (0.5 .. 1.5) from the first minibatch's gradients, and
    x = 3 v on the even entries (the maximum stays x: the update divides by sqrt(x), not sqrt(v)), x = 0.3 v on the odd ones (the maximum becomes
    the new v, and must be stored)."""
    rng = np.random.default_rng(step)
    fresh = model(case)[1]
    out = []
    for r in range(case["R"]):
        st = {"step": step}
        for grp, key in (("W", "gW"), ("h", "gh")):
            g0 = fresh[r][key][0]
            v = g0 * g0 * rng.uniform(0.5, 1.5, g0.shape)
            x = v * np.where(np.arange(g0.size).reshape(g0.shape) % 2 == 0, 3.0, 0.3)
            st["m" + grp], st["v" + grp], st["x" + grp] = (0.5 * g0).astype(np.float32), v.astype(np.float32), x.astype(np.float32)
        out.append(st)
    return out

"""Float64 numpy model of vaeq_cma_epilogue_info: the figures of tests/_ref_info.py (AIR, GMI, NGMI, pre-FEC BER, counts) of one frame of the
constant-modulus DP baselines, composed of what is already there:

    normalise(y, tx, shift_c, r_c)   tests/_ref_epilogue.py's align by the constellation stage, then the mean-radius normalisation of the window
                                     W_c = [11, N - 11 - max|shift_c|): fac = sum |tx| / sum |ya| over W_c and both polarisations, ya scaled by fac
                                     inside W_c and left as it is outside (the reference normalises a slice view in place, shared_funcs.py:242)
    _ref_info.info_y(yn, ...)        on that sequence, with the soft-demapper stage's shift_q / r_q and no per-minibatch cut.

A run whose sum of |ya| over W_c is zero has no normalisation: NaN figures, zero counts.

Test infrastructure only.  The input builder plants levels as _ref_info.make_run does, passes them through the stage-q channel, divides the W_c part
by a scale s, passes that through the stage-c channel and casts to float32: the samples outside W_c stay at constellation scale, so a kernel that
scaled them too would move them across thresholds.  MIN_POST_FLOOR is a q-mode precondition and does not apply (the posteriors are recomputed in
the log domain: a wrong symbol costs its true several hundred bits); QGAP_FLOOR does.
"""
import functools

import numpy as np

import _ref_epilogue as E
import _ref_info as I

CMA_DEV = 4.4e-6                                                               # bit: bounds float32_deviation over the launches below (test_ref_cma_info_host.py prints the maximum)
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")


def window_c(N, shift_c):
    return slice(E.EDGE, N - E.EDGE - int(np.max(np.abs(shift_c))))


def normalise(y, tx, shift_c, r_c):
    """y[2,2,N], tx[2,2,N] -> (yn[2,2,N] float64: aligned by (shift_c, r_c), W_c scaled by fac; fac, NaN when the radius sum is zero)."""
    ya = E.align(np.asarray(y, np.float64), shift_c, r_c)
    W = window_c(ya.shape[-1], shift_c)
    t = np.asarray(tx, np.float64)[..., W]
    st, sy = np.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2).sum(), np.sqrt(ya[:, 0, W] ** 2 + ya[:, 1, W] ** 2).sum()
    if sy == 0:
        return ya, float("nan")
    yn = ya.copy()
    yn[..., W] *= st / sy
    return yn, float(st / sy)


def info(y, tx, P, amp, nu_sc, var, shift_c, r_c, shift_q, r_q):
    yn, fac = normalise(y, tx, shift_c, r_c)
    if np.isnan(fac):
        z = np.zeros(2, np.int64)
        nan = np.full(2, np.nan)
        return dict(AIR=nan, GMI=nan, NGMI=nan, BER=nan, kept=z, sym_err=z, bit_err=z, hyp=z, min_post=np.inf, qgap=np.inf, fac=fac)
    m = I.info_y(yn, tx, P, amp, nu_sc, var, shift_q, r_q, None)
    m["fac"] = fac
    return m


# ------------------------------------------------------------------ inputs
def make_run(seed, N, n, shift_c, r_c, shift_q, r_q, hyp, s, nu, var, n_err, scale_edges=False):
    """One run whose stage-c aligned, window-normalised sequence carries the TX levels under hypothesis hyp (n_err[p] wrong symbols of polarisation p
    inside the stage-q window, jitter of at most a fifth of half the level spacing), delayed by shift_q and exchanged by r_q; its W_c part is
    divided by s, and the whole is delayed by shift_c and exchanged by r_c.  scale_edges: the samples outside W_c are divided by s too (what the
    grid must be able to tell apart)."""
    rng = np.random.default_rng(seed)
    amp = E.amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2
    P = I.pmf(n, nu)
    lev = rng.choice(n, size=(2, 2, N), p=P)
    tx = amp[lev].astype(np.float16)
    pool = E.kept_indices(N, shift_q, None)
    rxl = lev.copy()
    for p in range(2):
        for pos in rng.choice(pool, size=min(n_err[p], len(pool)), replace=False):
            c = int(rng.integers(2))
            rxl[p, c, pos] = rng.choice([v for v in range(n) if v != rxl[p, c, pos]])
    dI, dQ = I.unrotate(rxl[:, 0], rxl[:, 1], hyp, S)
    rcv = np.stack([dI, dQ], axis=1)
    clean = amp[rcv].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rcv.shape)
    ya = I.channel(clean, r_q, np.asarray(shift_q))                             # the sequence the soft demapper sees, at constellation scale
    if scale_edges:
        ya = ya / s
    else:
        ya[..., window_c(N, shift_c)] /= s
    y = I.channel(ya, r_c, np.asarray(shift_c)).astype(np.float32)
    nu_sc = np.float32(nu / float(np.min(np.abs(amp))) ** 2)
    return dict(y=y, tx=tx, amp=amp, P=P.astype(np.float32), nu_sc=nu_sc, var=np.asarray(var, np.float32), shift_c=np.asarray(shift_c, np.int64),
                r_c=int(r_c), shift_q=np.asarray(shift_q, np.int64), r_q=int(r_q), hyp=hyp, n=n, s=s, n_err=tuple(n_err))


def model(x):
    return info(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift_c"], x["r_c"], x["shift_q"], x["r_q"])


def build_run(seed, **kw):
    """The seed is advanced (at most 200 times) until the model's top-two posterior gap meets QGAP_FLOOR and the model recovers the planted symbol
    errors and hypothesis (at N <= 47 a few planted errors move the mean radius, so fac can miss s by enough to add an error): the floor is
    never lowered, and a case never depends on a lucky draw."""
    for sd in range(seed, seed + 200):
        x = make_run(sd, **kw)
        m = model(x)
        if m["qgap"] >= E.QGAP_FLOOR and planted_recovered(x, m):
            return x, m
    raise RuntimeError(f"no seed in [{seed}, {seed + 200}) meets QGAP_FLOOR for {kw}")


def planted_recovered(x, m):
    return all(int(m["sym_err"][p]) == min(x["n_err"][p], int(m["kept"][p])) and int(m["hyp"][p]) == x["hyp"] for p in range(2))


# one entry = one kernel launch of R = 3 runs: the smallest row, an odd one, and one beyond 4 x 256 symbols
LENGTHS = (43, 47, 400, 1030)
SHIFTS_C = [(-10, 0), (0, 10), (10, -10)]
SHIFTS_Q = [(0, 0), (2, -1), (-3, 3)]
SCALES = (0.8, 1.25, 0.6)


@functools.lru_cache(maxsize=None)
def launches():
    L = {}
    for i, N in enumerate(LENGTHS):
        for j, n in enumerate((2, 4, 8)):
            runs = []
            for k in range(3):
                # r_c: the reference applies shift[p] of the row it measured to the row the exchange puts there, so with unequal shifts the epilogue
                # finds a planted alignment only at r_c = 0 -- the runs with a zero stage-q shift and r_q = 0 (compared with the epilogue) have that
                sq = (i + j + k) % 3
                runs.append(dict(seed=12000 + 100 * i + 10 * j + k, N=N, n=n, shift_c=SHIFTS_C[k], r_c=(i + k + (sq == 1)) % 2, shift_q=SHIFTS_Q[sq],
                                 r_q=(i + k) % 2, hyp=(3 * i + 5 * j + k) % 8, s=SCALES[k], nu=(0.0, I.NU_SHAPED, I.NU_SHAPED)[(k + j) % 3],
                                 var=(0.003 + 0.001 * k, 0.006 - 0.001 * j), n_err=(1 + k, 4 - k)))
            L[f"N{N}-n{n}"] = runs
    return L


LAUNCHES = list(launches())


@functools.lru_cache(maxsize=None)
def build_launch(name):
    """-> (per-run inputs, per-run model results); built once, shared by the tests, never modified."""
    xs, ms = [], []
    for spec in launches()[name]:
        x, m = build_run(**spec)
        for v in x.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        xs.append(x)
        ms.append(m)
    return xs, ms


def _radius_sum(rad, lo):
    """cma_radius_factor's order in float32: rad[2][len(W_c)] radii of the window that starts at index lo; thread t adds its indices t, t + 256, ...
    in turn, both polarisations of an index one after the other, then the threads are added."""
    f = np.float32
    per = np.zeros(256, f)
    for i in range(rad.shape[-1]):
        t = (lo + i) % 256
        per[t] = f(f(per[t] + rad[0, i]) + rad[1, i])
    return per.sum(dtype=f)


def float32_deviation(x, ordered=False):
    """What the float32 format costs: the kernel's operation order (fac from float32 sums of float32 radii, the scaled sample, the soft demapper's
    exponent, a log-sum-exp per bit-wise set around its own maximum, per-symbol terms, mean) evaluated in numpy float32 under the model's hypothesis,
    against the float64 model.  ordered: the radii are summed per thread at stride 256 and then over the threads (the kernel's documented order:
    what decides fac at short windows) and not by numpy's pairwise sum.  -> largest |AIR or GMI deviation| of the run in bit, None where
    nothing is kept."""
    f = np.float32
    n, S = x["n"], x["n"] - 1
    b = int(round(np.log2(n)))
    m = model(x)
    N = x["y"].shape[-1]
    ya = E.align(np.asarray(x["y"], f), x["shift_c"], x["r_c"])
    W = window_c(N, x["shift_c"])
    t = np.asarray(x["tx"], f)[..., W]
    rt = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]).astype(f)).astype(f)
    ry = np.sqrt((ya[:, 0, W] * ya[:, 0, W] + ya[:, 1, W] * ya[:, 1, W]).astype(f)).astype(f)
    st, sy = (_radius_sum(rt, W.start), _radius_sum(ry, W.start)) if ordered else (rt.sum(dtype=f), ry.sum(dtype=f))
    if sy == 0 or not m["kept"].any():
        return None
    yn = ya.copy()
    yn[..., W] = (yn[..., W] * f(st / sy)).astype(f)
    amp, var, nusc, l2e = x["amp"].astype(f), x["var"].astype(f), f(x["nu_sc"]), f(1.4426950408889634)
    z = np.empty((2, 2, n, N), f)
    for sp in range(2):
        i2v = f(0.5) / var[sp]
        for i in range(n):
            dd = (yn[sp] - amp[i]).astype(f)
            z[sp, :, i] = (-((dd * dd).astype(f) * i2v + f(nusc * f(amp[i] * amp[i]))).astype(f) * l2e).astype(f)
    za = E.window(E.align(z.reshape(2, 2 * n, -1), x["shift_q"], x["r_q"]), x["shift_q"], None).reshape(2, 2, n, -1)
    lev = E.window(E.tx_levels(x["tx"], n), x["shift_q"], None)
    K = za.shape[-1]
    g, H, worst = I.gray(np.arange(n)), f(I.entropy(x["P"])), 0.0
    for p in range(2):
        h = int(m["hyp"][p])
        tQ = S - lev[p, 1] if h >> 2 else lev[p, 1]
        (zI, zQ), _ = I._apply(za[p], np.zeros((2, K), np.int64), h, S)
        a, gg = np.zeros(K, f), np.zeros(K, f)
        for zz, tl in ((zI, lev[p, 0]), (zQ, tQ)):
            def lse(mask):
                w = np.where(mask, zz, f(-np.inf)).astype(f)
                mx = w.max(0)
                return (mx + np.log2(np.exp2((w - mx).astype(f)).astype(f).sum(0, dtype=f)).astype(f)).astype(f)
            bit0 = (g & 1)[:, None]
            l0, l1 = lse(bit0 == 0), lse(bit0 == 1)
            hi, lo = np.maximum(l0, l1), np.minimum(l0, l1)
            tot = (hi + np.log2(f(1) + np.exp2((lo - hi).astype(f)).astype(f)).astype(f)).astype(f)
            a = (a + (zz[tl, np.arange(K)] - tot).astype(f)).astype(f)
            gs = np.zeros(K, f)
            for k in range(b):
                gs = (gs + lse(((g >> k) & 1)[:, None] == ((g[tl] >> k) & 1)[None, :])).astype(f)
            gg = (gg + (gs - f(b) * tot).astype(f)).astype(f)
        air, gmi = f(f(2) * H + f(a.sum(dtype=f) / f(K))), f(f(2) * H + f(gg.sum(dtype=f) / f(K)))
        worst = max(worst, abs(float(air) - m["AIR"][p]), abs(float(gmi) - m["GMI"][p]))
    return worst

"""Float64 numpy model of vaeq_dp_epilogue_info: achievable rate of symbol-wise mismatched decoding (AIR), generalised mutual information
of the bit-wise decoder (GMI), NGMI and pre-FEC BER of one DP frame, per polarisation, written from the closed-form definitions (the
reference has no such metric).  Roll, polarisation exchange and kept window are tests/_ref_epilogue.py's -- the symbols are exactly the ones
the soft-demapper SER keeps.

Level i of an axis carries the binary-reflected Gray label g(i) = i ^ (i >> 1), b = log2 n bits; H = -sum P log2 P of the run's per-axis pmf.
Hypothesis h = 4 flip + rot, rot in (0, pi, pi/2, 3 pi/2): rot pi maps a decided level d to n-1-d on both axes, rot pi/2 gives
I' = n-1-d_Q, Q' = d_I, rot 3 pi/2 is pi applied to that; flip maps the transmitted Q level t_Q to n-1-t_Q.  The posterior vectors follow the
same index maps.  The hypothesis with the fewest symbol errors of argmax(q) wins, ties to the smallest h.  Under it
    AIR = 2 H + mean[l(q_I[t_I]) + l(q_Q[t_Q])],   GMI = 2 H + mean sum_axis sum_k l(sum_{i: bit_k g(i) = bit_k g(t_axis)} q_axis[i]),
    NGMI = 1 - (2 H - GMI) / (2 b),   BER = bit_err / (2 b kept),
l(x) = log2 max(x, FLT_MIN) on a stored q (q-mode), an exact log-softmax of the soft demapper's exponent when the posteriors are recomputed
from y (y-mode).  Nothing kept: NaN figures, zero counts.

Test infrastructure only.  Besides the figures and the integer counts the model returns what makes the comparison with a float32 kernel
fair: `min_post`, the smallest posterior at a transmitted level it took a log of (float32 and float64 logs agree above 1e-30), and `qgap`,
the smallest gap between the two largest posteriors of a kept symbol and axis (the decisions of a float32 demapper are the model's above
tests/_ref_epilogue.py's QGAP_FLOOR).
"""
import functools

import numpy as np

import _ref_epilogue as E

FLT_MIN = float(np.finfo(np.float32).tiny)
MIN_POST_FLOOR = 1e-30
Y_DEV = 1.3e-5                                                                 # bit: largest y-mode deviation recorded on the GPU cases
NU_SHAPED = 0.1222578                                                          # the strongest shaping of the PCS-64-QAM sweep (4.125 bit)


def gray(i):
    i = np.asarray(i, np.int64)
    return i ^ (i >> 1)


def entropy(P):
    P = np.asarray(P, np.float64)
    nz = P > 0
    return float(-(P[nz] * np.log2(P[nz])).sum())


def _hyp_maps(h, S):
    """-> (axis, reversed) of the I' and of the Q' posterior, and the decision maps, of hypothesis h."""
    rot = h & 3
    return [((0, False), (1, False)), ((0, True), (1, True)), ((1, True), (0, False)), ((1, False), (0, True))][rot]


def _apply(lp, dec, h, S):
    """lp[2][n][K] (log2 posteriors or posteriors, axis 0 = I, 1 = Q), dec[2][K] -> the hypothesis's (lp', dec')."""
    (cI, rI), (cQ, rQ) = _hyp_maps(h, S)
    lpI = lp[cI][::-1] if rI else lp[cI]
    lpQ = lp[cQ][::-1] if rQ else lp[cQ]
    dI = S - dec[cI] if rI else dec[cI]
    dQ = S - dec[cQ] if rQ else dec[cQ]
    return (lpI, lpQ), (dI, dQ)


def _figures(post, logdom, lev, P, n):
    """post[2 pol][2 axis][n][K] kept, aligned posteriors (logdom: log2 of them, unnormalised or not), lev[2][2][K] TX levels."""
    S, b = n - 1, int(round(np.log2(n)))
    H = entropy(P)
    K = post.shape[-1]
    out = dict(AIR=np.full(2, np.nan), GMI=np.full(2, np.nan), NGMI=np.full(2, np.nan), BER=np.full(2, np.nan),
               kept=np.full(2, K if K else 0, np.int64), sym_err=np.zeros(2, np.int64), bit_err=np.zeros(2, np.int64), hyp=np.zeros(2, np.int64),
               cnt=np.zeros((8, 2), np.int64), min_post=np.inf, qgap=np.inf)
    if K == 0:
        return out
    if logdom:                                                                # exact log-softmax, float64
        mx = post.max(2, keepdims=True)
        lp = post - (mx + np.log2(np.exp2(post - mx).sum(2, keepdims=True)))
        lin = np.exp2(lp)
    else:
        lin = post
        lp = np.log2(np.maximum(post, FLT_MIN))
    srt = np.sort(lin, axis=2)
    out["qgap"] = float((srt[:, :, -1] - srt[:, :, -2]).min())
    dec = lin.argmax(2)                                                       # [2][2][K], first maximum
    bits = (gray(np.arange(n))[:, None] >> np.arange(b)[None, :]) & 1         # [n][b]
    for p in range(2):
        tI = lev[p, 0]
        res = []
        for h in range(8):
            tQ = S - lev[p, 1] if h >> 2 else lev[p, 1]
            (dI, dQ) = _apply(lin[p], dec[p], h, S)[1]
            res.append(int(((dI != tI) | (dQ != tQ)).sum()))
        out["cnt"][:, p] = res
        h = int(np.argmin(res))                                               # ties: the smallest h
        tQ = S - lev[p, 1] if h >> 2 else lev[p, 1]
        (lpI, lpQ), (dI, dQ) = _apply(lp[p], dec[p], h, S)
        (liI, liQ), _ = _apply(lin[p], dec[p], h, S)
        air = gmi = 0.0
        for lpa, lia, t in ((lpI, liI, tI), (lpQ, liQ, tQ)):
            k_idx = np.arange(K)
            air = air + lpa[t, k_idx]
            out["min_post"] = min(out["min_post"], float(lia[t, k_idx].min()))
            for k in range(b):
                same = bits[:, k][:, None] == bits[t, k][None, :]              # [n][K]: levels whose bit k equals the transmitted level's
                if logdom:
                    z = np.where(same, lpa, -np.inf)
                    m = z.max(0)
                    gmi = gmi + m + np.log2(np.exp2(z - m).sum(0))
                else:
                    gmi = gmi + np.log2(np.maximum(np.where(same, lia, 0.0).sum(0), FLT_MIN))
        out["AIR"][p] = 2 * H + air.mean()
        out["GMI"][p] = 2 * H + gmi.mean()
        out["NGMI"][p] = 1 - (2 * H - out["GMI"][p]) / (2 * b)
        out["hyp"][p], out["sym_err"][p] = h, res[h]
        out["bit_err"][p] = int(sum(bin(int(v)).count("1") for v in (gray(dI) ^ gray(tI))) + sum(bin(int(v)).count("1") for v in (gray(dQ) ^ gray(tQ))))
        out["BER"][p] = np.float32(out["bit_err"][p]) / np.float32(2 * b * K)
    return out


def _kept(arr, shift, r, batch_len):
    return E.window(E.align(np.asarray(arr), shift, r), shift, batch_len)


def info_q(q, tx, P, shift, r, batch_len=None):
    """q-mode: q[2][2n][N] as stored (float32 values, evaluated in float64), tx[2][2][N], P[n], shift[2], r."""
    n = len(P)
    N = q.shape[-1]
    lev = E.window(tx_levels(tx, n), shift, batch_len)
    qa = _kept(np.asarray(q, np.float64), shift, r, batch_len).reshape(2, 2, n, -1)
    return _figures(qa, False, lev, P, n)


def info_y(y, tx, P, amp, nu_sc, var, shift, r, batch_len=None):
    """y-mode: the posteriors are the soft demapper's (softmax_i(-(y - a_i)^2 / (2 var_p) - nu_sc a_i^2) with the RECEIVED polarisation's
    var), evaluated in float64 in the log domain from the float32 y."""
    n = len(P)
    a = np.asarray(amp, np.float64)
    y = np.asarray(y, np.float64)
    z = -(y[:, :, None, :] - a[None, None, :, None]) ** 2 / (2 * np.asarray(var, np.float64)[:, None, None, None]) \
        - float(nu_sc) * (a ** 2)[None, None, :, None]
    z = z * np.log2(np.e)                                                     # [2][2][n][N], log2 of the unnormalised posterior
    lev = E.window(tx_levels(tx, n), shift, batch_len)
    za = _kept(z.reshape(2, 2 * n, -1), shift, r, batch_len).reshape(2, 2, n, -1)
    return _figures(za, True, lev, P, n)


def tx_levels(tx, n):
    """_ref_epilogue.tx_levels with info_tx_level's clamp to 0 .. n - 1 (a TX sample beyond the outer level is the outer level)."""
    return np.clip(E.tx_levels(tx, n), 0, n - 1)


# ------------------------------------------------------------------ inputs
def pmf(n, nu):
    """The per-axis PCS pmf of shared_funcs.py:566-568 (nu scales the squared level in units of the innermost one)."""
    lev = np.arange(-(n - 1), n, 2).astype(np.float64)
    p = np.exp(-nu * lev ** 2)
    return p / p.sum()


def unrotate(LI, LQ, h, S):
    """Received levels (d_I, d_Q) that hypothesis h = 4 flip + rot decodes to (LI, LQ)."""
    Qf = S - LQ if h >> 2 else LQ
    return [(LI, Qf), (S - LI, S - Qf), (Qf, S - LI), (S - Qf, LI)][h & 3]


def channel(seq, r, shift):
    """seq[2,C,N] in TX order -> what E.align(., shift, r) undoes: polarisations exchanged by r, the row that ends up as polarisation p
    delayed by shift[p]."""
    s = np.roll(seq, r, axis=0)
    d = shift[::-1] if r else shift
    return np.stack([np.roll(s[0], int(d[0]), axis=-1), np.roll(s[1], int(d[1]), axis=-1)])


def make_run(seed, N, n, shift, r, hyp, batch_len, nu, var, n_err, P=None):
    """One run whose q AND y carry the TX levels (with n_err[p] wrong symbols in polarisation p, each axis error to a random other level)
    under hypothesis hyp, rolled by shift and exchanged by r.  q: top posterior 0.55 .. 0.9 at the received level, the rest spread
    over the other levels (none below 1e-3); y: the received level's amplitude plus up to a fifth of half the level spacing.  P: the per-axis
    pmf the TX levels are drawn from and the run reports, where it is not pmf(n, nu) (zero entries allowed)."""
    rng = np.random.default_rng(seed)
    amp = E.amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2
    P = pmf(n, nu) if P is None else np.asarray(P, np.float64)
    lev = rng.choice(n, size=(2, 2, N), p=P)
    tx = amp[lev].astype(np.float16)
    pool = E.kept_indices(N, shift, batch_len)
    rxl = lev.copy()
    for p in range(2):
        for pos in (rng.choice(pool, size=min(n_err[p], len(pool)), replace=False) if len(pool) else []):
            c = int(rng.integers(2))
            rxl[p, c, pos] = rng.choice([v for v in range(n) if v != rxl[p, c, pos]])
    dI, dQ = unrotate(rxl[:, 0], rxl[:, 1], hyp, S)
    rcv = np.stack([dI, dQ], axis=1)
    top = rng.uniform(0.55, 0.9, rcv.shape)
    rest = rng.uniform(0.2, 1.0, rcv.shape[:2] + (n,) + rcv.shape[2:])
    np.put_along_axis(rest, rcv[:, :, None, :], 0.0, axis=2)
    rest *= ((1 - top) / rest.sum(2))[:, :, None, :]
    np.put_along_axis(rest, rcv[:, :, None, :], top[:, :, None, :], axis=2)
    clean = amp[rcv].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rcv.shape)
    q = channel(rest.reshape(2, 2 * n, N), r, shift).astype(np.float32)
    y = channel(clean, r, shift).astype(np.float32)
    nu_sc = np.float32(nu / float(np.min(np.abs(amp))) ** 2)
    return dict(q=q, y=y, tx=tx, amp=amp, P=P.astype(np.float32), nu_sc=nu_sc, var=np.asarray(var, np.float32), shift=np.asarray(shift, np.int64),
                r=int(r), batch_len=batch_len, hyp=hyp, n=n)


# one entry = one kernel launch of R = 3 runs: the compact kernel's tile edges 43 and 47, one minibatch geometry at both cuts, one tile boundary
SHAPES = [(43, None), (47, None), (400, None), (400, 20), (400, 100), (1030, None)]
SHIFTS = [(-10, 0), (0, 10), (10, -10)]


@functools.lru_cache(maxsize=None)
def launches():
    L = {}
    for i, (N, B) in enumerate(SHAPES):
        for j, n in enumerate((2, 4, 8)):
            runs = []
            for k, sh in enumerate(SHIFTS):
                runs.append(dict(seed=9000 + 100 * i + 10 * j + k, N=N, n=n, shift=sh, r=(i + j + k) % 2, hyp=(3 * i + 5 * j + k) % 8, batch_len=B,
                                 nu=(0.0, NU_SHAPED, NU_SHAPED)[(k + j) % 3], var=(0.003 + 0.001 * k, 0.006 - 0.001 * j), n_err=(1 + k, 4 - k)))
            L[f"N{N}-B{B or 0}-n{n}"] = runs
    return L


LAUNCHES = list(launches())


@functools.lru_cache(maxsize=None)
def build_launch(name):
    """-> (per-run inputs, per-run q-mode model results, per-run y-mode model results); built once, shared by the tests, never modified."""
    xs, mq, my = [], [], []
    for spec in launches()[name]:
        x = make_run(**spec)
        for v in x.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        xs.append(x)
        mq.append(info_q(x["q"], x["tx"], x["P"], x["shift"], x["r"], x["batch_len"]))
        my.append(info_y(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], x["batch_len"]))
    return xs, mq, my


def y_mode_float32_deviation(x):
    """What the float32 format costs y-mode: the kernel's operation order (the soft demapper's exponent, log-sum-exp of every bit-wise set around
    its own maximum, per-symbol terms, mean) evaluated in numpy float32 under the model's hypothesis, against the float64 model.
    -> largest |AIR or GMI deviation| of the run in bit, None when nothing is kept."""
    f = np.float32
    n, S = x["n"], x["n"] - 1
    b = int(round(np.log2(n)))
    amp, y, var, nusc, l2e = x["amp"].astype(f), x["y"], x["var"].astype(f), f(x["nu_sc"]), f(1.4426950408889634)
    z = np.empty((2, 2, n, y.shape[-1]), f)
    for sp in range(2):
        i2v = f(0.5) / var[sp]
        for i in range(n):
            dd = (y[sp] - amp[i]).astype(f)
            z[sp, :, i] = (-((dd * dd).astype(f) * i2v + f(nusc * f(amp[i] * amp[i]))).astype(f) * l2e).astype(f)
    za = _kept(z.reshape(2, 2 * n, -1), x["shift"], x["r"], x["batch_len"]).reshape(2, 2, n, -1)
    lev = E.window(tx_levels(x["tx"], n), x["shift"], x["batch_len"])
    K = za.shape[-1]
    if K == 0:
        return None
    m = info_y(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], x["batch_len"])
    g, H, worst = gray(np.arange(n)), f(entropy(x["P"])), 0.0
    for p in range(2):
        h = int(m["hyp"][p])
        tQ = S - lev[p, 1] if h >> 2 else lev[p, 1]
        (zI, zQ), _ = _apply(za[p], np.zeros((2, K), np.int64), h, S)
        a, gg = np.zeros(K, f), np.zeros(K, f)
        for zz, t in ((zI, lev[p, 0]), (zQ, tQ)):
            def lse(mask):
                w = np.where(mask, zz, f(-np.inf)).astype(f)
                mx = w.max(0)
                return (mx + np.log2(np.exp2((w - mx).astype(f)).astype(f).sum(0, dtype=f)).astype(f)).astype(f)
            bit0 = (g & 1)[:, None]
            l0, l1 = lse(bit0 == 0), lse(bit0 == 1)
            hi, lo = np.maximum(l0, l1), np.minimum(l0, l1)
            tot = (hi + np.log2(f(1) + np.exp2((lo - hi).astype(f)).astype(f)).astype(f)).astype(f)
            a = (a + (zz[t, np.arange(K)] - tot).astype(f)).astype(f)
            gs = np.zeros(K, f)
            for k in range(b):
                gs = (gs + lse(((g >> k) & 1)[:, None] == ((g[t] >> k) & 1)[None, :])).astype(f)
            gg = (gg + (gs - f(b) * tot).astype(f)).astype(f)
        air, gmi = f(f(2) * H + f(a.sum(dtype=f) / f(K))), f(f(2) * H + f(gg.sum(dtype=f) / f(K)))
        worst = max(worst, abs(float(air) - m["AIR"][p]), abs(float(gmi) - m["GMI"][p]))
    return worst

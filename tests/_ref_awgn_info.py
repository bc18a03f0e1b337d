"""Float64 numpy model of vaeq_awgn_info: achievable rate of symbol-wise mismatched decoding (AIR), generalised mutual information of the
bit-wise decoder (GMI), NGMI and pre-FEC BER of one AWGN validation frame, per run, written from the closed-form definitions (the reference
has no such metric).

Per run, n levels per axis, S = n - 1, b = log2 n.  Level i carries the Gray label g(i) = i ^ (i >> 1); H = -sum P log2 P of the per-axis pmf (a
zero entry contributes 0).
Window (SER_q's, func_VAELE_MQAM_shaping.py:318: q[:, 11+sh : -11] against data[:, 11 : -11-sh]): kept symbol j in [0, len), len = N - 22 - sh,
pairs the posterior or sample 11 + sh + j with the TX symbol 11 + j; empty when 11 + sh <= 0 or len <= 0.
TX level t = clamp(rint(S/2 tx + S/2), 0, S) per axis; decision d_c = first maximum of the posterior of axis c.
Hypothesis h in (0, 1, 2, 3) = rotation by 0, pi, pi/2, 3 pi/2: (d_I', d_Q') = (d_I, d_Q), (S - d_I, S - d_Q), (S - d_Q, d_I), (d_Q, S - d_I); the
posterior vectors follow the same index maps.  The hypothesis with the fewest symbol errors wins, ties to the smallest h.  Under it
    AIR = 2 H + mean[l(q_I'[t_I]) + l(q_Q'[t_Q])],   GMI = 2 H + mean sum_axis sum_k l(sum_{i: bit_k g(i) = bit_k g(t_axis)} q_axis'[i]),
    NGMI = 1 - (2 H - GMI) / (2 b),   BER = bit_err / (2 b kept),   bit_err = sum popcount(g(d') ^ g(t)) over both axes,
l(x) = log2 max(x, FLT_MIN) on a stored q (q-mode), an exact log-softmax in y-mode.  Nothing kept: NaN figures, zero counts.
y-mode posteriors (:228-229): m_c = sum_{n<N} |y_c[n]| / N over the whole row, yhat_c = y_c (amp_mean / m_c), z_i = -(yhat_c - a_i)^2 / var,
posteriors = softmax of z.  A component with m_c == 0 has no normalisation: the empty-window result.

Test infrastructure only.  Besides the figures and the integer counts the model returns what makes the comparison with a float32 kernel fair:
`margin`, the least distance of any normalised yhat of the WHOLE row to a decision threshold in units of the level spacing (y-mode; above
MARGIN_FLOOR a float32 demapper, and the validation kernel's rounding decision, decide as the model does), `min_post`, the smallest posterior
at a transmitted level it took a log of, and `qgap`, the smallest gap between the two largest posteriors of a kept symbol and axis.
"""
import functools
import itertools

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
EDGE = 11
MIN_POST_FLOOR = 1e-30                                                         # float32 and float64 logs agree above it
QGAP_FLOOR = 0.05
MARGIN_FLOOR = 0.05
# bit: the largest deviation of y_mode_float32 (the kernel's operation order in numpy float32) from the float64 model over the launches
# below, computed on the CPU by tests/test_ref_awgn_info_host.py (1.71e-4), rounded up.  It is set by launch N24-n4 at shift 0: two kept symbols,
# both planted wrong, up to three 16-QAM levels off at var 0.004 -- terms of about -1300 bit, whose float32 spacing is 1.2e-4.  The GPU test
# holds y-mode to three times this.  MEASURED_Y_DEV is the kernel's own largest deviation on the MI355X over the same launches (DESIGN.md
# section 5), recorded beside it and used by nothing.
Y_DEV = 1.8e-4
MEASURED_Y_DEV = 1.713e-4                                                      # the same launch and run: the figure itself is a float32 near -578
NU_SHAPED = 0.1222578                                                          # the strongest shaping of the PCS-64-QAM sweep
GAINS = (0.7, 1.9)                                                             # per-component gain of the planted y: the normalisation has work to do


def gray(i):
    i = np.asarray(i, np.int64)
    return i ^ (i >> 1)


def entropy(P):
    P = np.asarray(P, np.float64)
    nz = P > 0
    return float(-(P[nz] * np.log2(P[nz])).sum())


def pmf(n, nu):
    """The per-axis PCS pmf (nu scales the squared level in units of the innermost one)."""
    lev = np.arange(-(n - 1), n, 2).astype(np.float64)
    p = np.exp(-nu * lev ** 2)
    return p / p.sum()


def amp_levels(n):
    """The n amplitude levels of one axis of n^2-QAM at unit mean symbol power under a uniform pmf (float32, as the kernels get them)."""
    lev = np.arange(-(n - 1), n, 2).astype(np.float64)
    return (lev / np.sqrt(2 * np.mean(lev ** 2))).astype(np.float32)


def window(N, sh):
    """-> (posterior / sample indices, TX indices) of the kept symbols, both empty when the window is."""
    N, sh = int(N), int(sh)
    ln = N - 2 * EDGE - sh
    if EDGE + sh <= 0 or ln <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    j = np.arange(ln, dtype=np.int64)
    return EDGE + sh + j, EDGE + j


def tx_levels(tx, n):
    S = n - 1
    return np.clip(np.rint(S / 2 * np.asarray(tx, np.float64) + S / 2), 0, S).astype(np.int64)


def _maps(h):
    """-> ((axis, reversed) of the I' posterior, (axis, reversed) of the Q' posterior) under hypothesis h."""
    return [((0, False), (1, False)), ((0, True), (1, True)), ((1, True), (0, False)), ((1, False), (0, True))][h]


def _apply(v, dec, h, S):
    """v[2][n][K] (posteriors or their log2), dec[2][K] -> the hypothesis's ((v_I', v_Q'), (d_I', d_Q'))."""
    (cI, rI), (cQ, rQ) = _maps(h)
    return ((v[cI][::-1] if rI else v[cI], v[cQ][::-1] if rQ else v[cQ]),
            (S - dec[cI] if rI else dec[cI], S - dec[cQ] if rQ else dec[cQ]))


def _empty():
    nan = float("nan")
    return dict(AIR=nan, GMI=nan, NGMI=nan, BER=nan, kept=0, sym_err=0, bit_err=0, hyp=0, cnt=np.zeros(4, np.int64), min_post=np.inf, qgap=np.inf,
                margin=np.inf)


def _figures(post, logdom, lev, P, n):
    """post[2 axis][n][K] kept, aligned posteriors (logdom: log2 of them, unnormalised), lev[2][K] TX levels."""
    S, b = n - 1, int(round(np.log2(n)))
    K = post.shape[-1]
    out = _empty()
    if K == 0:
        return out
    H = entropy(P)
    if logdom:                                                                # exact log-softmax, float64
        mx = post.max(1, keepdims=True)
        lp = post - (mx + np.log2(np.exp2(post - mx).sum(1, keepdims=True)))
        lin = np.exp2(lp)
    else:
        lin = post
        lp = np.log2(np.maximum(post, FLT_MIN))
    srt = np.sort(lin, axis=1)
    out["qgap"] = float((srt[:, -1] - srt[:, -2]).min())
    dec = lin.argmax(1)                                                       # [2][K], first maximum
    tI, tQ = lev
    cnt = [int(((dI != tI) | (dQ != tQ)).sum()) for dI, dQ in (_apply(lin, dec, h, S)[1] for h in range(4))]
    h = int(np.argmin(cnt))                                                   # ties: the smallest h
    (lpI, lpQ), (dI, dQ) = _apply(lp, dec, h, S)
    (liI, liQ), _ = _apply(lin, dec, h, S)
    bits = (gray(np.arange(n))[:, None] >> np.arange(b)[None, :]) & 1         # [n][b]
    k_idx = np.arange(K)
    air, gmi = np.zeros(K), np.zeros(K)
    for lpa, lia, t in ((lpI, liI, tI), (lpQ, liQ, tQ)):
        air = air + lpa[t, k_idx]
        out["min_post"] = min(out["min_post"], float(lia[t, k_idx].min()))
        for k in range(b):
            same = bits[:, k][:, None] == bits[t, k][None, :]                 # [n][K]: the levels whose bit k equals the transmitted level's
            if logdom:
                z = np.where(same, lpa, -np.inf)
                m = z.max(0)
                gmi = gmi + m + np.log2(np.exp2(z - m).sum(0))
            else:
                gmi = gmi + np.log2(np.maximum(np.where(same, lia, 0.0).sum(0), FLT_MIN))
    bit_err = int(sum(bin(int(v)).count("1") for v in gray(dI) ^ gray(tI)) + sum(bin(int(v)).count("1") for v in gray(dQ) ^ gray(tQ)))
    out.update(AIR=2 * H + air.mean(), GMI=2 * H + gmi.mean(), kept=K, sym_err=cnt[h], bit_err=bit_err, hyp=h, cnt=np.array(cnt, np.int64),
               BER=float(np.float32(bit_err) / np.float32(2 * b * K)))
    out["NGMI"] = 1 - (2 * H - out["GMI"]) / (2 * b)
    return out


def info_q(q, tx, P, shift):
    """q-mode: q[2n][N] as stored (float32 values, evaluated in float64), tx[2][N], P[n], shift."""
    n = len(P)
    q = np.asarray(q, np.float64)
    ri, ti = window(q.shape[-1], shift)
    return _figures(q.reshape(2, n, -1)[:, :, ri], False, tx_levels(tx, n)[:, ti], P, n)


def normalised(y, amp_mean):
    """-> yhat[2][N] in float64, or None where a component has no normalisation."""
    y = np.asarray(y, np.float64)
    m = np.abs(y).sum(1) / y.shape[-1]
    if (m == 0).any():
        return None
    return y * (float(amp_mean) / m)[:, None]


def info_y(y, tx, P, amp, amp_mean, var, shift):
    """y-mode: the posteriors are softmax_i(-(yhat_c - a_i)^2 / var), evaluated in float64 in the log domain from the float32 y[2][N]."""
    n = len(P)
    a = np.asarray(amp, np.float64)
    yh = normalised(y, amp_mean)
    if yh is None:
        return _empty()
    z = -(yh[:, None, :] - a[None, :, None]) ** 2 / float(var) * np.log2(np.e)  # [2][n][N], log2 of the unnormalised posterior
    ri, ti = window(yh.shape[-1], shift)
    out = _figures(z[:, :, ri], True, tx_levels(tx, n)[:, ti], P, n)
    thr = (a[1:] + a[:-1]) / 2
    out["margin"] = float(np.abs(yh[:, :, None] - thr[None, None, :]).min() / (a[1] - a[0]))
    return out


# ------------------------------------------------------------------ inputs
def unrotate(LI, LQ, h, S):
    """Received levels (d_I, d_Q) that hypothesis h decodes to (LI, LQ)."""
    return [(LI, LQ), (S - LI, S - LQ), (LQ, S - LI), (S - LQ, LI)][h]


def make_run(seed, N, n, shift, hyp, nu, var, n_err, gain=GAINS, P=None):
    """One run whose q AND y carry the TX levels (drawn from the shaped pmf, with n_err wrong symbols planted inside the window, each an axis
    error to a random other level) un-rotated by hyp and rolled by +shift.  q: top posterior 0.55 .. 0.9 at the received level, the rest spread
    over the other levels (none below 1e-3); y: the received level's amplitude plus up to +-0.2 of half the level spacing, times the
    component's gain.  amp_mean = sum P_i |a_i|.  P: the per-axis pmf where it is not pmf(n, nu) (zero entries allowed)."""
    rng = np.random.default_rng(seed)
    amp = amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2
    P = pmf(n, nu) if P is None else np.asarray(P, np.float64)
    lev = rng.choice(n, size=(2, N), p=P)
    tx = amp[lev].astype(np.float16)
    pool = window(N, shift)[1]
    rxl = lev.copy()
    for pos in (rng.choice(pool, size=min(n_err, len(pool)), replace=False) if len(pool) else []):
        c = int(rng.integers(2))
        rxl[c, pos] = rng.choice([v for v in range(n) if v != rxl[c, pos]])
    rcv = np.stack(unrotate(rxl[0], rxl[1], hyp, S))                          # [2][N]
    top = rng.uniform(0.55, 0.9, rcv.shape)
    rest = rng.uniform(0.2, 1.0, (2, n, N))
    np.put_along_axis(rest, rcv[:, None, :], 0.0, axis=1)
    rest *= ((1 - top) / rest.sum(1))[:, None, :]
    np.put_along_axis(rest, rcv[:, None, :], top[:, None, :], axis=1)
    clean = (amp[rcv].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rcv.shape)) * np.asarray(gain, np.float64)[:, None]
    q = np.roll(rest.reshape(2 * n, N), int(shift), axis=-1).astype(np.float32)
    y = np.roll(clean, int(shift), axis=-1).astype(np.float32)
    return dict(q=q, y=y, tx=tx, amp=amp, P=P.astype(np.float32), amp_mean=np.float32((P * np.abs(amp.astype(np.float64))).sum()),
                var=np.float32(var), shift=int(shift), hyp=int(hyp), n=n, n_err=min(n_err, len(pool)), seed=seed)


def models(x):
    return (info_q(x["q"], x["tx"], x["P"], x["shift"]), info_y(x["y"], x["tx"], x["P"], x["amp"], x["amp_mean"], x["var"], x["shift"]))


def meets_floors(x, mq, my):
    """The preconditions of a fair comparison (tests/test_ref_awgn_info_host.py asserts them for every GPU case)."""
    if not my["margin"] >= MARGIN_FLOOR:
        return False
    if mq["kept"] == 0:
        return True
    if mq["min_post"] < MIN_POST_FLOOR or not (mq["qgap"] > QGAP_FLOOR and my["qgap"] > QGAP_FLOOR):
        return False
    if any(mq[k] != my[k] for k in ("sym_err", "bit_err", "hyp")):           # a short row's scale error put a sample on the wrong side of a threshold
        return False
    if mq["kept"] >= 11:
        return all(m["hyp"] == x["hyp"] and m["sym_err"] == x["n_err"] for m in (mq, my))
    return True


def conditioned_run(spec):
    """make_run(**spec) at the first seed from spec's on that meets every floor (short rows move the sample mean of |y| off amp_mean, and with it
    every yhat towards a threshold: a seed that misses a floor is replaced by the next one, no floor is lowered) -> (x, mq, my)."""
    for seed in itertools.count(spec["seed"]):
        x = make_run(**dict(spec, seed=seed))
        mq, my = models(x)
        if meets_floors(x, mq, my):
            return x, mq, my
        if seed - spec["seed"] > 200:
            raise RuntimeError(f"no seed meets the floors for {spec}")


# one entry = one kernel launch of R = 3 runs with shifts -10 / 0 / +10.  N = 23 keeps 11 / 1 / 0 symbols, 33 keeps 21 / 11 / 1, 257 puts one symbol
# in the second round of a 256-thread workgroup (shift -10: 245 kept; the row pass for m_c has it at every shift), 1030 and 2100 straddle the
# 1000-symbol shift-search length
SIZES = (23, 24, 33, 60, 257, 1030, 2100)
SHIFTS = (-10, 0, 10)
VARS = (0.004, 0.0063, 0.01)


@functools.lru_cache(maxsize=None)
def launches():
    L = {}
    for i, N in enumerate(SIZES):
        for j, n in enumerate((2, 4, 8)):
            L[f"N{N}-n{n}"] = [dict(seed=20000 + 1000 * i + 300 * j + 100 * k, N=N, n=n, shift=sh, hyp=(i + 2 * j + k) % 4,
                                    nu=(0.0, NU_SHAPED)[(i + j + k) % 2], var=VARS[(i + j + k) % 3], n_err=1 + (i + k) % 3)
                               for k, sh in enumerate(SHIFTS)]
    return L


LAUNCHES = list(launches())


@functools.lru_cache(maxsize=None)
def build_launch(name):
    """-> (per-run inputs, per-run q-mode model results, per-run y-mode model results); built once, shared by the tests, never modified."""
    xs, mq, my = [], [], []
    for spec in launches()[name]:
        x, a, b = conditioned_run(spec)
        for v in x.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        xs.append(x)
        mq.append(a)
        my.append(b)
    return xs, mq, my


def y_mode_float32(x, hyp):
    """The kernel's y-mode operation order in numpy float32 under hypothesis hyp: the sums of |y_c| per thread (stride 256) and then over the
    threads, one scale per component, z = -(d d) (log2 e / var), the log-sum-exp of every bit-wise set around its own maximum, per-symbol
    terms, mean.  -> (AIR, GMI) as float, None when nothing is kept."""
    f = np.float32
    n, S = x["n"], x["n"] - 1
    b = int(round(np.log2(n)))
    y, amp = x["y"], x["amp"].astype(f)
    N = y.shape[-1]
    ri, ti = window(N, x["shift"])
    K = len(ri)
    if K == 0:
        return None
    sa = [np.array([np.abs(y[c, t::256]).sum(dtype=f) for t in range(min(256, N))], f).sum(dtype=f) for c in range(2)]
    if sa[0] == 0 or sa[1] == 0:
        return None
    sc = [f(x["amp_mean"]) / f(s / f(N)) for s in sa]
    ivl = f(f(1.4426950408889634) / f(x["var"]))
    z = np.empty((2, n, K), f)
    for c in range(2):
        yv = (y[c, ri] * sc[c]).astype(f)
        for i in range(n):
            dd = (yv - amp[i]).astype(f)
            z[c, i] = (-(dd * dd).astype(f) * ivl).astype(f)
    lev = tx_levels(x["tx"], n)[:, ti]
    (zI, zQ), _ = _apply(z, np.zeros((2, K), np.int64), hyp, S)
    g, H = gray(np.arange(n)), f(entropy(x["P"]))
    a, gg = np.zeros(K, f), np.zeros(K, f)
    for zz, t in ((zI, lev[0]), (zQ, lev[1])):
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
    return float(f(f(2) * H + f(a.sum(dtype=f) / f(K)))), float(f(f(2) * H + f(gg.sum(dtype=f) / f(K))))


def y_mode_float32_deviation(x, my):
    """What the float32 format costs y-mode -> largest |AIR or GMI deviation| of the run from its float64 model my in bit, None when nothing is kept."""
    r = y_mode_float32(x, my["hyp"])
    return None if r is None else max(abs(r[0] - my["AIR"]), abs(r[1] - my["GMI"]))

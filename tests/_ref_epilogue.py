"""Float64 numpy model of the per-frame epilogue (vaeq_dp_epilogue, vaeq_dp_epilogue_compact, vaeq_cma_epilogue), written from the
semantics of optical_DP_channel/shared_funcs.py (find_shift :290-314, find_shift_symb_full :316-338, SER_IQflip :188-222,
SER_constell_shaping :225-287, soft_dec :529-542) and of the roll / cut / slice lines of func_VAELE_DP_MQAM_shaping.py:68-89,
func_VAEflex_DP_MQAM_shaping.py:72-84 and func_CMA_DP_MQAM_shaping.py:39-52: np.roll for every roll, Python slices for every cut.

Test infrastructure only: nothing in the package imports it, and it imports neither the package nor the oracle.

What it returns beyond the kernels' outputs is what makes an EXACT comparison with a float32 kernel fair:
- the error counts of all 8 hypotheses (rotation k = 0, pi, pi/2, 3pi/2 times IQ flip f; row 2 k + f) x 2 polarisations and the kept count
  as integers; SER = float32(min count) / float32(kept), NaN when nothing is kept (the reference takes the mean of an empty slice);
- margins: the relative gap between the best and the second-best lag of each winning correlation (`lag_*`), the relative gap between the
  straight and the swapped pairing sums (`pair_*`), the smallest distance of a kept, normalised constellation sample from a decision
  threshold (`thr`), the smallest gap between the two largest q of a symbol (`qgap`; in the CMA form: of the model's own soft demapper,
  over the symbols that the soft-demapper path keeps -- the others are demapped but never compared).
A float32 evaluation in any summation order decides as the model does when these margins exceed its rounding error; the floors below
are asserted for every case of the GPU suite by test_ref_epilogue_host.py.

Layouts: q[2][2 n][N] (rows 0..n-1 of a polarisation = I levels, n..2n-1 = Q levels), y[2][2][N], tx[2][2][N] = [pol][I/Q][symbol].
"""
import functools

import numpy as np

N_SHIFT, HALF, N_CUT, EDGE = 21, 10, 10, 11
LAG_FLOOR, THR_FLOOR, QGAP_FLOOR = 1e-3, 2e-2, 0.05          # floors of the margins (reasons: test_ref_epilogue_host.py)
INF = float("inf")


def amp_levels(n):
    """The n amplitude levels of one axis of n^2-QAM, scaled to unit mean symbol power under a uniform pmf (float32, as the kernels get them)."""
    lev = np.arange(-(n - 1), n, 2).astype(np.float64)
    return (lev / np.sqrt(2 * np.mean(lev ** 2))).astype(np.float32)


# ------------------------------------------------------------------ the reference's steps
def shift_search(E, tx):
    """E[2,N] (equaliser side, per output polarisation b), tx[2,2,N] -> (shift[2], r, lag margin, pairing margin)   (:299-314)."""
    E, tx = np.asarray(E, np.float64), np.asarray(tx, np.float64)
    corr = np.empty((2, 2, 2, N_SHIFT))                                       # [c = I/Q of TX][b][a = TX pol][lag]
    for i in range(N_SHIFT):
        corr[..., i] = np.abs(np.einsum("acn,bn->cba", tx, np.roll(E, i - HALF, axis=-1)))
    cmax, cind = corr.max(-1), corr.argmax(-1)
    imax, cm = cmax.argmax(0), cmax.max(0)                                    # over I/Q: [b][a]
    pick = np.take_along_axis(cind, imax[None], 0)[0]
    s_xy, s_yx = cm[0, 0] + cm[1, 1], cm[0, 1] + cm[1, 0]
    straight = s_xy >= s_yx
    pairs = ((0, 0), (1, 1)) if straight else ((0, 1), (1, 0))
    shift = np.array([HALF - pick[b, a] for b, a in pairs], np.int64)
    lag = INF
    for b, a in pairs:                                                        # best value against the best one at any OTHER lag
        best, other = corr[:, b, a, :].max(), np.delete(corr[:, b, a, :], pick[b, a], axis=1).max()
        lag = min(lag, (best - other) / best)
    return shift, int(not straight), float(lag), float(abs(s_xy - s_yx) / max(s_xy, s_yx))


def align(t, shift, r):
    """t[2,C,N]: roll the polarisation axis by r, then polarisation p's symbol axis by -shift[p]."""
    t = np.roll(t, r, axis=0)
    return np.stack([np.roll(t[0], -int(shift[0]), axis=-1), np.roll(t[1], -int(shift[1]), axis=-1)])


def window(a, shift, batch_len):
    """The symbols of a[..., N] that the SER sees: [: batch_len - shift[0] - 10] of every minibatch (batch_len given), then
    [11 : -11 - max|shift|] of what is left -- both as Python slices, so a negative end counts from the end."""
    if batch_len is not None:
        N = a.shape[-1]
        a = a.reshape(a.shape[:-1] + (N // batch_len, batch_len))[..., :batch_len - int(shift[0]) - N_CUT]
        a = a.reshape(a.shape[:-2] + (a.shape[-2] * a.shape[-1],))
    return a[..., EDGE:-EDGE - int(np.max(np.abs(shift)))]


def kept_indices(N, shift, batch_len):
    """Indices (in the aligned frame) of the kept symbols."""
    return window(np.arange(N), shift, batch_len)


def tx_levels(tx, n):
    """TX level indices rint(scale t + scale) per axis (:198 / :239), int64[2,2,K]."""
    scale = (n - 1) / 2
    return np.round(scale * np.asarray(tx, np.float64) + scale).astype(np.int64)


def _hyp_counts(err_of):
    """err_of(k, f) -> bool[2,K]; -> int64[8,2]."""
    return np.array([[err_of(k, f)[p].sum() for p in range(2)] for k in range(4) for f in range(2)], np.int64).reshape(8, 2)


def soft_counts(dec, lev, n):
    """SER_IQflip on hard decisions dec[2,2,K] against TX levels lev[2,2,K]: error counts [8][2]."""
    S = n - 1
    a0, a1 = dec[:, 0].astype(np.int64), dec[:, 1].astype(np.int64)
    rot = [(a0, a1), (S - a0, S - a1), (S - a1, a0), (a1, S - a0)]            # decisions under rotation by 0, pi, pi/2, 3pi/2
    return _hyp_counts(lambda k, f: (lev[:, 0] != rot[k][0]) | ((S - lev[:, 1] if f else lev[:, 1]) != rot[k][1]))


def const_counts(y, tx, amp, nu_sc, var0):
    """SER_constell_shaping on the kept window y[2,2,K], tx[2,2,K]: (error counts [8][2], threshold margin, normalised y)."""
    n, S = len(amp), len(amp) - 1
    a = np.asarray(amp, np.float64)
    d_vec = (1 + 2 * float(nu_sc) * float(var0)) * (a[:-1] + a[1:]) / 2
    lo, hi = np.concatenate(([-INF], d_vec)), np.concatenate((d_vec, [INF]))
    lev = tx_levels(tx, n)
    tx, y = np.asarray(tx, np.float64), np.asarray(y, np.float64)
    if y.shape[-1] == 0:
        return np.zeros((8, 2), np.int64), INF, y
    y = y * (np.mean(np.sqrt(tx[:, 0] ** 2 + tx[:, 1] ** 2)) / np.mean(np.sqrt(y[:, 0] ** 2 + y[:, 1] ** 2)))
    rot = [(y[:, 0], y[:, 1]), (-y[:, 0], -y[:, 1]), (-y[:, 1], y[:, 0]), (y[:, 1], -y[:, 0])]
    ok = lambda v, d: (lo[d] <= v) & (v < hi[d])
    cnt = _hyp_counts(lambda k, f: ~(ok(rot[k][0], lev[:, 0]) & ok(rot[k][1], S - lev[:, 1] if f else lev[:, 1])))
    thr = min(float(np.min(np.abs(np.abs(y) - abs(t)))) for t in d_vec) if S else INF     # |v| against |t| covers v and -v
    return cnt, thr, y


def soft_dec(y, var, amp, nu_sc):
    """soft_dec (:529-542): q[2][2n][N] = softmax_i(-(y - a_i)^2 / (2 var_p) - nu_sc a_i^2) per axis."""
    a = np.asarray(amp, np.float64)
    y = np.asarray(y, np.float64)
    z = -(y[:, :, None, :] - a[None, None, :, None]) ** 2 / (2 * np.asarray(var, np.float64)[:, None, None, None]) \
        - float(nu_sc) * (a ** 2)[None, None, :, None]
    z = np.exp(z - z.max(2, keepdims=True))
    z /= z.sum(2, keepdims=True)
    return z.reshape(2, 2 * len(a), y.shape[-1])


def q_to_compact(q, amp):
    """What the training kernel hands the compact entry point: eq[2,N] = E_q[x_I] (:296-297), dec[2,2,N] = argmax q per axis (:201)."""
    n = len(amp)
    q = np.asarray(q, np.float64)
    eq = np.einsum("i,pin->pn", np.asarray(amp, np.float64), q[:, :n])
    dec = np.stack([q[:, :n].argmax(1), q[:, n:].argmax(1)], axis=1)
    return eq, dec


def q_gap(q, n):
    """Smallest gap between the two largest q of any symbol and axis."""
    s = np.sort(np.asarray(q, np.float64).reshape(2, 2, n, -1), axis=2)
    return float((s[:, :, -1] - s[:, :, -2]).min()) if s.shape[-1] else INF


def _ser(cnt, kept):
    if kept == 0:
        return np.full(2, np.nan, np.float32)
    return (cnt.min(0).astype(np.float32) / np.float32(kept)).astype(np.float32)


# ------------------------------------------------------------------ the three entry points
def dp_compact(eq, dec, y, tx, amp, nu_sc, var, batch_len=None, qgap=INF):
    """vaeq_dp_epilogue_compact: eq[2,N], dec[2,2,N], y[2,2,N], tx[2,2,N]."""
    n, N = len(amp), y.shape[-1]
    tx64 = np.asarray(tx, np.float64)
    lev = tx_levels(tx64, n)
    shift_q, r_q, lag_q, pair_q = shift_search(eq, tx64)
    cnt_q = soft_counts(window(align(np.asarray(dec), shift_q, r_q), shift_q, batch_len), window(lev, shift_q, batch_len), n)
    kept_q = len(kept_indices(N, shift_q, batch_len))
    shift_c, r_c, lag_c, pair_c = shift_search(np.asarray(y, np.float64)[:, 0], tx64)
    cnt_c, thr, _ = const_counts(window(align(np.asarray(y, np.float64), shift_c, r_c), shift_c, batch_len), window(tx64, shift_c, batch_len),
                                 amp, nu_sc, np.asarray(var).reshape(-1)[0])
    kept_c = len(kept_indices(N, shift_c, batch_len))
    return dict(shift_q=shift_q, r_q=r_q, shift_c=shift_c, r_c=r_c, cnt_q=cnt_q, cnt_c=cnt_c, kept_q=kept_q, kept_c=kept_c,
                SER=np.concatenate([_ser(cnt_c, kept_c), _ser(cnt_q, kept_q)]),
                margins=dict(lag_q=lag_q, pair_q=pair_q, lag_c=lag_c, pair_c=pair_c, thr=thr, qgap=qgap))


def dp_full(q, y, tx, amp, nu_sc, var, batch_len=None):
    """vaeq_dp_epilogue: q[2,2n,N] materialised."""
    eq, dec = q_to_compact(q, amp)
    return dp_compact(eq, dec, y, tx, amp, nu_sc, var, batch_len, qgap=q_gap(q, len(amp)))


def cma(y, tx, amp, nu_sc, var):
    """vaeq_cma_epilogue: y[2,2,N] = phase-corrected output cut to [10:-10], tx cut likewise.  The constellation stage runs first; its mean-radius
    normalisation stays in the kept window of the aligned y (the reference normalises a slice view in place), the soft demapper sees that, and
    the soft-demapper stage's shifts are relative to the aligned sequence.  Also returns that aligned y (`y_after`)."""
    n, N = len(amp), y.shape[-1]
    tx64, y = np.asarray(tx, np.float64), np.asarray(y, np.float64)
    lev = tx_levels(tx64, n)
    shift_c, r_c, lag_c, pair_c = shift_search(y[:, 0], tx64)
    ya = align(y, shift_c, r_c)
    cnt_c, thr, yn = const_counts(window(ya, shift_c, None), window(tx64, shift_c, None), amp, nu_sc, np.asarray(var).reshape(-1)[0])
    kc = kept_indices(N, shift_c, None)
    ya[:, :, kc] = yn
    q = soft_dec(ya, var, amp, nu_sc)
    eq, dec = q_to_compact(q, amp)
    shift_q, r_q, lag_q, pair_q = shift_search(eq, tx64)
    cnt_q = soft_counts(window(align(dec, shift_q, r_q), shift_q, None), window(lev, shift_q, None), n)
    kq = kept_indices(N, shift_q, None)
    return dict(shift_q=shift_q, r_q=r_q, shift_c=shift_c, r_c=r_c, cnt_q=cnt_q, cnt_c=cnt_c, kept_q=len(kq), kept_c=len(kc), y_after=ya,
                SER=np.concatenate([_ser(cnt_c, len(kc)), _ser(cnt_q, len(kq))]),
                margins=dict(lag_q=lag_q, pair_q=pair_q, lag_c=lag_c, pair_c=pair_c, thr=thr,
                             qgap=q_gap(window(align(q, shift_q, r_q), shift_q, None), n)))


def margins_ok(m):
    return min(m["lag_q"], m["pair_q"], m["lag_c"], m["pair_c"]) >= LAG_FLOOR and m["thr"] >= THR_FLOOR and m["qgap"] >= QGAP_FLOOR


# ------------------------------------------------------------------ inputs with margins by design
def _pmf(amp, nu):
    p = np.exp(-nu * np.asarray(amp, np.float64) ** 2)
    return p / p.sum()


def _unrotate(LI, LQ, hyp, S):
    """Received levels (a0, a1) for which hypothesis hyp = 2 k + f (rotation k, IQ flip f) decodes (LI, LQ) without error."""
    k, f = hyp >> 1, hyp & 1
    Qf = S - LQ if f else LQ
    return [(LI, Qf), (S - LI, S - Qf), (Qf, S - LI), (S - Qf, LI)][k]


def _channel(seq, r, delays):
    """seq[2,C,N] in TX order -> polarisations rolled by r, row b delayed by delays[b] (what align undoes when the rows' delays allow it)."""
    s = np.roll(seq, r, axis=0)
    return np.stack([np.roll(s[0], int(delays[0]), axis=-1), np.roll(s[1], int(delays[1]), axis=-1)])


def _one_dp(seed, N, n, shift, r, hyp, batch_len, shift_q, gain, nu_sc, var, nu_pcs, n_err):
    rng = np.random.default_rng(seed)
    amp = amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2                                  # u: half the level spacing
    lev = rng.choice(n, size=(2, 2, N), p=_pmf(amp, nu_pcs))
    tx = amp[lev].astype(np.float16)
    # symbol errors: whole-level jumps of one axis at positions that (where possible) both paths keep, n_err[p] of them in polarisation p
    kc, kq = kept_indices(N, shift, batch_len), kept_indices(N, shift_q, batch_len)
    pool = np.intersect1d(kc, kq) if len(kc) and len(kq) else (kc if len(kc) else kq)
    rxl = lev.copy()
    for p in range(2):
        for pos in rng.choice(pool, size=min(n_err[p], len(pool)), replace=False) if len(pool) else []:
            c = int(rng.integers(2))
            rxl[p, c, pos] += 1 if rxl[p, c, pos] < S else -1
    a0, a1 = _unrotate(rxl[:, 0], rxl[:, 1], hyp, S)
    rcv = np.stack([a0, a1], axis=1)                                          # [2,2,N] received levels
    clean = amp[rcv].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rcv.shape)
    y = _channel(gain * clean, r, shift).astype(np.float32)
    # q with a clear winner at the received level: top probability 0.55 .. 0.9, the rest spread over the other levels
    top = rng.uniform(0.55, 0.9, rcv.shape)
    rest = rng.uniform(0.2, 1.0, rcv.shape[:2] + (n,) + rcv.shape[2:])
    np.put_along_axis(rest, rcv[:, :, None, :], 0.0, axis=2)
    rest *= ((1 - top) / rest.sum(2))[:, :, None, :]
    np.put_along_axis(rest, rcv[:, :, None, :], top[:, :, None, :], axis=2)
    q = _channel(rest.reshape(2, 2 * n, N), r, shift_q).astype(np.float32)
    return dict(q=q, y=y, tx=tx, amp=amp, nu_sc=np.float32(nu_sc), var=np.asarray(var, np.float32), batch_len=batch_len)


def _one_cma(seed, N, n, shift, r, hyp, shift2, nu_sc, var, nu_pcs, n_err, n_big=10):
    """A frame whose I rows lock at `shift` in a linear correlation and whose DEMAPPED sequence locks `shift2` symbols further: n_big samples
    per polarisation in the frame's edges -- outside the constellation stage's kept window, so outside its mean-radius normalisation -- carry
    an amplitude of N with the TX signs at lag `shift`.  They own the linear correlation; the soft demapper saturates them to the outer
    level, and the bulk, which follows TX at lag shift + shift2, owns the second stage.  The bulk's gain is solved so that the normalisation
    of the kept window puts it on the level grid exactly."""
    rng = np.random.default_rng(seed)
    amp = amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2
    lev = rng.choice(n, size=(2, 2, N), p=_pmf(amp, nu_pcs))
    tx = amp[lev].astype(np.float16)
    kq = kept_indices(N, shift2, None)
    rxl = lev.copy()
    for p in range(2):
        for pos in rng.choice(kq, size=min(n_err[p], len(kq)), replace=False):
            c = int(rng.integers(2))
            rxl[p, c, pos] += 1 if rxl[p, c, pos] < S else -1
    bulk = amp[rxl].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rxl.shape)
    bulk = np.stack([np.roll(bulk[0], int(shift2[0]), axis=-1), np.roll(bulk[1], int(shift2[1]), axis=-1)])   # in the first stage's aligned frame
    kc = kept_indices(N, shift, None)
    edge = np.setdiff1d(np.arange(N), kc)
    big = np.zeros((2, N), bool)
    for p in range(2):
        big[p, rng.choice(edge, size=n_big, replace=False)] = True
    sign = np.where(amp[lev].astype(np.float64) >= 0, 1.0, -1.0)
    t64 = tx.astype(np.float64)
    g = np.sqrt(t64[:, 0] ** 2 + t64[:, 1] ** 2)[:, kc].sum() / np.sqrt(bulk[:, 0] ** 2 + bulk[:, 1] ** 2)[:, kc].sum()
    seq = np.where(big[:, None, :], float(N) * sign, g * bulk)
    a0, a1 = _unrotate(seq[:, 0], seq[:, 1], hyp, 0.0)                        # (amplitudes: level S - l is amplitude -a)
    y = _channel(np.stack([a0, a1], axis=1), r, shift).astype(np.float32)
    return dict(y=y, tx=tx, amp=amp, nu_sc=np.float32(nu_sc), var=np.asarray(var, np.float32))


def build_run(kind, seed, **kw):
    """One run's inputs and the model's result for them; the seed is advanced (at most 200 times) until the margins meet the floors, so a
    case never depends on a lucky draw and never on a lowered floor.  -> (inputs, model result)."""
    for s in range(seed, seed + 200):
        if kind == "cma":
            x = _one_cma(s, **kw)
            m = cma(x["y"], x["tx"], x["amp"], x["nu_sc"], x["var"])
            want = (kw["shift"], kw["r"], kw["shift2"], 0)
        else:
            x = _one_dp(s, **kw)
            m = dp_full(x["q"], x["y"], x["tx"], x["amp"], x["nu_sc"], x["var"], x["batch_len"])
            want = (kw["shift"], kw["r"], kw["shift_q"], kw["r"])
        hit = (tuple(m["shift_c"]), m["r_c"], tuple(m["shift_q"]), m["r_q"]) == (tuple(want[0]), want[1], tuple(want[2]), want[3])
        if hit and margins_ok(m["margins"]):
            return x, m
    raise AssertionError(f"no seed in {seed} .. {seed + 199} meets the margin floors for {kind} {kw}")


def dp_run(seed, N, n, shift, r=0, hyp=0, batch_len=None, shift_q=None, gain=1.0, nu_sc=0.0, var=(0.004, 0.004), nu_pcs=0.0, n_err=(2, 3)):
    return dict(kind="dp", seed=seed, N=N, n=n, shift=tuple(shift), r=r, hyp=hyp, batch_len=batch_len,
                shift_q=tuple(shift if shift_q is None else shift_q), gain=gain, nu_sc=nu_sc, var=tuple(var), nu_pcs=nu_pcs, n_err=tuple(n_err))


def cma_run(seed, N, n, shift, shift2, r=0, hyp=0, nu_sc=0.0, var=(0.002, 0.002), nu_pcs=0.0, n_err=(2, 3)):
    return dict(kind="cma", seed=seed, N=N, n=n, shift=tuple(shift), r=r, hyp=hyp, shift2=tuple(shift2), nu_sc=nu_sc, var=tuple(var),
                nu_pcs=nu_pcs, n_err=tuple(n_err))


# ------------------------------------------------------------------ the launches of the GPU suite (one entry = one kernel launch of R runs)
EPI2_SHARED_BYTES = 28768       # sizeof(vaeq::Epi2Shared), pinned by a static_assert in vaeq_epilogue_lds.h
TXC_LDS_BUDGET = 53 * 1024


def nib_words(N):
    return (N + 16 + 24 + 7) // 8


def txc_resident(N):
    """The launch's own switch in vaeq_dp_epilogue_compact: the TX level cache (4 rows of nib_words(N) 32-bit words) lives in LDS when
    4 * nib_words(N) * 4 + sizeof(Epi2Shared) <= 53 KiB."""
    return 4 * nib_words(N) * 4 + EPI2_SHARED_BYTES <= TXC_LDS_BUDGET


def residency_lengths():
    """The last resident N and its neighbours: (multiple of 4, odd) on the resident side, (odd, multiple of 4) on the other."""
    n_max = max(N for N in range(43, 70000) if txc_resident(N))               # 12712
    lo4 = n_max - n_max % 4
    hi4 = lo4 + 4
    return [lo4, n_max if n_max % 2 else n_max - 1, n_max + 1 if n_max % 2 == 0 else n_max + 2, hi4]


STRAIGHT_EXTREMES = [((10, -10), 0), ((-10, 10), 0), ((10, 10), 1), ((-10, -10), 1)]
NU_PCS = (0.0, 0.8, 2.0)


def _other(s0, i):
    """A shift[1] different from shift[0], inside -10 .. 10."""
    s1 = ((s0 + 10 + 3 + 2 * (i % 5)) % 21) - 10
    return s1 if s1 != s0 else (s1 + 1 if s1 < 10 else s1 - 1)


@functools.lru_cache(maxsize=None)
def launches():
    """name -> list of run specs that share N, n and batch_len."""
    L = {}
    # every shift[0] in -10 .. 10, both r, every hypothesis, every n_lev (7 shifts per launch)
    for j, n in enumerate((2, 4, 8)):
        runs = []
        for i, s0 in enumerate(range(-10 + j, 11, 3)):
            r = (i + j) % 2
            runs.append(dp_run(1000 + 10 * s0, 300, n, (s0, s0 if r else _other(s0, i)), r=r, hyp=(i + 3 * j) % 8, nu_pcs=NU_PCS[(i + j) % 3],
                               gain=0.7 + 0.1 * i, nu_sc=0.3 * (i % 3), n_err=(1 + i % 3, 4 + i % 2)))
        L[f"shift-n{n}"] = runs
    L["shift-extremes"] = [dp_run(1100 + i, 300, 8, s, r=0, hyp=2 * i + 1) for i, s in enumerate([(10, -10), (-10, 10), (10, 10), (-10, -10)])]
    # frame lengths without a minibatch cut: the minimum and every N % 4 residue, the correlation tile's edges, tile + one chunk
    for j, N in enumerate((43, 44, 45, 46, 47, 703, 704, 705, 726, 1407, 1408, 1409)):
        L[f"N{N}"] = [dp_run(2000 + 16 * j + i, N, (2, 4, 8)[j % 3], s, r=r, hyp=(i + 4 * j) % 8, nu_pcs=NU_PCS[i % 3], gain=0.5 + 0.3 * i)
                      for i, (s, r) in enumerate(STRAIGHT_EXTREMES)]
    for j, N in enumerate(residency_lengths()):
        L[f"residency-N{N}"] = [dp_run(2400 + 4 * j + i, N, 8, s, r=r, hyp=(2 * j + i) % 8) for i, (s, r) in enumerate([((10, -10), 0), ((-10, -10), 1)])]
    # minibatch cuts: shift[0] at -10 (whole minibatch kept), 0 and +10
    for j, (B, N) in enumerate([(20, 400), (25, 250), (50, 150), (64, 192), (100, 300), (128, 256), (255, 510), (256, 512), (257, 771), (300, 600),
                                (1000, 2000), (100, 100), (257, 257), (1000, 1000)]):
        L[f"B{B}-N{N}"] = [dp_run(3000 + 16 * j + i, N, (8, 4, 2)[j % 3], (s0, s0 if r else _other(s0, i + j)), r=r, hyp=(i + 3 * j) % 8, batch_len=B,
                                  nu_pcs=NU_PCS[(i + j) % 3], gain=0.6 + 0.4 * i, n_err=(2 + i, 5 + j % 2))
                           for i, (s0, r) in enumerate([(-10, 0), (0, j % 2), (10, 0)])]
    # empty kept windows: NaN in all four rows; then in the soft-demapper rows only
    L["empty-N60-B20"] = [dp_run(4000, 60, 8, (10, 10), batch_len=20), dp_run(4001, 60, 8, (5, 5), batch_len=20, hyp=3)]
    L["empty-N400-B20"] = [dp_run(4010, 400, 4, (10, 3), batch_len=20, hyp=5), dp_run(4011, 400, 4, (0, 2), batch_len=20, shift_q=(10, 3), hyp=6)]
    # batch_len < 20: the slice end batch_len - shift[0] - 10 is negative and counts from the minibatch's end
    L["short-B14"] = [dp_run(4100, 140, 8, (8, 3), batch_len=14, hyp=1, n_err=(3, 6)), dp_run(4101, 140, 8, (8, 8), r=1, batch_len=14, hyp=4, n_err=(5, 2))]
    L["short-B10"] = [dp_run(4110, 100, 4, (5, -2), batch_len=10, hyp=2, n_err=(2, 4)), dp_run(4111, 100, 4, (5, 5), r=1, batch_len=10, hyp=7, n_err=(4, 1))]
    # 37 runs with their own shift, swap, rotation, gain, nu_sc, var and pmf in one launch
    rng = np.random.default_rng(77)
    runs = []
    for i in range(37):
        s0, r = int(rng.integers(-10, 11)), i % 2
        runs.append(dp_run(5000 + 8 * i, 1000, 8, (s0, s0 if r else _other(s0, i)), r=r, hyp=i % 8, batch_len=100, gain=float(rng.uniform(0.5, 1.5)),
                           nu_sc=float(rng.uniform(0, 1.2)), var=tuple(rng.uniform(0.002, 0.008, 2)), nu_pcs=float(rng.uniform(0, 2.0)),
                           n_err=(1 + i % 4, 6 + i % 3)))
    L["per-run-R37"] = runs
    # the CMA entry point: second-stage shifts relative to the aligned sequence
    for j, N in enumerate((43, 47, 704, 705, 2000)):
        n = (4, 8, 2, 8, 4)[j]
        L[f"cma-N{N}"] = [cma_run(6000 + 16 * j + i, N, n, s, s2, r=r, hyp=(i + 3 * j) % 8, nu_pcs=NU_PCS[(i + j) % 3], nu_sc=0.4 * i)
                          for i, (s, s2, r) in enumerate([((3, -4), (2, -1), 0), ((-10, -10), (-3, 5), 1), ((10, -7), (1, 1), 0)])]
    return L


DP_LAUNCHES = [k for k in launches() if not k.startswith("cma-")]
CMA_LAUNCHES = [k for k in launches() if k.startswith("cma-")]


@functools.lru_cache(maxsize=None)
def build_launch(name):
    """-> (list of per-run inputs, list of per-run model results); built once, shared by the tests, never modified."""
    xs, ms = [], []
    for spec in launches()[name]:
        kw = {k: v for k, v in spec.items() if k not in ("kind", "seed")}
        x, m = build_run(spec["kind"], spec["seed"], **kw)
        for v in x.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        xs.append(x)
        ms.append(m)
    return xs, ms

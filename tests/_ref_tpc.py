"""Two models of vaeq_tpc_decode (include/vaeq.h): Chase-Pyndiah decoding of a product code whose rows and columns are words of two
single-error-correcting codes given by the columns of their parity-check matrices.  The rule is stated on r, the LLR towards the transmitted bit,
so there is no encoder; integers, and float32 operations in the order the header fixes, so that the kernel has to reproduce every bit.

word()    (1) one component word of the specification, with a syndrome -> position table and a counter on every branch: status0 / status1 /
          status2, competitor / no-competitor (a position with and without one), delta-zero (a competitor whose metric equals the winner's),
          clamp-W (an extrinsic value that the clip changed);
block()   (1) one product block: the schedule, the stop test and out[8]; counters clamp-r (an input that the clip changed), clamp-beta (a
          beta_h scale above the clip), stop-h0, stop-odd, stop-even (a stop at an even h > 0), no-stop;
decode()  (1) over device-layout tensors: out[R, C, 8], the stream (llr[R, C n] float32, bits[R, C n] int8), ext[R, C, n] float32,
          half_err[R, C, 2 iters] and the Counter;
word2() / block2()  (2) an independent restatement for components of n' <= 16 bits without any syndrome table: the code is the list of its
          codewords (every word of n' bits with H c = 0), a test pattern's candidate is the listed codeword within distance 1 of the flipped
          word, its metric the sum over the positions where it differs from the hard decisions, and the competitor of a position is found by
          brute force over all candidates that differ from the winner there.  The stop test multiplies with the dense H.
          tests/test_ref_tpc_host.py holds the two to each other.
"""
import collections
import functools

import numpy as np

import _ref_chase as X
import _ref_ldpc as M

F = np.float32
ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)               # Pyndiah's schedules, per half-iteration, continued with 1
BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
CLIP = F(2.0 ** 60)


def schedule(values, iters, last=1.0):
    """The first 2 iters entries of a schedule continued with `last`, float32."""
    v = list(values)[:2 * iters]
    return np.array(v + [last] * (2 * iters - len(v)), F)


def word(cols, p, Rv, beta, clip, count):
    """(1) for one word: Rv[n'] float32, the soft input -> (status, d[n'] bool, W'[n'] float32, the positions without a competitor)."""
    cols = [int(c) for c in cols]
    n = len(cols)
    a, e = np.abs(Rv), Rv < 0
    where = {c: j for j, c in enumerate(cols)}
    s0 = 0
    for j in np.nonzero(e)[0]:
        s0 ^= cols[j]
    least = [int(j) for j in np.lexsort((np.arange(n), a))[:p]]    # by (a_j, j) ascending
    cands = []                                                 # (metric bits, T, metric, flips)
    for T in range(1 << p):
        FT = [least[i] for i in range(p) if (T >> i) & 1]
        s = s0
        for j in FT:
            s ^= cols[j]
        v = None
        if s:
            v = where.get(s)
            if v is None:
                continue
        metric, flips = F(0.0), []
        for j in FT:
            if j == v:
                continue
            metric = F(metric + a[j])
            flips.append(j)
        if v is not None and v not in FT:
            metric = F(metric + a[v])
            flips.append(v)
        cands.append((int(metric.view(np.uint32)), T, metric, frozenset(flips)))
    if not cands:
        count["status2"] += 1
        return 2, e.copy(), np.zeros(n, F), 0
    _, _, mD, D = min(cands, key=lambda c: (c[0], c[1]))
    count[f"status{int(bool(D))}"] += 1
    assert bool(D) == (s0 != 0)
    d = e.copy()
    d[list(D)] ^= True
    mC = np.full(n, np.inf, F)                                 # every metric is finite: inf = no competitor
    for _, _, m, flips in cands:
        for j in flips ^ D:
            mC[j] = min(mC[j], m)
    has = np.isfinite(mC)
    delta = np.where(has, mC, mD) - mD                         # float32 - float32
    assert delta.dtype == F and (delta >= 0).all()
    L = np.where(d, -delta, delta)
    Wn = np.where(has, L - Rv, np.where(d, -beta, beta)).astype(F)
    Wc = np.minimum(np.maximum(Wn, -clip), clip)
    count["competitor"] += int(has.sum())
    count["no-competitor"] += int((~has).sum())
    count["delta-zero"] += int((has & (delta == 0)).sum())
    count["clamp-W"] += int((Wc != Wn).sum())
    return int(bool(D)), d, Wc, int((~has).sum())


def _prepare(x, b, clip):
    x = np.array(x, F)
    x[np.isnan(x)] = F(0.0)                                    # a NaN is +0
    b = np.asarray(b).astype(bool)
    r = np.where(b, -x, x).astype(F)
    rc = np.minimum(np.maximum(r, -clip), clip)
    return x, b, r, rc


def _beta(beta_h, scale, clip, count):
    prod = F(F(beta_h) * F(scale))
    if not prod > 0:                                           # a NaN, a zero of either sign or a negative product: +0
        return F(0.0)
    if prod > clip:
        count["clamp-beta"] += 1
    return min(prod, clip)


def _finish(h, stopped, d, b, K1, K2, pre, erased, nstat2, nbeta, half, count):
    count["no-stop" if not stopped else "stop-h0" if h == 0 else "stop-odd" if h & 1 else "stop-even"] += 1
    return np.array([h + 1, int(stopped), int(d.sum()), pre, erased, int(d[:K1, :K2].sum()), nstat2, nbeta], np.int64), half


def block(cols1, cols2, x, b, p, iters, alpha, beta, scale, clip, K1, K2, count=None):
    """(1) for one block: x[n1, n2] LLRs, b[n1, n2] TX bits; alpha[2 iters], beta[2 iters] float32 ->
    (out[8], d[n1, n2] bool, W[n1, n2] float32, half_err[2 iters])."""
    count = collections.Counter() if count is None else count
    clip = F(clip)
    x, b, r, rc = _prepare(x, b, clip)
    count["clamp-r"] += int((rc != r).sum())
    n1, n2 = x.shape
    pre, erased = int(((x < 0) ^ b).sum()), int((x == 0).sum())
    W = np.zeros((n1, n2), F)
    half = np.full(2 * iters, -1, np.int64)
    nstat2 = nbeta = 0
    for h in range(2 * iters):
        Rv = rc + F(alpha[h]) * W                              # one float32 multiplication, one float32 addition
        assert Rv.dtype == F
        bh = _beta(beta[h], scale, clip, count)
        d, Wn, worst = np.zeros((n1, n2), bool), np.zeros((n1, n2), F), 0
        for k in range(n2 if h & 1 else n1):
            at = (slice(None), k) if h & 1 else (k, slice(None))
            st, d[at], Wn[at], nb = word(cols1 if h & 1 else cols2, p, Rv[at], bh, clip, count)
            nstat2, nbeta, worst = nstat2 + (st == 2), nbeta + nb, max(worst, st)
        W = Wn
        half[h] = int(d.sum())
        syn = np.zeros(n1 if h & 1 else n2, np.int64)          # the other direction's syndromes on d
        for j, c in enumerate(cols2 if h & 1 else cols1):
            syn ^= np.where(d[:, j] if h & 1 else d[j, :], int(c), 0)
        if worst < 2 and not syn.any():
            return *_finish(h, True, d, b, K1, K2, pre, erased, nstat2, nbeta, half, count), d, W
    return *_finish(h, False, d, b, K1, K2, pre, erased, nstat2, nbeta, half, count), d, W


def decode(llr, bits, cols1, cols2, p, iters, alpha, beta, scale, clip, K1, K2, t0, C, count=None):
    """(1) over device-layout tensors llr[R, w, N] float32, bits[R, w, N] int8; scale[R] or None ->
    (out[R, C, 8] int64, stream llr[R, C n] float32, stream bits[R, C n] int8, ext[R, C, n] float32, half_err[R, C, 2 iters] int64, Counter)."""
    count = collections.Counter() if count is None else count
    n1, n2, R = len(cols1), len(cols2), llr.shape[0]
    n = n1 * n2
    x, tx = M.codewords(llr, t0, C, n), M.codewords(bits, t0, C, n).astype(bool)
    out, half = np.zeros((R, C, 8), np.int64), np.zeros((R, C, 2 * iters), np.int64)
    s_llr, s_bits, ext = np.zeros((R, C * n), F), np.zeros((R, C * n), np.int8), np.zeros((R, C, n), F)
    for r in range(R):
        for c in range(C):
            b = tx[r, c].reshape(n1, n2)
            out[r, c], half[r, c], d, W = block(cols1, cols2, x[r, c].reshape(n1, n2), b, p, iters, alpha, beta,
                                                F(1.0) if scale is None else scale[r], clip, K1, K2, count)
            s_bits[r, c * n:(c + 1) * n] = b.ravel()
            s_llr[r, c * n:(c + 1) * n] = np.where(b ^ d, F(-1.0), F(1.0)).ravel()
            ext[r, c] = W.ravel()
    return out, s_llr, s_bits, ext, half, count


def figures(out, n, K):
    """The per-run figures of engine.tpc_decode from out[R, C, 8], as it forms them: float64 quotients rounded to float32."""
    C = out.shape[1]
    return dict(BER_post=(out[..., 2].sum(1) / np.float64(C * n)).astype(F), BER_pre=(out[..., 3].sum(1) / np.float64(C * n)).astype(F),
                BER_payload=(out[..., 5].sum(1) / np.float64(C * K)).astype(F), FER=((out[..., 2] > 0).sum(1) / np.float64(C)).astype(F))


# ---- model 2 ----

@functools.lru_cache(maxsize=None)
def _codebook(cols, r):
    """Every codeword of the code with the parity-check columns `cols` (a tuple), n' <= 16: [count, n'] bool."""
    n = len(cols)
    assert n <= 16
    words = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    H = X.dense_H(cols, r)
    return words[~((words @ H.T) % 2).any(1)].astype(bool)


def word2(cols, r, p, Rv, beta, clip):
    """(2) for one word of n' <= 16 bits -> (status, d, W', the positions without a competitor)."""
    n = len(cols)
    book = _codebook(tuple(int(c) for c in cols), r)
    a, e = np.abs(Rv), Rv < 0
    taken, least = np.zeros(n, bool), []
    for _ in range(p):                                         # the smallest a not yet taken; a strict < keeps the smallest j among equals
        pick = None
        for j in range(n):
            if not taken[j] and (pick is None or a[j] < a[pick]):
                pick = j
        taken[pick] = True
        least.append(pick)
    cands = []                                                 # (metric, T, the codeword)
    for T in range(1 << p):
        members = [least[i] for i in range(p) if (T >> i) & 1]
        flipped = e.copy()
        flipped[members] ^= True
        near = book[(book ^ flipped).sum(1) <= 1]
        assert len(near) <= 1                                  # minimum distance 3: at most one
        if not len(near):
            continue
        diff = near[0] ^ e
        extra = [int(j) for j in np.nonzero(diff)[0] if j not in members]
        metric = F(0.0)
        for j in [j for j in members if diff[j]] + extra:      # the members in the order of the list, then the syndrome's position
            metric = F(metric + a[j])
        cands.append((float(metric), T, near[0]))
    if not cands:
        return 2, e.copy(), np.zeros(n, F), 0
    mD, _, d = min(cands, key=lambda c: (c[0], c[1]))
    Wn, none = np.zeros(n, F), 0
    for j in range(n):
        rivals = [m for m, _, c in cands if c[j] != d[j]]
        if rivals:
            delta = F(F(min(rivals)) - F(mD))
            Wn[j] = F((-delta if d[j] else delta) - Rv[j])
        else:
            Wn[j] = -beta if d[j] else beta
            none += 1
        Wn[j] = min(max(Wn[j], -clip), clip)
    return int((d != e).any()), d.copy(), Wn, none


def block2(cols1, r1, cols2, r2, x, b, p, iters, alpha, beta, scale, clip, K1, K2):
    """(2) for one block -> (out[8], half_err[2 iters], d, W)."""
    clip = F(clip)
    x = np.array(x, F)
    n1, n2 = x.shape
    b = np.asarray(b).astype(bool)
    r = np.zeros((n1, n2), F)
    pre = erased = 0
    for i in range(n1):
        for j in range(n2):
            v = F(0.0) if np.isnan(x[i, j]) else x[i, j]
            pre += int((v < 0) != b[i, j])
            erased += int(v == 0)
            v = -v if b[i, j] else v
            r[i, j] = clip if v > clip else -clip if v < -clip else v
    H1, H2 = X.dense_H(cols1, r1).astype(np.int64), X.dense_H(cols2, r2).astype(np.int64)
    W = np.zeros((n1, n2), F)
    half = np.full(2 * iters, -1, np.int64)
    nstat2 = nbeta = stopped = 0
    for h in range(2 * iters):
        prod = F(F(beta[h]) * F(scale))
        bh = min(prod, clip) if prod > 0 else F(0.0)
        Rv = (r + (F(alpha[h]) * W).astype(F)).astype(F)
        d, Wn, clean = np.zeros((n1, n2), bool), np.zeros((n1, n2), F), True
        if h & 1:
            for k in range(n2):
                st, d[:, k], Wn[:, k], nb = word2(cols1, r1, p, Rv[:, k], bh, clip)
                nstat2, nbeta, clean = nstat2 + (st == 2), nbeta + nb, clean and st < 2
            other = (H2 @ d.T.astype(np.int64)) % 2            # the rows under the row code
        else:
            for k in range(n1):
                st, d[k], Wn[k], nb = word2(cols2, r2, p, Rv[k], bh, clip)
                nstat2, nbeta, clean = nstat2 + (st == 2), nbeta + nb, clean and st < 2
            other = (H1 @ d.astype(np.int64)) % 2              # the columns under the column code
        W = Wn
        half[h] = int(d.sum())
        if clean and not other.any():
            stopped = 1
            break
    return np.array([h + 1, stopped, int(d.sum()), pre, erased, int(d[:K1, :K2].sum()), nstat2, nbeta], np.int64), half, d, W

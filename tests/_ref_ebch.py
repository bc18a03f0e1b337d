"""Two models of vaeq_chase_bch_decode and vaeq_tpc_bch_decode (include/vaeq.h): Chase and Chase-Pyndiah decoding over (extended)
double-error-correcting BCH words.  Integers, and float32 operations in the order the header fixes, so that the kernels have to reproduce every bit.

Code                 (m, n, extended) with n_i, k: the component as the entry points take it;
candidates()         (1) the test patterns of one word.  The locator is _ref_bch.decode(m, 2, n_i, ...): Berlekamp-Massey plus a root search over
                     all positions, which shares nothing with the kernel's closed form.  A counter on every branch: inner-status0 / one-position /
                     two-positions / no-cand-S1=0 / no-cand-no-root / no-cand-shortened (the inner word), u-flipped / u-kept (the parity bit),
                     v-cancels (a located position that is listed and a member of F_T), v-listed-new (listed, not in F_T), u-listed;
chase_word()         (1) vaeq_chase_bch_decode for one word -> out[6]; counters status0 / status1 / status2, miscorrected, undetected;
tpc_word(), block(), decode_tpc()   (1) vaeq_tpc_bch_decode with _ref_tpc's counters: competitor / no-competitor, delta-zero, clamp-W, clamp-r,
                     clamp-beta, stop-h0 / stop-odd / stop-even / no-stop;
decode_chase()       (1) over device-layout tensors, as _ref_chase.decode;
word2() / chase_word2() / block2()   (2) for n <= 16: the code is nothing but the list of its codewords.  A pattern's candidate is the inner
                     codeword within distance 2 of the inner part of the flipped word, completed by its parity bit; the competitors are found by
                     search over all candidates; the stop test looks the words up in the list.  tests/test_ref_ebch_host.py holds (1) to (2).
"""
import collections
import functools

import numpy as np

import _ref_bch as B
import _ref_chase as X
import _ref_ldpc as M
import _ref_tpc as P

F = np.float32


class Code:
    def __init__(self, m, n=None, extended=True):
        self.m, self.ext = m, int(bool(extended))
        self.n = (1 << m) - 1 + self.ext if n is None else n
        self.n_i = self.n - self.ext
        self.k = self.n_i - 2 * m
        assert 4 <= m <= 8 and 2 * m < self.n_i <= (1 << m) - 1

    def args(self):
        return self.m, self.n, self.ext


_MEMO = {}
_BRANCH = {"status0": "inner-status0", "L>t": "no-cand-S1=0", "roots<L": "no-cand-no-root", "shortened-root": "no-cand-shortened"}


def locate(code, positions, count):
    """vaeq_bch_outer's rule with t = 2, n_o = n_i for one inner error pattern -> (status, V).  Remembered per syndrome: the rule is a function
    of S_1 .. S_4 alone."""
    key = (code.m, code.n_i, tuple(B.syndromes(code.m, 2, positions)))
    if key not in _MEMO:
        own = collections.Counter()
        status, V = B.decode(code.m, 2, code.n_i, positions, own)
        _MEMO[key] = status, tuple(V), [_BRANCH[k] for k in own if k in _BRANCH and own[k]]
    status, V, branches = _MEMO[key]
    for b in branches:
        count[b] += 1
    if status == 1:
        count["one-position" if len(V) == 1 else "two-positions"] += 1
    return status, V


def least_reliable(a, p):
    return [int(j) for j in np.lexsort((np.arange(len(a)), a))[:p]]    # by (a_j, j) ascending


def candidates(code, p, a, e, count):
    """(1) -> (least, [(metric bits, T, metric, Phi_T as a frozenset)]) for one word: a[n] float32 >= 0, e[n] bool."""
    n_i, u = code.n_i, code.n_i
    least = least_reliable(a, p)
    cands = []
    for T in range(1 << p):
        FT = [least[i] for i in range(p) if (T >> i) & 1]
        x = e.copy()
        x[FT] ^= True
        status, V = locate(code, [int(j) for j in np.nonzero(x[:n_i])[0]], count)
        if status == 2:
            continue
        flips = set(FT) ^ set(V)
        for v in V:
            if v in least:
                count["v-cancels" if v in FT else "v-listed-new"] += 1
        if code.ext:
            fu = (int(x.sum()) + len(V)) & 1
            count["u-flipped" if fu else "u-kept"] += 1
            if fu:
                flips ^= {u}
            if u in least:
                count["u-listed"] += 1
        metric = F(0.0)
        for j in [j for j in least if j in flips] + sorted(j for j in flips if j not in least):
            metric = F(metric + a[j])
        cands.append((int(metric.view(np.uint32)), T, metric, frozenset(flips)))
    return least, cands


def chase_word(code, p, K, x, b, count=None):
    """(1) vaeq_chase_bch_decode for one word -> (out[6], the final e[n])."""
    count = collections.Counter() if count is None else count
    x, a, e = X._inputs(x, b)
    _, cands = candidates(code, p, a, e, count)
    pre, erased = int(e.sum()), int((x == 0).sum())
    if not cands:
        count["status2"] += 1
        return np.array([2, pre, pre, 0, erased, int(e[:K].sum())], np.int64), e
    best = min(cands, key=lambda c: (c[0], c[1]))
    e = e.copy()
    e[list(best[3])] ^= True
    status, post = int(bool(best[3])), int(e.sum())
    count[f"status{status}"] += 1
    count["miscorrected"] += status == 1 and post > 0
    count["undetected"] += status == 0 and pre > 0
    count["winner-T>0"] += best[1] > 0
    return np.array([status, pre, post, len(best[3]), erased, int(e[:K].sum())], np.int64), e


def decode_chase(llr, bits, code, p, K, t0, C, depth=0, spread=1, count=None):
    """(1) over device-layout tensors -> (out[R, C, 6] int64, stream llr[R, C K] float32, stream bits[R, C K] int8, the Counter)."""
    count = collections.Counter() if count is None else count
    n, R = code.n, llr.shape[0]
    x, tx = X.gather(llr, t0, C, n, depth), X.gather(bits, t0, C, n, depth).astype(bool)
    out = np.zeros((R, C, 6), np.int64)
    s_llr, s_bits = np.zeros((R, C * K), F), np.zeros((R, C * K), np.int8)
    u = X.stream_index(C, K, spread)
    for r in range(R):
        for c in range(C):
            out[r, c], e = chase_word(code, p, K, x[r, c], tx[r, c], count)
            s_bits[r, u[c]] = tx[r, c, :K]
            s_llr[r, u[c]] = np.where(tx[r, c, :K] ^ e[:K], F(-1.0), F(1.0))
    return out, s_llr, s_bits, count


def _soft_out(n, Rv, e, cands, beta, clip, count):
    """The tail of a Chase-Pyndiah word from its candidates on -> (status, d, W', the positions without a competitor)."""
    if not cands:
        count["status2"] += 1
        return 2, e.copy(), np.zeros(n, F), 0
    _, _, mD, D = min(cands, key=lambda c: (c[0], c[1]))
    count[f"status{int(bool(D))}"] += 1
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


def tpc_word(code, p, Rv, beta, clip, count):
    """(1) for one word of a product block: Rv[n] float32, the soft input -> (status, d[n] bool, W'[n] float32, positions without a competitor)."""
    a, e = np.abs(Rv), Rv < 0
    _, cands = candidates(code, p, a, e, count)
    return _soft_out(code.n, Rv, e, cands, beta, clip, count)


def is_codeword(code, d, count=None):
    """S_1 = S_3 = 0 on the inner part and, if extended, even weight."""
    S = B.syndromes(code.m, 2, [int(j) for j in np.nonzero(d[:code.n_i])[0]])
    return S[0] == 0 and S[2] == 0 and not (code.ext and int(d.sum()) & 1)


def block(code1, code2, x, b, p, iters, alpha, beta, scale, clip, K1, K2, count=None, word=None, clean=None):
    """(1) for one block: x[n1, n2] LLRs, b[n1, n2] TX bits; the columns are words of code1, the rows of code2 ->
    (out[8], half_err[2 iters], d[n1, n2] bool, W[n1, n2] float32).  word / clean: model (2)'s word and codeword test in their place."""
    count = collections.Counter() if count is None else count
    word = tpc_word if word is None else word
    clean = is_codeword if clean is None else clean
    clip = F(clip)
    x, b, r, rc = P._prepare(x, b, clip)
    count["clamp-r"] += int((rc != r).sum())
    n1, n2 = x.shape
    pre, erased = int(((x < 0) ^ b).sum()), int((x == 0).sum())
    W = np.zeros((n1, n2), F)
    half = np.full(2 * iters, -1, np.int64)
    nstat2 = nbeta = 0
    for h in range(2 * iters):
        Rv = rc + F(alpha[h]) * W                              # one float32 multiplication, one float32 addition
        assert Rv.dtype == F
        bh = P._beta(beta[h], scale, clip, count)
        d, Wn, worst = np.zeros((n1, n2), bool), np.zeros((n1, n2), F), 0
        for k in range(n2 if h & 1 else n1):
            at = (slice(None), k) if h & 1 else (k, slice(None))
            st, d[at], Wn[at], nb = word(code1 if h & 1 else code2, p, Rv[at], bh, clip, count)
            nstat2, nbeta, worst = nstat2 + (st == 2), nbeta + nb, max(worst, st)
        W = Wn
        half[h] = int(d.sum())
        other = all(clean(code2, d[k]) for k in range(n1)) if h & 1 else all(clean(code1, d[:, k]) for k in range(n2))
        if worst < 2 and other:
            return *P._finish(h, True, d, b, K1, K2, pre, erased, nstat2, nbeta, half, count), d, W
    return *P._finish(h, False, d, b, K1, K2, pre, erased, nstat2, nbeta, half, count), d, W


def decode_tpc(llr, bits, code1, code2, p, iters, alpha, beta, scale, clip, K1, K2, t0, C, count=None):
    """(1) over device-layout tensors llr[R, w, N] float32, bits[R, w, N] int8; scale[R] or None ->
    (out[R, C, 8] int64, stream llr[R, C n] float32, stream bits[R, C n] int8, ext[R, C, n] float32, half_err[R, C, 2 iters] int64, Counter)."""
    count = collections.Counter() if count is None else count
    n1, n2, R = code1.n, code2.n, llr.shape[0]
    n = n1 * n2
    x, tx = M.codewords(llr, t0, C, n), M.codewords(bits, t0, C, n).astype(bool)
    out, half = np.zeros((R, C, 8), np.int64), np.zeros((R, C, 2 * iters), np.int64)
    s_llr, s_bits, ext = np.zeros((R, C * n), F), np.zeros((R, C * n), np.int8), np.zeros((R, C, n), F)
    for r in range(R):
        for c in range(C):
            b = tx[r, c].reshape(n1, n2)
            out[r, c], half[r, c], d, W = block(code1, code2, x[r, c].reshape(n1, n2), b, p, iters, alpha, beta,
                                                F(1.0) if scale is None else scale[r], clip, K1, K2, count)
            s_bits[r, c * n:(c + 1) * n] = b.ravel()
            s_llr[r, c * n:(c + 1) * n] = np.where(b ^ d, F(-1.0), F(1.0)).ravel()
            ext[r, c] = W.ravel()
    return out, s_llr, s_bits, ext, half, count


# ---- model 2 ----

@functools.lru_cache(maxsize=None)
def codebook(m, n_i):
    """Every word of n_i <= 15 bits with S_1 = S_3 = 0, by a dense parity-check matrix over GF(2): [count, n_i] bool."""
    assert n_i <= 15
    exp, _ = B.tables(m)
    q = (1 << m) - 1
    H = np.array([[(int(exp[j * pos % q]) >> bit) & 1 for pos in range(n_i)] for j in (1, 3) for bit in range(m)], np.int64)
    words = (np.arange(1 << n_i)[:, None] >> np.arange(n_i)[None, :]) & 1
    return words[~((words @ H.T) % 2).any(1)].astype(bool)


def _extend(code, inner):
    return np.append(inner, inner.sum() & 1).astype(bool) if code.ext else inner.copy()


def _candidates2(code, p, a, e):
    """(2) -> [(metric, T, the candidate codeword of n bits)]"""
    n, n_i = code.n, code.n_i
    book = codebook(code.m, n_i)
    taken, least = np.zeros(n, bool), []
    for _ in range(p):                                         # the smallest a not yet taken; a strict < keeps the smallest j among equals
        pick = None
        for j in range(n):
            if not taken[j] and (pick is None or a[j] < a[pick]):
                pick = j
        taken[pick] = True
        least.append(pick)
    cands = []
    for T in range(1 << p):
        members = [least[i] for i in range(p) if (T >> i) & 1]
        flipped = e.copy()
        flipped[members] ^= True
        near = book[(book ^ flipped[:n_i]).sum(1) <= 2]
        assert len(near) <= 1                                  # minimum distance 5: at most one
        if not len(near):
            continue
        word = _extend(code, near[0])
        diff = word ^ e
        metric = F(0.0)
        for j in [j for j in least if diff[j]] + [int(j) for j in np.nonzero(diff)[0] if j not in least]:   # the list's order, then ascending
            metric = F(metric + a[j])
        cands.append((float(metric), T, word))
    return cands


def chase_word2(code, p, K, x, b):
    """(2) vaeq_chase_bch_decode for one word of n <= 16 bits -> (out[6], the final e)."""
    x, a, e = X._inputs(x, b)
    cands = _candidates2(code, p, a, e)
    pre, erased = int(e.sum()), int((x == 0).sum())
    if not cands:
        return np.array([2, pre, pre, 0, erased, int(e[:K].sum())], np.int64), e
    _, _, word = min(cands, key=lambda c: (c[0], c[1]))
    nflip = int((word ^ e).sum())
    return np.array([int(nflip > 0), pre, int(word.sum()), nflip, erased, int(word[:K].sum())], np.int64), word.copy()


def word2(code, p, Rv, beta, clip, count=None):
    """(2) for one word of a product block -> (status, d, W', the positions without a competitor)."""
    n = code.n
    a, e = np.abs(Rv), Rv < 0
    cands = _candidates2(code, p, a, e)
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


def in_book(code, d, count=None):
    """(2)'s codeword test: the word is in the list."""
    book = codebook(code.m, code.n_i)
    return bool((book == d[:code.n_i]).all(1).any()) and not (code.ext and int(d.sum()) & 1)


def block2(code1, code2, x, b, p, iters, alpha, beta, scale, clip, K1, K2):
    """(2) for one block: model (1)'s schedule around model (2)'s word and codeword test -> (out[8], half_err, d, W)."""
    return block(code1, code2, x, b, p, iters, alpha, beta, scale, clip, K1, K2, None, word2, in_book)

"""Two models of vaeq_chase_decode (include/vaeq.h): Chase decoding of a single-error-correcting code given by the columns of its parity-check
matrix, acting on the error pattern e = (llr < 0) xor the TX bits.  Integers, and float32 additions in the order the header fixes, so that the
kernel has to reproduce every bit.

word()        (a) the specification with a syndrome -> position table, and a counter on every branch: status0 / status1 / status2, no-candidate (a
              test pattern without a candidate), v-cancelled (the syndrome's position was a member of F_T and left the flips), winner-T>0,
              metric-tie (the winning metric is shared by a candidate with a larger T), reliability-tie (two equal |llr| whose order decides the
              list of least reliable positions, or the order inside it), miscorrected, undetected, inf-metric (a candidate of infinite metric);
word_search() (b) an independent restatement for n <= 20 without any syndrome table: the least reliable positions by repeated argmin; for every
              test pattern the words within distance 1 of the flipped word are multiplied with the dense H over GF(2), and the one that gives
              zero is the candidate.  tests/test_ref_chase_host.py holds the two to each other;
gather()      x[R, C, n], tx[R, C, n] of device-layout tensors under the bit map of the depth;
decode()      (a) over them: out[R, C, 6], the payload stream (llr[R, C K] float32, bits[R, C K] int8) and the Counter.
"""
import collections

import numpy as np

import _ref_ldpc as M
import _ref_ldpc_il as IL

F = np.float32


def hamming_cols(m, extended=True, n=None):
    """-> (cols[n] int64, r): the two column rules of engine.hamming_code."""
    n = ((1 << m) - (0 if extended else 1)) if n is None else n
    j = np.arange(n, dtype=np.int64)
    return ((j << 1) | 1, m + 1) if extended else (j + 1, m)


def _inputs(x, b):
    x = np.array(x, dtype=F)
    x[np.isnan(x)] = F(0.0)                                    # a NaN is +0
    y = x < 0                                                  # +-0 is bit 0
    return x, np.abs(x), y ^ np.asarray(b).astype(bool)


def word(cols, p, K, x, b, count=None):
    """(a) for one codeword: x[n] float32, b[n] TX bits -> (out[6] = status, pre_err, post_err, nflip, erased, pay_err; the final e[n] bool)."""
    count = collections.Counter() if count is None else count
    cols = [int(c) for c in cols]
    n = len(cols)
    x, a, e = _inputs(x, b)
    where = {c: j for j, c in enumerate(cols)}
    s0 = 0
    for j in np.nonzero(e)[0]:
        s0 ^= cols[j]
    order = np.lexsort((np.arange(n), a))                      # by (a_j, j) ascending
    least = [int(j) for j in order[:p]]
    if any(a[order[i]] == a[order[i + 1]] for i in range(min(p, n - 1))):
        count["reliability-tie"] += 1
    cands = []                                                 # (metric bits, T, flips)
    for T in range(1 << p):
        FT = [least[i] for i in range(p) if (T >> i) & 1]
        s = s0
        for j in FT:
            s ^= cols[j]
        v = None
        if s:
            v = where.get(s)
            if v is None:
                count["no-candidate"] += 1
                continue
        metric, flips = F(0.0), []
        for j in FT:
            if j == v:
                count["v-cancelled"] += 1
                continue
            metric = F(metric + a[j])
            flips.append(j)
        if v is not None and v not in FT:
            metric = F(metric + a[v])
            flips.append(v)
        if np.isinf(metric):
            count["inf-metric"] += 1
        cands.append((int(metric.view(np.uint32)), T, flips))
    pre, erased = int(e.sum()), int((x == 0).sum())
    if not cands:
        count["status2"] += 1
        return np.array([2, pre, pre, 0, erased, int(e[:K].sum())], np.int64), e
    best = min(cands, key=lambda c: (c[0], c[1]))
    if sum(c[0] == best[0] for c in cands) > 1:
        count["metric-tie"] += 1
    if best[1] > 0:
        count["winner-T>0"] += 1
    e = e.copy()
    e[best[2]] ^= True
    status, post = int(bool(best[2])), int(e.sum())
    assert (status == 0) == (s0 == 0)
    count[f"status{status}"] += 1
    if status == 1 and post:
        count["miscorrected"] += 1
    if status == 0 and pre:
        count["undetected"] += 1
    return np.array([status, pre, post, len(best[2]), erased, int(e[:K].sum())], np.int64), e


def dense_H(cols, r):
    return np.array([[(int(c) >> k) & 1 for c in cols] for k in range(r)], np.uint8)


def word_search(cols, r, p, K, x, b):
    """(b) for one codeword of n <= 20 bits: the same figures without a syndrome table."""
    n = len(cols)
    assert n <= 20
    H = dense_H(cols, r)
    x, a, e = _inputs(x, b)
    taken, least = np.zeros(n, bool), []
    for _ in range(p):                                         # the smallest a not yet taken; a strict < keeps the smallest j among equals
        pick = None
        for j in range(n):
            if not taken[j] and (pick is None or a[j] < a[pick]):
                pick = j
        taken[pick] = True
        least.append(pick)
    best = None
    for T in range(1 << p):
        members = [least[i] for i in range(p) if (T >> i) & 1]
        flipped = e.copy()
        flipped[members] ^= True
        found = []                                             # the codewords within distance 1 of the flipped word: -1 = the word itself
        for v in range(-1, n):
            cand = flipped.copy()
            if v >= 0:
                cand[v] ^= True
            if not (H @ cand.astype(np.uint8) % 2).any():
                found.append(v)
        assert len(found) <= 1                                 # distinct non-zero columns: at most one
        if not found:
            continue
        v = found[0]
        flips = [j for j in members if j != v] + ([v] if v >= 0 and v not in members else [])
        metric = F(0.0)
        for j in flips:
            metric = F(metric + a[j])
        key = (float(metric), T)
        if best is None or key < best[0]:
            best = key, flips
    pre, erased = int(e.sum()), int((x == 0).sum())
    if best is None:
        return np.array([2, pre, pre, 0, erased, int(e[:K].sum())], np.int64), e
    e = e.copy()
    e[best[1]] ^= True
    return np.array([int(bool(best[1])), pre, int(e.sum()), len(best[1]), erased, int(e[:K].sum())], np.int64), e


def gather(t, t0, C, n, depth):
    """t[R, w, N] -> [R, C, n]: the bit-packed map (depth 0) or the symbol interleaver over groups of `depth` codewords."""
    return IL.codewords_il(t, t0, C, n, depth) if depth else M.codewords(t, t0, C, n)


def stream_index(C, K, spread):
    """-> u[C, K]: where payload bit i of codeword c lies in the run's stream."""
    c, i = np.arange(C)[:, None], np.arange(K)[None, :]
    return i * C + c if spread else c * K + i


def decode(llr, bits, cols, p, K, t0, C, depth=0, spread=1, count=None):
    """(a) over device-layout tensors llr[R, w, N] float32, bits[R, w, N] int8 -> (out[R, C, 6] int64, stream llr[R, C K] float32, stream bits
    [R, C K] int8, the Counter)."""
    count = collections.Counter() if count is None else count
    n, R = len(cols), llr.shape[0]
    x, tx = gather(llr, t0, C, n, depth), gather(bits, t0, C, n, depth).astype(bool)
    out = np.zeros((R, C, 6), np.int64)
    s_llr, s_bits = np.zeros((R, C * K), F), np.zeros((R, C * K), np.int8)
    u = stream_index(C, K, spread)
    for r in range(R):
        for c in range(C):
            out[r, c], e = word(cols, p, K, x[r, c], tx[r, c], count)
            s_bits[r, u[c]] = tx[r, c, :K]
            s_llr[r, u[c]] = np.where(tx[r, c, :K] ^ e[:K], F(-1.0), F(1.0))
    return out, s_llr, s_bits, count


def figures(out, n, K):
    """The per-run figures of engine.chase_decode from out[R, C, 6], as it forms them: float64 quotients rounded to float32."""
    C = out.shape[1]
    return dict(BER_post=(out[..., 2].sum(1) / np.float64(C * n)).astype(F), BER_pre=(out[..., 1].sum(1) / np.float64(C * n)).astype(F),
                BER_payload=(out[..., 5].sum(1) / np.float64(C * K)).astype(F), FER=((out[..., 2] > 0).sum(1) / np.float64(C)).astype(F),
                miscorrected=((out[..., 0] == 1) & (out[..., 2] > 0)).sum(1), undetected=((out[..., 0] == 0) & (out[..., 1] > 0)).sum(1))

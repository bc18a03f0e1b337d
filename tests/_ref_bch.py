"""The integer model of vaeq_bch_outer (include/vaeq.h): a bounded-distance decoder of a shortened narrow-sense binary BCH code over the payload
bits of the LDPC decoders' `post`, against the TX bits under the decoders' own map.

tables(), parity()   GF(2^m) from the header's polynomials; the generator's degree from the cyclotomic cosets;
decode()             one error pattern: syndromes, Berlekamp-Massey on Python integers, a root search over all 2^m - 1 positions and the header's
                     three-status rule in its locator form, with a counter for every branch;
Table                an independent restatement for small codes: no locator at all, but the header's rule word for word -- a table from the 2t
                     syndromes to the unique pattern of weight <= t inside [0, n_o), built by enumeration; tests/test_ref_bch_host.py holds the
                     two to each other;
stream_map()         where position p of outer codeword a lies in the payload stream: (LDPC codeword, bit) per (a, p), both spreads;
errors(), outer()    the error patterns of device-layout tensors (the TX-bit map is tests/_ref_ldpc.py's and tests/_ref_ldpc_il.py's) and the
                     model over them: out[R, C_o, 4], loc[R, C_o, t], and the counters.
"""
import collections
import functools
import itertools

import numpy as np

import _ref_ldpc as M
import _ref_ldpc_il as IL

POLY = {4: 0x13, 5: 0x25, 6: 0x43, 7: 0x89, 8: 0x11D, 9: 0x211, 10: 0x409, 11: 0x805, 12: 0x1053, 13: 0x201B}
PARITY = {(4, 1): 4, (4, 2): 8, (4, 3): 10, (5, 3): 15, (6, 3): 18, (8, 2): 16, (8, 4): 32, (10, 8): 80, (13, 12): 156, (13, 16): 208}
SMALL = ((4, 2, 15), (4, 3, 15), (4, 2, 11), (4, 3, 9), (5, 3, 31), (5, 3, 23))   # (m, t, n_o): the cases the header's locator test was checked on


@functools.lru_cache(maxsize=None)
def tables(m):
    """-> (exp[2 q] int64 with exp[k] = alpha^k, log[q + 1] int64 with log[0] unused), q = 2^m - 1."""
    q = (1 << m) - 1
    exp, log = np.zeros(2 * q, np.int64), np.zeros(q + 1, np.int64)
    x = 1
    for k in range(q):
        exp[k] = exp[k + q] = x
        log[x] = k
        x <<= 1
        if x >> m:
            x ^= POLY[m]
    return exp, log


def order_of_alpha(m):
    """The least k >= 1 with alpha^k = 1, by stepping (no table)."""
    x, k = 2, 1
    while x != 1:
        x <<= 1
        if x >> m:
            x ^= POLY[m]
        k += 1
    return k


def parity(m, t):
    q = (1 << m) - 1
    seen = set()
    for j in range(1, 2 * t + 1):
        x = j % q
        while x not in seen:
            seen.add(x)
            x = 2 * x % q
    return len(seen)


def syndromes(m, t, positions):
    """-> [S_1, .., S_2t] of the error positions."""
    exp, _ = _lists(m)
    q = (1 << m) - 1
    S = []
    for j in range(1, 2 * t + 1):
        s = 0
        for p in positions:
            s ^= exp[j * p % q]
        S.append(s)
    return S


@functools.lru_cache(maxsize=None)
def _lists(m):
    """tables(m) as Python lists, for the scalar arithmetic."""
    return tuple(x.tolist() for x in tables(m))


def _mul(m, a, b):
    exp, log = _lists(m)
    return exp[log[a] + log[b]] if a and b else 0


def _inv(m, a):
    exp, log = _lists(m)
    return exp[((1 << m) - 1 - log[a]) % ((1 << m) - 1)]


def locator(m, S):
    """Berlekamp-Massey over the syndromes S_1 .. S_2t -> (Lambda as a list of coefficients, Lambda[0] = 1; L)."""
    lam, B, L, b, gap = [1], [1], 0, 1, 1
    for r in range(len(S)):
        d = S[r]
        for i in range(1, L + 1):
            if i < len(lam):
                d ^= _mul(m, lam[i], S[r - i])
        if d == 0:
            gap += 1
            continue
        coef = _mul(m, d, _inv(m, b))
        new = lam + [0] * max(0, len(B) + gap - len(lam))
        for i, x in enumerate(B):
            new[i + gap] ^= _mul(m, coef, x)
        if 2 * L <= r:
            L, B, b, gap = r + 1 - L, lam, d, 1
        else:
            gap += 1
        lam = new
    return lam, L


def roots(m, lam):
    """The positions p in 0 .. q - 1 with Lambda(alpha^(-p)) = 0, ascending (all positions at once)."""
    exp, log = tables(m)
    q = (1 << m) - 1
    g = (q - np.arange(q)) % q
    val = np.zeros(q, np.int64)
    for k, c in enumerate(lam):
        if c:
            val ^= exp[(int(log[c]) + k * g) % q]
    return np.nonzero(val == 0)[0]


def decode(m, t, n_o, positions, count=None):
    """One error pattern (its positions, all below n_o) -> (status, the flipped positions ascending).  count: a Counter of the branches taken."""
    count = collections.Counter() if count is None else count
    S = syndromes(m, t, positions)
    if not any(S):
        count["status0"] += 1
        count["undetected"] += len(positions) > 0
        return 0, []
    lam, L = locator(m, S)
    if L > t:
        count["status2"] += 1
        count["L>t"] += 1
        return 2, []
    rt = roots(m, lam)
    if len(rt) != L:
        count["status2"] += 1
        count["roots<L"] += 1
        return 2, []
    if (rt >= n_o).any():
        count["status2"] += 1
        count["shortened-root"] += 1
        return 2, []
    count["status1"] += 1
    count["miscorrected"] += sorted(int(p) for p in rt) != sorted(positions)
    return 1, [int(p) for p in rt]


class Table:
    """The header's rule for a small code with no locator: syndromes -> the unique set of at most t positions below n_o that has them."""

    def __init__(self, m, t, n_o):
        self.m, self.t, self.n_o = m, t, n_o
        exp, _ = tables(m)
        q = (1 << m) - 1
        col = [tuple(int(exp[j * p % q]) for j in range(1, 2 * t + 1)) for p in range(n_o)]
        self.col, self.table = col, {}
        for wt in range(1, t + 1):
            for pos in itertools.combinations(range(n_o), wt):
                s = self.of(pos)
                assert s not in self.table and any(s), "the set of at most t positions is unique"
                self.table[s] = list(pos)

    def of(self, positions):
        s = [0] * (2 * self.t)
        for p in positions:
            s = [a ^ b for a, b in zip(s, self.col[p])]
        return tuple(s)

    def decode(self, positions):
        s = self.of(positions)
        if not any(s):
            return 0, []
        return (1, self.table[s]) if s in self.table else (2, [])


def stream_map(C_o, n_o, K, spread):
    """-> (c[C_o, n_o], i[C_o, n_o]) int64: position p of outer codeword a is bit i[a, p] of LDPC codeword c[a, p]."""
    a, p = np.arange(C_o)[:, None], np.arange(n_o)[None, :]
    u = p * C_o + a if spread else a * n_o + p
    return u // K, u % K


def errors(post, bits, t0, n, depth):
    """post[R, C, n] (float32 or int16) and bits[R, w, N] -> e[R, C, n] bool: (post < 0) against the TX bits in codeword order; depth None or 0 is
    the bit-packed map, an int >= 1 the symbol interleaver's.  A NaN and +-0 are bit 0."""
    C = post.shape[1]
    tx = IL.codewords_il(bits, t0, C, n, depth) if depth else M.codewords(bits, t0, C, n)
    with np.errstate(invalid="ignore"):
        return (post < 0) != (tx & 1).astype(bool)


def outer(post, bits, m, t, n_o, C_o, K, spread, t0=0, depth=None, memo=None):
    """-> (out[R, C_o, 4] int64 = status, pre_err, post_err, nflip; loc[R, C_o, t] int16; the Counter of the branches).  memo: a dict that
    keeps decode()'s answer and branches per error pattern, for tensors of many thousand codewords drawn from few patterns."""
    R, C, n = post.shape
    assert C_o * n_o <= C * K and 1 <= K <= n
    e = errors(post, bits, t0, n, depth)
    c, i = stream_map(C_o, n_o, K, spread)
    out, loc, count = np.zeros((R, C_o, 4), np.int64), np.full((R, C_o, t), -1, np.int16), collections.Counter()
    for r in range(R):
        pat = e[r][c, i]                                        # [C_o, n_o]
        for a in range(C_o):
            pos = [int(p) for p in np.nonzero(pat[a])[0]]
            if memo is None:
                status, flips = decode(m, t, n_o, pos, count)
            else:
                key = (m, t, n_o, tuple(pos))
                if key not in memo:
                    own = collections.Counter()
                    memo[key] = decode(m, t, n_o, pos, own) + (own,)
                status, flips, own = memo[key]
                count.update(own)
            left = set(pos) ^ set(flips)
            out[r, a] = status, len(pos), len(left), len(flips)
            loc[r, a, :len(flips)] = flips
    return out, loc, count


def figures(out, n_o):
    """The per-run figures engine.bch_outer derives from out[R, C_o, 4]."""
    C_o = out.shape[1]
    tot = float(C_o * n_o)
    return dict(BER_outer=(out[..., 2].sum(1) / tot).astype(np.float32), BER_in=(out[..., 1].sum(1) / tot).astype(np.float32),
                FER_outer=((out[..., 2] > 0).sum(1) / float(C_o)).astype(np.float32),
                miscorrected=((out[..., 0] == 1) & (out[..., 2] > 0)).sum(1), undetected=((out[..., 0] == 0) & (out[..., 1] > 0)).sum(1))


def codeword_of(m, t, n_o, rng=None):
    """The positions of the ones of a non-zero codeword of the shortened code: a non-zero vector of the null space of the 2t syndrome rows over
    GF(2) (m bits each), by elimination.  None if the shortened code holds only the zero word."""
    exp, _ = tables(m)
    q = (1 << m) - 1
    rows = []                                                  # one GF(2) row per syndrome bit, as Python integers over the n_o positions
    for j in range(1, 2 * t + 1):
        colv = exp[j * np.arange(n_o) % q]
        for bit in range(m):
            rows.append(int.from_bytes(np.packbits(((colv >> bit) & 1).astype(np.uint8), bitorder="little").tobytes(), "little"))
    pivots = {}                                                # pivot column -> its reduced row
    for rw in rows:
        for pc, pr in pivots.items():
            if (rw >> pc) & 1:
                rw ^= pr
        if rw:
            pc = rw.bit_length() - 1
            for k in list(pivots):
                if (pivots[k] >> pc) & 1:
                    pivots[k] ^= rw
            pivots[pc] = rw
    free = [p for p in range(n_o) if p not in pivots]
    if not free:
        return None
    f = free[0] if rng is None else free[int(rng.integers(len(free)))]
    word = 1 << f                                              # the free bit set, every pivot bit solved for
    for pc, pr in pivots.items():
        if (pr >> f) & 1:
            word |= 1 << pc
    pos = [p for p in range(n_o) if (word >> p) & 1]
    assert not any(syndromes(m, t, pos))
    return pos

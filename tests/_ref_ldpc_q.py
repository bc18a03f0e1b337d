"""The integer model of vaeq_ldpc_decode_q (include/vaeq.h): layered min-sum with q-bit channel LLRs, q-bit check messages and saturating
a-posteriori values.  The quantiser is the only float arithmetic (numpy float32, each operation rounded on its own); behind it every value is
an integer and the header fixes every rounding, clamp and tie, so the kernel has to reproduce every bit.

quantise()        llr -> Q, the header's quantiser;
decode()          one codeword, vectorised over the Z checks of a layer, with the compressed state (m1, m2, idx, signs) as the kernel stores
                  it; `stats` (a dict) counts how often each rule of the header binds;
decode_scalar()   an independent restatement: walks the dense H row by row and edge by edge with one explicit integer message per edge and no
                  compressed state -- tests/test_ref_ldpc_q_host.py holds the two to each other in every counter and every final L;
make_case_q()     _ref_ldpc.make_case's inputs with, per run and inside the codewords, LLRs of exactly +-0.5 / scale, +-1.5 / scale and
                  +-2.5 / scale (ties of the rounding: random data never hits one), one +inf and, unless nan=False, one NaN;
make_case_il_q()  the same on _ref_ldpc_il.make_case_il's inputs, planted through the interleaver's map.
A parameter set is dict(bits, scale, app_bits, num, beta): SETS holds the five of the tests.
"""
import functools

import numpy as np

import _ref_ldpc as M
import _ref_ldpc_il as IL

F = np.float32
SETS = {
    "A": dict(bits=5, scale=1.0, app_bits=7, num=6, beta=0),
    "B": dict(bits=4, scale=0.5, app_bits=4, num=8, beta=1),
    "C": dict(bits=8, scale=8.0, app_bits=15, num=6, beta=0),
    "D": dict(bits=2, scale=0.125, app_bits=4, num=8, beta=0),
    "E": dict(bits=6, scale=2.0, app_bits=6, num=5, beta=2),
}
STATS = ("channel_clamp", "message_clamp", "app_clamp", "f_zero", "tie_not_first", "t_zero", "half", "nan")
PLANTED = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, np.inf, np.nan)


def limits(prm):
    """-> (Cmax = Mmax, Lmax)."""
    return 2 ** (prm["bits"] - 1) - 1, 2 ** (prm["app_bits"] - 1) - 1


def quantise(llr, prm, stats=None):
    cmax, _ = limits(prm)
    with np.errstate(all="ignore"):
        x = (np.asarray(llr, F) * F(prm["scale"])).astype(F)
        nan = np.isnan(x)
        x = np.where(nan, F(0.0), x).astype(F)
        y = np.minimum(np.maximum(x, F(-cmax)), F(cmax)).astype(F)
        Q = np.rint(y).astype(np.int64)                        # ties to even
    if stats is not None:
        stats["nan"] += int(nan.sum())
        stats["channel_clamp"] += int((np.abs(x) > cmax).sum())
        stats["half"] += int((np.abs(y - np.trunc(y)) == F(0.5)).sum())
    return Q


def _f(mag, prm):
    return np.maximum(((prm["num"] * mag + 4) >> 3) - prm["beta"], 0)


def _satisfied(L, layers, sigma):
    return all(not ((np.bitwise_xor.reduce(L[V] < 0, axis=0)) ^ sg).any() for V, sg in zip(layers, sigma))


def decode(shifts, Z, llr, bits, prm, max_iter=20, stats=None):
    """-> (out[5] = iters, ok, post_err, pre_err, erased; post[n] int16)."""
    shifts = np.asarray(shifts)
    mmax, lmax = limits(prm)
    raw = np.asarray(llr, F)
    bits = np.asarray(bits).astype(bool)
    L = quantise(raw, prm, stats)
    with np.errstate(invalid="ignore"):
        pre_err = int(((raw < 0) != bits).sum())               # of the raw input; a NaN is bit 0
    erased = int((L == 0).sum())
    layers = M._layers(shifts, Z)
    sigma = [np.bitwise_xor.reduce(bits[V], axis=0) for V in layers]
    z = lambda: np.zeros(Z, np.int64)
    st = [dict(m1=z(), m2=z(), idx=z(), sg=np.zeros(V.shape, bool)) for V in layers]
    ar = np.arange(Z)
    iters, ok = 0, _satisfied(L, layers, sigma)
    while not ok and iters < max_iter:
        for V, sgm, s in zip(layers, sigma, st):
            e = np.arange(V.shape[0])[:, None]
            mag = _f(np.where(e == s["idx"], s["m2"], s["m1"]), prm)
            t = L[V] - np.where(s["sg"], -mag, mag)
            A = np.minimum(np.abs(t), mmax)
            idx = np.argmin(A, axis=0)                         # the first edge that attains the minimum, after the clamp
            m1 = A[idx, ar]
            A2 = A.copy()
            A2[idx, ar] = 1 << 20
            m2 = A2.min(axis=0)
            neg = t < 0
            S = np.bitwise_xor.reduce(neg, axis=0) ^ sgm
            nmag = _f(np.where(e == idx, m2, m1), prm)
            nsg = S ^ neg
            u = t + np.where(nsg, -nmag, nmag)
            L[V] = np.clip(u, -lmax, lmax)
            if stats is not None:
                stats["message_clamp"] += int((np.abs(t) > mmax).sum())
                stats["app_clamp"] += int((np.abs(u) > lmax).sum())
                stats["f_zero"] += int(((_f(m1, prm) == 0) & (m1 > 0)).sum() + ((_f(m2, prm) == 0) & (m2 > 0)).sum())
                stats["tie_not_first"] += int((((A == m1).sum(axis=0) > 1) & (idx > 0)).sum())
                stats["t_zero"] += int((t == 0).sum())
            s.update(m1=m1, m2=m2, idx=idx, sg=nsg)
        iters += 1
        ok = _satisfied(L, layers, sigma)
    return np.array([iters, int(ok), int(((L < 0) != bits).sum()), pre_err, erased], np.int64), L.astype(np.int16)


def decode_scalar(shifts, Z, llr, bits, prm, max_iter=20):
    """The same figures from the dense H, one check and one edge at a time, with the full message of every edge kept as a Python int."""
    H = M.dense_H(np.asarray(shifts), Z)
    rows = [[int(v) for v in np.nonzero(h)[0]] for h in H]     # ascending variable = ascending block column: one edge per block
    cmax = mmax = 2 ** (prm["bits"] - 1) - 1
    lmax = 2 ** (prm["app_bits"] - 1) - 1
    num, beta, scale = int(prm["num"]), int(prm["beta"]), F(prm["scale"])
    b = [int(x) & 1 for x in bits]
    L = []
    pre_err = 0
    for x, y in zip(np.asarray(llr, F), b):
        pre_err += int(bool(x < 0)) != y
        with np.errstate(all="ignore"):
            v = F(x * scale)
        if v != v:
            v = F(0.0)
        v = F(min(max(v, F(-cmax)), F(cmax)))
        lo = int(np.floor(v))
        d = float(v) - lo                                      # exact: |v| <= 127 in float32
        L.append(lo if d < 0.5 else lo + 1 if d > 0.5 else lo + (lo & 1))   # a tie goes to the even neighbour
    erased = sum(x == 0 for x in L)
    sigma = [sum(b[v] for v in r) & 1 for r in rows]
    msg = [[0] * len(r) for r in rows]

    def f(a):
        return max(((num * a + 4) >> 3) - beta, 0)

    def test():
        return all((sum(int(L[v] < 0) for v in r) & 1) == sg for r, sg in zip(rows, sigma))

    iters, ok = 0, test()
    while not ok and iters < max_iter:
        for i, r in enumerate(rows):                           # rows in order = layers in order, and the checks of a layer in any order
            t = [L[v] - msg[i][k] for k, v in enumerate(r)]
            mags = [min(abs(x), mmax) for x in t]
            first = mags.index(min(mags))
            m1 = mags[first]
            m2 = min(x for k, x in enumerate(mags) if k != first)
            S = (sum(int(x < 0) for x in t) + sigma[i]) & 1
            for k, v in enumerate(r):
                mag = f(m2 if k == first else m1)
                msg[i][k] = -mag if S ^ int(t[k] < 0) else mag
                L[v] = min(max(t[k] + msg[i][k], -lmax), lmax)
        iters += 1
        ok = test()
    return np.array([iters, int(ok), sum(int(x < 0) != y for x, y in zip(L, b)), pre_err, erased], np.int64), np.array(L, np.int16)


def _plant(llr, seed, scale, R, where, total, nan):
    """Per run, at len(PLANTED) distinct codeword bits g (where(g) -> plane, symbol): the planted values over the scale."""
    rng = np.random.default_rng(seed)
    for r in range(R):
        g = rng.choice(total, len(PLANTED), replace=False)
        for k, val in zip(g, PLANTED):
            if val != val and not nan:
                continue
            p, s = where(int(k))
            llr[r, p, s] = F(val / scale)
    return llr


def make_case_q(seed, n, sigma, R, C, w, t0, scale, nan=True, erasures=4):
    llr, bits = M.make_case(seed, n, sigma, R, C, w, t0, erasures)
    return _plant(llr.copy(), seed + 7777, scale, R, lambda g: (g % w, t0 + g // w), C * n, nan), bits


def make_case_il_q(seed, n, sigma, R, C, w, t0, depth, scale, nan=True, erasures=4):
    llr, bits = IL.make_case_il(seed, n, sigma, R, C, w, t0, depth, erasures)
    sym, plane = IL.il_map(t0, C, n, w, depth)
    return _plant(llr.copy(), seed + 7777, scale, R, lambda g: (int(plane.ravel()[g]), int(sym.ravel()[g])), C * n, nan), bits


def decode_batch(shifts, Z, llr, bits, t0, C, prm, max_iter=20, depth=0, stats=None):
    """-> (out[R,C,5] int64, post[R,C,n] int16) of device-layout tensors llr[R,w,N], bits[R,w,N]; depth >= 1: behind the interleaver."""
    n = shifts.shape[1] * Z
    if depth:
        lc, bc = IL.codewords_il(llr, t0, C, n, depth), IL.codewords_il(bits, t0, C, n, depth)
    else:
        lc, bc = M.codewords(llr, t0, C, n), M.codewords(bits, t0, C, n)
    res = [[decode(shifts, Z, lc[r, c], bc[r, c], prm, max_iter, stats) for c in range(C)] for r in range(llr.shape[0])]
    return np.array([[o for o, _ in row] for row in res]), np.array([[p for _, p in row] for row in res])


# ------------------------------------------------------------------ the cases of tests/test_ldpc_q_gpu.py, built and decoded once
@functools.lru_cache(maxsize=None)
def case(code, w, t0, level, name, nan=True):
    shifts, Z = M.CODES[code]
    return make_case_q(M.case_seed(code, w, t0, level), shifts.shape[1] * Z, M.SIGMAS[level], M.R_, M.C_, w, t0, SETS[name]["scale"], nan)


@functools.lru_cache(maxsize=None)
def expected(code, w, t0, level, name, max_iter, nan=True):
    shifts, Z = M.CODES[code]
    llr, bits = case(code, w, t0, level, name, nan)
    return decode_batch(shifts, Z, llr, bits, t0, M.C_, SETS[name], max_iter)


@functools.lru_cache(maxsize=None)
def case_il(code, w, t0, level, depth, name):
    shifts, Z = M.CODES[code]
    return make_case_il_q(IL.case_seed(code, w, t0, level, depth), shifts.shape[1] * Z, M.SIGMAS[level], M.R_, M.C_, w, t0, depth, SETS[name]["scale"])


@functools.lru_cache(maxsize=None)
def expected_il(code, w, t0, level, depth, name, max_iter):
    shifts, Z = M.CODES[code]
    llr, bits = case_il(code, w, t0, level, depth, name)
    return decode_batch(shifts, Z, llr, bits, t0, M.C_, SETS[name], max_iter, depth)

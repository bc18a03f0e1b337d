"""The model of vaeq_ldpc_decode_il (include/vaeq.h): the symbol interleaver over groups of `depth` codewords in plain numpy, in front of
tests/_ref_ldpc.py's float32 decoder.

il_map()          where the interleaver puts every codeword bit: (symbol, plane) per (codeword, bit), from the header's words, one codeword
                  and one bit at a time;
codewords_il()    the codeword-order view of a device-layout tensor under that map;
decode_batch_il() _ref_ldpc.decode over it;
make_case_il()    _ref_ldpc.make_case's inputs at N = t0 + C S exactly (a read past the last symbol leaves the buffer), with the planes that
                  belong to no codeword made loud: a large negative LLR against a 0 bit (counting one changes pre_err), one of them an exact
                  zero (counting it changes erased).
"""
import functools

import numpy as np

import _ref_ldpc as M

F = np.float32
LOUD = F(-1.0e4)


def symbols_per_codeword(n, w):
    return -(-n // w)


def il_map(t0, C, n, w, depth):
    """-> (sym[C, n], plane[C, n]) int64: bit j of codeword c sits at symbol sym[c, j], plane plane[c, j]."""
    S = symbols_per_codeword(n, w)
    sym, plane = np.empty((C, n), np.int64), np.empty((C, n), np.int64)
    for c in range(C):
        k = c // depth                                          # the group, its size (ragged at the end), the local index
        D = min((k + 1) * depth, C) - k * depth
        d = c - k * depth
        base = t0 + k * depth * S
        for j in range(n):
            sym[c, j] = base + (j // w) * D + d
            plane[c, j] = j % w
    return sym, plane


def codewords_il(x, t0, C, n, depth):
    """x[R,w,N] -> [R,C,n] under il_map."""
    sym, plane = il_map(t0, C, n, x.shape[1], depth)
    return np.ascontiguousarray(x[:, plane, sym])


def decode_batch_il(shifts, Z, llr, bits, t0, C, depth, max_iter=20, alpha=0.75):
    """-> (out[R,C,5] int64, post[R,C,n] float32) of device-layout tensors llr[R,w,N], bits[R,w,N]."""
    n = shifts.shape[1] * Z
    lc, bc = codewords_il(llr, t0, C, n, depth), codewords_il(bits, t0, C, n, depth)
    res = [[M.decode(shifts, Z, lc[r, c], bc[r, c], max_iter, alpha) for c in range(C)] for r in range(llr.shape[0])]
    return np.array([[o for o, _ in row] for row in res]), np.array([[p for _, p in row] for row in res])


def unused(t0, C, n, w, depth):
    """-> mask[w, N] bool at N = t0 + C S: the (plane, symbol) pairs behind t0 that belong to no codeword."""
    S = symbols_per_codeword(n, w)
    sym, plane = il_map(t0, C, n, w, depth)
    m = np.ones((w, t0 + C * S), bool)
    m[:, :t0] = False
    m[plane, sym] = False
    return m


def make_case_il(seed, n, sigma, R, C, w, t0, depth, erasures=4):
    """llr[R,w,N] float32, bits[R,w,N] int8 with N = t0 + C ceil(n / w): random TX bits, llr = 2 y / sigma^2 in float32 of y = (1 - 2 b) + sigma
    noise, `erasures` entries per run inside the codewords forced to +0.0; every unused plane LOUD against a 0 bit, the first one of a run 0.0."""
    rng = np.random.default_rng(seed)
    N = t0 + C * symbols_per_codeword(n, w)
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    y = (1.0 - 2.0 * bits) + sigma * rng.standard_normal((R, w, N))
    llr = (2.0 * y / sigma ** 2).astype(F)
    sym, plane = il_map(t0, C, n, w, depth)
    for r in range(R):
        g = rng.choice(C * n, erasures, replace=False)
        llr[r, plane.ravel()[g], sym.ravel()[g]] = F(0.0)
    m = unused(t0, C, n, w, depth)
    if m.any():
        llr[:, m] = LOUD
        bits[:, m] = 0
        p, s = (int(a[0]) for a in np.nonzero(m))
        llr[:, p, s] = F(0.0)
    return llr, bits


# ------------------------------------------------------------------ the cases of tests/test_ldpc_il_gpu.py, built and decoded once
DEPTHS = (1, 2, 5)                                         # of C = 5: symbol-aligned contiguous; groups of 2, 2 and a ragged 1; the whole frame


def case_seed(code, w, t0, level, depth):
    return 50000 + 10 * M.case_seed(code, w, t0, level) + depth


@functools.lru_cache(maxsize=None)
def case(code, w, t0, level, depth):
    shifts, Z = M.CODES[code]
    return make_case_il(case_seed(code, w, t0, level, depth), shifts.shape[1] * Z, M.SIGMAS[level], M.R_, M.C_, w, t0, depth)


@functools.lru_cache(maxsize=None)
def expected(code, w, t0, level, depth, max_iter):
    shifts, Z = M.CODES[code]
    llr, bits = case(code, w, t0, level, depth)
    return decode_batch_il(shifts, Z, llr, bits, t0, M.C_, depth, max_iter)


@functools.lru_cache(maxsize=None)
def expected_old(code, w, t0, level, depth, max_iter):
    """The contiguous decoder's model on the same tensors."""
    shifts, Z = M.CODES[code]
    llr, bits = case(code, w, t0, level, depth)
    return M.decode_batch(shifts, Z, llr, bits, t0, M.C_, max_iter)

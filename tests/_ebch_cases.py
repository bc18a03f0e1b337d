"""The cases of tests/test_ref_ebch_host.py, tests/test_chase_bch_gpu.py and tests/test_tpc_bch_gpu.py, built once: device-layout tensors with
everything the rules of vaeq_chase_bch_decode and vaeq_tpc_bch_decode (include/vaeq.h) distinguish, and what tests/_ref_ebch.py makes of them.

The codes (m, n, extended): the plain (15, 7) and the extended (16, 7) code; n_i = 9 extended (k = 1, n = 10: every pattern but a handful has no
candidate); m = 5 extended (32); m = 6 extended (64: exactly one lane slot); m = 7 with n_i = 64 extended (65: a ragged second slot); m = 7
extended (128); m = 8 plain (255), shortened to n_i = 200 and extended (256: four slots); n_i = 16 of m = 5 extended (17) for the products.
The tensors are those of tests/_chase_cases.py and tests/_tpc_cases.py: BPSK + AWGN LLRs in float32, every third word (block) rounded to
integers (ties), one word (block) per run with a NaN, +-0 and +-inf, run 1's block 0 noiseless in the product cases, and every entry outside
the used span loud and wrong.  sigma is larger than in those files: a t = 2 word has to meet three and more errors.
"""
import collections
import functools

import numpy as np

import _ref_ebch as E
import _ref_ldpc_il as IL
import _ref_tpc as T

F = np.float32
LOUD = F(50.0)

CODES = {
    "b15": E.Code(4, 15, False), "x16": E.Code(4), "x10": E.Code(4, 10), "x32": E.Code(5), "x64": E.Code(6), "x65": E.Code(7, 65), "x128": E.Code(7),
    "b255": E.Code(8, 255, False), "x201": E.Code(8, 201), "x256": E.Code(8), "x17": E.Code(5, 17), "b200": E.Code(8, 200, False),
}
WORD_COUNTERS = ("inner-status0", "one-position", "two-positions", "no-cand-S1=0", "no-cand-no-root", "no-cand-shortened", "u-flipped", "u-kept",
                 "v-cancels", "v-listed-new", "u-listed", "status0", "status1", "status2")
TPC_COUNTERS = ("competitor", "no-competitor", "delta-zero", "clamp-r", "clamp-W", "clamp-beta", "stop-h0", "stop-odd", "stop-even", "no-stop")

# ---- vaeq_chase_bch_decode ----

ChaseCase = collections.namedtuple("ChaseCase", "name code p w t0 depth K spread sigma R C seed")
CHASE_CODES = ("b15", "x16", "x10", "x32", "x64", "x65", "x128", "b255", "b200", "x256")
PATTERNS = (0, 1, 4, 6)


def _chase_cases():
    out = []
    for ci, code in enumerate(CHASE_CODES):
        c = CODES[code]
        for pi, p in enumerate(PATTERNS):
            i = 4 * ci + pi
            w, depth = (1, 4, 12)[i % 3], (0, 2, 5)[(i // 3) % 3]
            full, spread = (i + i // 8) % 2, (i // 2) % 2
            out.append(ChaseCase(f"{code}-p{p}-w{w}-d{depth}-{'Kn' if full else 'K'}-s{spread}", code, p, w, (0, 5)[(i + ci) % 2], depth,
                                 c.n if full else c.k, spread, (0.7, 0.85)[(i // 4 + pi) % 2], 2 if c.n > 64 else 3, 5, 9300 + i))
    return tuple(out)


CHASE = _chase_cases()
# the grid-stride path: tiles of 8 words at n = 256 and a grid capped at 2048 workgroups: R ceil(C / 8) = 2253 tiles, a ragged last tile per run.
# p = 0 keeps the model at one locator call per word
CHASE_STRIDE = ChaseCase("x256-stride", "x256", 0, 4, 0, 0, 239, 1, 0.6, 3, 6003, 9390)
# more words than a tile holds (32): tiles that cut through the interleaver's groups of 5, a ragged last tile
CHASE_TILES = ChaseCase("x32-tiles-d5", "x32", 4, 12, 5, 5, 21, 0, 0.7, 2, 71, 9391)
CHASE_TINY = tuple(c for c in CHASE if CODES[c.code].n <= 16)


def bit_map(case, n):
    if case.depth:
        return IL.il_map(case.t0, case.C, n, case.w, case.depth)
    g = np.arange(case.C * n).reshape(case.C, n)
    return case.t0 + g // case.w, g % case.w


@functools.lru_cache(maxsize=None)
def chase_tensors(case):
    """-> (llr[R, w, N] float32, bits[R, w, N] int8)"""
    n = CODES[case.code].n
    rng = np.random.default_rng(case.seed)
    R, C, w = case.R, case.C, case.w
    N = case.t0 + C * IL.symbols_per_codeword(n, w) if case.depth else case.t0 + -(-C * n // w) + 3
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    llr = (2.0 * ((1.0 - 2.0 * bits) + case.sigma * rng.standard_normal((R, w, N))) / case.sigma ** 2).astype(F)
    sym, plane = bit_map(case, n)
    for r in range(R):
        for c in range(C):
            if (r * C + c) % 3 == 1:
                llr[r, plane[c], sym[c]] = np.rint(llr[r, plane[c], sym[c]])
        c = (r + 1) % C
        pos = rng.choice(n, 5, replace=False)
        llr[r, plane[c, pos], sym[c, pos]] = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], F)
        if r == 0:
            bits[r, plane[c, pos[3]], sym[c, pos[3]]] = 1      # an error of infinite reliability
    used = np.zeros((w, N), bool)
    used[plane, sym] = True
    llr[:, ~used] = np.where(bits[:, ~used] == 1, LOUD, -LOUD)
    return llr, bits


@functools.lru_cache(maxsize=None)
def chase_expected(case):
    """-> (out[R, C, 6], stream llr[R, C K], stream bits[R, C K], the Counter) of model (1)."""
    llr, bits = chase_tensors(case)
    return E.decode_chase(llr, bits, CODES[case.code], case.p, case.K, case.t0, case.C, case.depth, case.spread)


# ---- vaeq_tpc_bch_decode ----

TpcCase = collections.namedtuple("TpcCase", "name col row p iters w t0 R C sigma clip scale K1 K2 seed")
# 10 x 16; (16, 7)^2; (32, 21)^2; 65 x 64, just above the 4096-bit boundary of the wave count; 256 x 17 (m = 8 by m = 5)
SMALL = (("x10", "x16", 3, 3, 0.9), ("x16", "x16", 3, 3, 0.9), ("x32", "x32", 2, 3, 0.85), ("x65", "x64", 2, 2, 0.8), ("x256", "x17", 2, 2, 0.8))


def _tpc_cases():
    out = []
    for ci, (col, row, R, C, sigma) in enumerate(SMALL):
        c1, c2 = CODES[col], CODES[row]
        big = c1.n * c2.n > 1024
        for pi, p in enumerate(PATTERNS):
            i = 4 * ci + pi
            iters, w, t0 = (1, 2, 4)[(i + ci) % 3], (1, 4, 12)[(i // 2 + pi) % 3], (0, 5)[(i + ci) % 2]
            if big:
                iters = min(iters, 2)
            small_clip = i % 2 == 1
            scale = (0.7, 9.0, 1.3)[:R] if small_clip else None if i % 4 == 2 else (0.5, 2.0, 1.0)[:R]
            out.append(TpcCase(f"{col}x{row}-p{p}-i{iters}-w{w}-t{t0}-{'clip6' if small_clip else 'clip2^60'}", col, row, p, iters, w, t0, R, C, sigma,
                               6.0 if small_clip else 2.0 ** 60, scale, c1.k if i % 3 else c1.n, c2.k if i % 3 else c2.n, 9400 + i))
    return tuple(out)


TPC = _tpc_cases()
# the largest state and the launch above 64 KiB: the extended (128, 113)^2 block, shared tables
TPC_LARGE = (TpcCase("x128xx128-p1-i1-w4-t5-clip2^60", "x128", "x128", 1, 1, 4, 5, 1, 2, 0.6, 2.0 ** 60, (2.0,), 113, 113, 9450),
             TpcCase("x128xx128-p2-i2-w12-t0-clip6", "x128", "x128", 2, 2, 12, 0, 1, 2, 0.6, 6.0, (9.0,), 128, 128, 9451))
# the grid-stride path: 1027 blocks of 10 x 10 on a grid capped at 1024 workgroups
TPC_STRIDE = TpcCase("x10xx10-stride", "x10", "x10", 1, 2, 4, 5, 1, 1027, 0.8, 2.0 ** 60, (1.0,), 1, 1, 9460)
# model (2) follows these: both component codes have n <= 16.  The last one is there for a beta above the clip in reach of model (2)
TPC_TINY = tuple(c for c in TPC if CODES[c.col].n <= 16 and CODES[c.row].n <= 16) + (
    TpcCase("x16xx10-p0-i3-w4-t5-clip6", "x16", "x10", 0, 3, 4, 5, 3, 3, 0.9, 6.0, (0.7, 1.3, 9.0), 7, 1, 9470),)
# the fixed-seed turbo-gain statement of tests/test_ref_ebch_host.py
AWGN = TpcCase("x32xx32-awgn", "x32", "x32", 4, 4, 1, 0, 1, 4, 0.85, 2.0 ** 60, None, 21, 21, 7)


def schedules(case):
    return T.schedule(T.ALPHA, case.iters), T.schedule(T.BETA, case.iters)


def scale_of(case, llr, plain=False):
    if plain:
        return np.abs(llr).reshape(llr.shape[0], -1).mean(1, dtype=F)
    return None if case.scale is None else np.array(case.scale, F)


@functools.lru_cache(maxsize=None)
def tpc_tensors(case, plain=False):
    """-> (llr[R, w, N] float32, bits[R, w, N] int8); plain: the AWGN LLRs alone."""
    n = CODES[case.col].n * CODES[case.row].n
    rng = np.random.default_rng(case.seed)
    R, C, w = case.R, case.C, case.w
    N = case.t0 + -(-C * n // w) + (0 if plain else 3)
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    noise = rng.standard_normal((R, w, N))
    llr = (2.0 * ((1.0 - 2.0 * bits) + case.sigma * noise) / case.sigma ** 2).astype(F)
    if plain:
        return llr, bits
    g = np.arange(C * n).reshape(C, n)
    sym, plane = case.t0 + g // w, g % w
    for r in range(R):
        for c in range(C):
            if (r * C + c) % 3 == 1:
                llr[r, plane[c], sym[c]] = np.rint(llr[r, plane[c], sym[c]])
        if r == 1:
            llr[r, plane[0], sym[0]] = (2.0 * (1.0 - 2.0 * bits[r, plane[0], sym[0]]) / case.sigma ** 2).astype(F)
        c = 1 + r % (C - 1)                                    # never block 0, which is run 1's noiseless one
        pos = rng.choice(n, 5, replace=False)
        llr[r, plane[c, pos], sym[c, pos]] = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], F)
        if r == 0:
            bits[r, plane[c, pos[3]], sym[c, pos[3]]] = 1
    used = np.zeros((w, N), bool)
    used[plane, sym] = True
    llr[:, ~used] = np.where(bits[:, ~used] == 1, LOUD, -LOUD)
    return llr, bits


@functools.lru_cache(maxsize=None)
def tpc_expected(case, plain=False):
    """-> (out[R, C, 8], stream llr, stream bits, ext[R, C, n], half_err[R, C, 2 iters], the Counter) of model (1)."""
    llr, bits = tpc_tensors(case, plain)
    alpha, beta = schedules(case)
    return E.decode_tpc(llr, bits, CODES[case.col], CODES[case.row], case.p, case.iters, alpha, beta, scale_of(case, llr, plain), F(case.clip),
                        case.K1, case.K2, case.t0, case.C)

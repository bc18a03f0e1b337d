"""The cases of tests/test_ref_tpc_host.py and tests/test_tpc_gpu.py, built once: device-layout tensors with everything the specification of
vaeq_tpc_decode (include/vaeq.h) distinguishes, and what tests/_ref_tpc.py makes of them.

The blocks (column code x row code): the perfect (7, 4) code x the extended (16, 11) code, which model (2) can follow as well; 20 x 100 (the
extended codes of r = 6 and r = 8, shortened: a ragged second lane slot along the rows only); the extended (32, 26)^2 and (64, 57)^2; 256 x 60
(four slots along the columns; 16 waves); the extended (128, 120)^2, the largest state and the launch above 64 KiB.  The four smaller blocks meet
patterns 0, 1, 4 and 6 with iters in {1, 2, 4}, w in {1, 4, 12} (blocks start inside a symbol wherever n % w != 0) and t0 in {0, 5} rotating,
R <= 3, C <= 3; the two large ones run with C = 2, iters <= 2, p <= 2, which keeps the model's cost in seconds.  Every other case has a small clip
(6.0, below most |llr|: r, W' and beta all meet it; its scale is 0.7, 9.0 -- beta above the clip -- and 1.3 per run), the others clip = 2^60 and
a scale of 0.5, 2.0, 1.0 per run or none (NULL, 1.0).  p = 0 on an extended code is where a word has no candidate (status 2).

The LLRs: 2 y / sigma^2 of BPSK + AWGN in float32, sigma per case; every third block rounded to integers (ties among the least reliable
positions, between candidates and between a competitor and the winner: Delta == 0); block 0 of run 1 is noiseless (it stops at h = 0); per run
one block with a NaN, a +0, a -0, a +inf and a -inf at seeded positions; every entry outside the blocks loud and wrong.
"""
import collections
import functools

import numpy as np

import _ref_chase as X
import _ref_tpc as T

F = np.float32
LOUD = F(50.0)
COUNTERS = ("status0", "status1", "status2", "competitor", "no-competitor", "delta-zero", "clamp-r", "clamp-W", "clamp-beta", "stop-h0", "stop-odd",
            "no-stop")

CODES = {
    "h7": X.hamming_cols(3, False), "e16": X.hamming_cols(4), "e20": X.hamming_cols(5, n=20), "e100": X.hamming_cols(7, n=100),
    "e32": X.hamming_cols(5), "e64": X.hamming_cols(6), "e60": X.hamming_cols(6, n=60), "e256": X.hamming_cols(8), "e128": X.hamming_cols(7),
}
SMALL = (("h7", "e16", 3, 3, 0.8), ("e20", "e100", 2, 3, 0.62), ("e32", "e32", 2, 3, 0.66), ("e64", "e64", 2, 2, 0.6))
PATTERNS = (0, 1, 4, 6)

Case = collections.namedtuple("Case", "name col row p iters w t0 R C sigma clip scale K1 K2 seed")


def _cases():
    out = []
    for ci, (col, row, R, C, sigma) in enumerate(SMALL):
        n1, n2 = len(CODES[col][0]), len(CODES[row][0])
        for pi, p in enumerate(PATTERNS):
            i = 4 * ci + pi
            iters, w, t0 = (1, 2, 4)[(i + ci) % 3], (1, 4, 12)[(i // 2 + pi) % 3], (0, 5)[(i + ci) % 2]
            if col == "e64" and p == 6:
                iters = min(iters, 2)
            small_clip = i % 2 == 1
            scale = (0.7, 9.0, 1.3)[:R] if small_clip else None if i % 4 == 2 else (0.5, 2.0, 1.0)[:R]
            out.append(Case(f"{col}x{row}-p{p}-i{iters}-w{w}-t{t0}-{'clip6' if small_clip else 'clip2^60'}", col, row, p, iters, w, t0, R, C, sigma,
                            6.0 if small_clip else 2.0 ** 60, scale, n1 - CODES[col][1] if i % 3 else n1, n2 - CODES[row][1] if i % 3 else n2,
                            9100 + i))
    return out


CASES = tuple(_cases())
LARGE = (Case("e256xe60-p2-i2-w12-t5-clip6", "e256", "e60", 2, 2, 12, 5, 2, 2, 0.5, 6.0, (0.7, 9.0), 247, 53, 9150),
         Case("e256xe60-p0-i1-w1-t0-clip2^60", "e256", "e60", 0, 1, 1, 0, 1, 2, 0.5, 2.0 ** 60, None, 256, 60, 9151),
         Case("e128xe128-p1-i2-w4-t5-clip2^60", "e128", "e128", 1, 2, 4, 5, 2, 2, 0.45, 2.0 ** 60, (0.5, 2.0), 120, 120, 9152),
         Case("e128xe128-p2-i1-w12-t0-clip6", "e128", "e128", 2, 1, 12, 0, 1, 2, 0.45, 6.0, (9.0,), 128, 128, 9153))
# the grid-stride path: the launch caps the grid at 1024 workgroups, so with R C = 1027 blocks of the 7 x 7 product three workgroups decode two
# blocks on the same LDS
STRIDE = Case("h7xh7-stride", "h7", "h7", 1, 2, 4, 5, 1, 1027, 0.6, 2.0 ** 60, (1.0,), 4, 4, 9160)
# model (2) follows these: both component codes have n' <= 16
TINY = tuple(c for c in CASES if c.col == "h7") + (Case("e16xh7-p3-i3-w4-t5-clip6", "e16", "h7", 3, 3, 4, 5, 3, 3, 0.8, 6.0, (0.7, 9.0, 1.3), 11, 4, 9170),)
# the fixed-seed turbo-gain statement of tests/test_ref_tpc_host.py: six blocks of the extended (32, 26)^2 code, BPSK + AWGN at sigma = 0.66
AWGN = Case("e32xe32-awgn", "e32", "e32", 4, 4, 1, 0, 1, 6, 0.66, 2.0 ** 60, None, 26, 26, 7)


def cols(case):
    return CODES[case.col][0], CODES[case.row][0]


def schedules(case):
    return T.schedule(T.ALPHA, case.iters), T.schedule(T.BETA, case.iters)


def scale_of(case, llr, plain=False):
    """The case's scale[R] float32; the AWGN statement runs with engine.tpc_decode's default, the float32 mean of |llr| over the run's tensor."""
    if plain:
        return np.abs(llr).reshape(llr.shape[0], -1).mean(1, dtype=F)
    return None if case.scale is None else np.array(case.scale, F)


@functools.lru_cache(maxsize=None)
def tensors(case, plain=False):
    """-> (llr[R, w, N] float32, bits[R, w, N] int8); plain: the AWGN LLRs alone, nothing rounded, planted or made loud."""
    n = len(CODES[case.col][0]) * len(CODES[case.row][0])
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
            bits[r, plane[c, pos[3]], sym[c, pos[3]]] = 1      # an error of infinite reliability, which the clip makes finite
    used = np.zeros((w, N), bool)
    used[plane, sym] = True
    llr[:, ~used] = np.where(bits[:, ~used] == 1, LOUD, -LOUD)
    return llr, bits


@functools.lru_cache(maxsize=None)
def expected(case, plain=False):
    """-> (out[R, C, 8], stream llr[R, C n], stream bits[R, C n], ext[R, C, n], half_err[R, C, 2 iters], the Counter) of model (1)."""
    llr, bits = tensors(case, plain)
    alpha, beta = schedules(case)
    return T.decode(llr, bits, *cols(case), case.p, case.iters, alpha, beta, scale_of(case, llr, plain), F(case.clip), case.K1, case.K2, case.t0,
                    case.C)

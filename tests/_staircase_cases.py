"""The cases tests/test_staircase_gpu.py decodes and tests/test_ref_staircase_host.py counts the branches of, built and decoded by the model
(tests/_ref_staircase.py) once per process.

Seven component codes (m, t, s), the smallest at which something distinct can go wrong; for each, five (L, W, iters) and three error rates, 0.3, 1
and 2 times t / (2 s): R = 3 runs of C = 2 chains, w and t0 walking through {12, 8, 6} x {0, 11} over the fifteen cases of a shape, so chains
start inside a symbol.  Every bit outside the chains is loud and wrong; one NaN, one +0 and one -0 lie among the LLRs of each run's chains.
No pattern is planted: these seeds reach every branch named below in every shape (a miscorrection leaves a codeword behind, so the next visit
of that component is an undetected error even where a random pattern with zero syndromes has a chance of 2^-24)."""
import collections
import functools

import numpy as np

import _ref_staircase as S

SHAPES = ((4, 1, 7), (4, 2, 7), (5, 2, 15), (6, 3, 31), (7, 2, 33), (8, 3, 127), (9, 2, 128))
LARGE = ((8, 3, 127), (9, 2, 128))
LWI = ((1, 1, 4), (3, 5, 4), (5, 2, 1), (6, 3, 6), (4, 4, 3))  # one pair; one position; a window of two and one iteration; the cap; L = W
RATES = (0.3, 1.0, 2.0)
R_, C_ = 3, 2
WS, T0S = (12, 8, 6), (0, 11)
EVERY = ("status0", "status1", "status2", "miscorrected", "undetected", "shortened-root", "block0-root", "bad_flips", "pos-noflip", "pos-cap")
BUT_PERFECT = ("roots<L", "L>t")                           # a perfect code has a set of at most t positions for every syndrome


def lwi_of(shape, a):
    L, W, iters = LWI[a]
    return (min(L, 3) if shape in LARGE else L), W, iters


def make(seed, m, t, s, L, rate, w, t0):
    """-> llr[R, w, N] float32, bits[R, w, N] int8 with N = t0 + ceil(C n / w) + 3."""
    rng = np.random.default_rng(seed)
    n = L * s * s
    N = t0 + -(-C_ * n // w) + 3
    bits = rng.integers(0, 2, (R_, w, N)).astype(np.int8)
    mag = (0.5 + 4.0 * rng.random((R_, w, N))).astype(np.float32)
    g = np.arange(N * w).reshape(N, w).T - t0 * w              # [w, N]: the global bit of (plane, symbol), from the first chain's first bit
    inside = (g >= 0) & (g < C_ * n)
    wrong = np.where(inside[None], rng.random((R_, w, N)) < rate * t / (2.0 * s), True)
    rx = bits.astype(bool) ^ wrong
    llr = np.where(rx, -mag, mag).astype(np.float32)
    llr[:, ~inside] *= np.float32(25.0)                         # loud and wrong
    for r in range(R_):
        k = rng.choice(C_ * n, 3, replace=False) + t0 * w
        for kk, v in zip(k, (np.float32("nan"), np.float32(0.0), np.float32(-0.0))):
            llr[r, kk % w, kk // w] = v
    return llr, bits


@functools.lru_cache(maxsize=None)
def case(shape, a, b):
    """-> dict(args of the call, llr, bits, and the model's out, hard, pos_err, pos_iters, count)."""
    m, t, s = shape
    L, W, iters = lwi_of(shape, a)
    w, t0 = WS[(a + b) % 3], T0S[(a + b) % 2]
    llr, bits = make(10000 * SHAPES.index(shape) + 100 * a + b, m, t, s, L, RATES[b], w, t0)
    out, hard, pos_err, pos_iters, count = S.decode(llr, bits, m, t, s, L, W, iters, t0, C_, memo=_memo(shape))
    for x in (llr, bits, out, hard, pos_err, pos_iters):
        x.setflags(write=False)
    return dict(m=m, t=t, s=s, L=L, W=W, iters=iters, w=w, t0=t0, llr=llr, bits=bits, out=out, hard=hard, pos_err=pos_err, pos_iters=pos_iters,
                count=count)


@functools.lru_cache(maxsize=None)
def _memo(shape):
    return {}


@functools.lru_cache(maxsize=None)
def counts(shape):
    """The branches the fifteen cases of a shape take, summed."""
    total = collections.Counter()
    for a in range(len(LWI)):
        for b in range(len(RATES)):
            total.update(case(shape, a, b)["count"])
    return total


def reached(shape):
    """The branches that must have been taken for the device test of this shape to mean something."""
    return EVERY + (() if shape == (4, 1, 7) else BUT_PERFECT)

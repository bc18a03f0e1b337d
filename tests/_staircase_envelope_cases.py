"""The cases of tests/test_staircase_envelope_gpu.py and of the staircase part of tests/test_ref_fec_envelope_host.py: what vaeq_staircase_decode
(include/vaeq.h) accepts and the cases of its feature commit (tests/_staircase_cases.py) leave out, built and decoded by the model
(tests/_ref_staircase.py) once per process.

Where R = 3 runs of C = 2 chains serve, the tensors are _staircase_cases.make's.  frame() restates that recipe for another R and C, for a frame
without a spare symbol and for a given error pattern e[R, C, L, s, s] instead of a rate (no NaN or zero is planted then: the pattern is the point).

GROUPS, by the items of the issue:
  long      (4, 2, 7) L = 40 W = 3 (38 positions: the ring of 4 slots wraps nine times) and (5, 2, 15) L = 20 W = 2 (19 positions, a ring of 3);
  window    W = 32 at (4, 2, 7) with L = 34 (three positions, 33 slots), L = 32 (L = W) and L = 5 (a window longer than the chain: P = 1);
  cap       iters = 100 on (5, 2, 15) L = 8 W = 2 at 1.6 t / (2 s);
  smallest  s = 3 with (4, 1, 3).  s = 2 is accepted by the ranges but parity(m, t) < 2 s = 4 holds for no m >= 4 (parity(m, 1) = m), so
            s = 3 is the smallest block that exists; tests/test_ref_fec_envelope_host.py asserts the refusal of s = 2;
  tables    the exp / log tables are built by blockDim.x threads in chunks of ceil(q / NT): (10, 1, 20) is GF(2^10) on 64 threads, 16 exponents
            each; (9, 3, 255) is 256 threads with two each, rows one bit under 8 words and positions up to 509 = q - 2; (4, 2, 7) for contrast;
  widths    w in {1, 5, 13, 64} on (4, 2, 7) with t0 = 11 and t0 = 0 (at w = 64 a block of 49 bits is part of one symbol), and a frame that fits
            exactly, t0 w + C n_chain = N w;
  grid      C = 300 chains in one run and R = 40 runs of one chain;
  roots     planted patterns, see planted()."""
import collections
import functools

import numpy as np

import _ref_staircase as S
import _staircase_cases as K

Case = collections.namedtuple("Case", "name m t s L W iters w t0 R C rate seed spare")


def _std(name, m, t, s, L, W, iters, w, t0, rate, seed, R=K.R_):
    return Case(name, m, t, s, L, W, iters, w, t0, R, K.C_, rate, seed, 3)


GROUPS = {
    "long": tuple(_std(f"long-{m}-{t}-{s}-L{L}-W{W}-x{rate}", m, t, s, L, W, 4, w, t0, rate, 21000 + 10 * L + i)
                  for (m, t, s, L, W, w, t0) in ((4, 2, 7, 40, 3, 12, 11), (5, 2, 15, 20, 2, 8, 0)) for i, rate in enumerate((1.0, 2.0))),
    "window": tuple(_std(f"W32-L{L}-x{rate}", 4, 2, 7, L, 32, 3, 6, 11, rate, 22000 + 10 * L + i) for L in (34, 32, 5) for i, rate in enumerate((1.0, 2.0))),
    "cap": (_std("cap-100", 5, 2, 15, 8, 2, 100, 8, 0, 1.6, 23003),),
    "smallest": tuple(_std(f"s3-L{L}-W{W}-x{rate}", 4, 1, 3, L, W, 4, w, t0, rate, 24000 + 10 * L + i)
                      for (L, W, w, t0) in ((1, 1, 12, 11), (5, 2, 8, 0), (4, 4, 6, 11)) for i, rate in enumerate((1.0, 2.0))),
    "tables": (_std("gf1024-64-threads", 10, 1, 20, 3, 2, 3, 12, 11, 1.0, 25001), _std("gf1024-64-threads-x2", 10, 1, 20, 3, 2, 3, 8, 0, 2.0, 25002),
               _std("gf512-256-threads", 9, 3, 255, 3, 2, 2, 12, 5, 1.0, 25003, R=1), _std("gf16-64-threads", 4, 2, 7, 3, 2, 3, 12, 11, 1.0, 25004)),
    "widths": tuple(_std(f"w{w}-t{t0}", 4, 2, 7, 3, 2, 3, w, t0, 1.0, 26000 + 2 * w + (t0 > 0)) for w in (1, 5, 13, 64) for t0 in (11, 0))
              + (Case("exact-fit", 4, 2, 7, 4, 2, 3, 8, 5, 3, 2, 1.0, 26900, 0),),
    "grid": (Case("C300", 4, 2, 7, 3, 2, 3, 12, 11, 1, 300, 1.0, 27001, 3), Case("R40", 4, 2, 7, 3, 2, 3, 12, 11, 40, 1, 1.0, 27002, 3)),
}
REACHED = {"long": K.EVERY + K.BUT_PERFECT, "window": K.EVERY + K.BUT_PERFECT}


def frame(seed, s, L, w, t0, R, C, spare, wrong):
    """_staircase_cases.make for any R, C and `spare` symbols behind the chains -> llr[R, w, N] float32, bits[R, w, N] int8.  wrong: the probability
    of a wrong bit inside the chains (then one NaN, one +0 and one -0 lie among each run's chains), or the error pattern e[R, C, L, s, s] itself."""
    rng = np.random.default_rng(seed)
    n = L * s * s
    N = t0 + -(-C * n // w) + spare
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    mag = (0.5 + 4.0 * rng.random((R, w, N))).astype(np.float32)
    g = np.arange(N * w).reshape(N, w).T - t0 * w              # [w, N]: the global bit of (plane, symbol), from the first chain's first bit
    inside = (g >= 0) & (g < C * n)
    if np.ndim(wrong):
        flat = np.asarray(wrong, bool).reshape(R, C * n)
        err = np.ones((R, w, N), bool)                         # every bit outside the chains is wrong
        err[:, inside] = flat[:, g[inside]]
    else:
        err = np.where(inside[None], rng.random((R, w, N)) < wrong, True)
    llr = np.where(bits.astype(bool) ^ err, -mag, mag).astype(np.float32)
    llr[:, ~inside] *= np.float32(25.0)                         # loud and wrong
    if not np.ndim(wrong):
        for r in range(R):
            k = rng.choice(C * n, 3, replace=False) + t0 * w
            for kk, v in zip(k, (np.float32("nan"), np.float32(0.0), np.float32(-0.0))):
                llr[r, kk % w, kk // w] = v
    return llr, bits


def _decoded(c, llr, bits, memo=None):
    out, hard, pos_err, pos_iters, count = S.decode(llr, bits, c.m, c.t, c.s, c.L, c.W, c.iters, c.t0, c.C, memo=memo)
    for x in (llr, bits, out, hard, pos_err, pos_iters):
        x.setflags(write=False)
    return dict(c._asdict(), llr=llr, bits=bits, out=out, hard=hard, pos_err=pos_err, pos_iters=pos_iters, count=count)


@functools.lru_cache(maxsize=None)
def case(c):
    """-> dict(the fields of the Case, llr, bits, and the model's out, hard, pos_err, pos_iters, count)."""
    if (c.R, c.C, c.spare) in ((K.R_, K.C_, 3), (1, K.C_, 3)):
        llr, bits = K.make(c.seed, c.m, c.t, c.s, c.L, c.rate, c.w, c.t0)
        llr, bits = llr[:c.R].copy(), bits[:c.R].copy()        # (one run of the three where the model is slow)
    else:
        llr, bits = frame(c.seed, c.s, c.L, c.w, c.t0, c.R, c.C, c.spare, c.rate * c.t / (2.0 * c.s))
    return _decoded(c, llr, bits)


def counts(group):
    total = collections.Counter()
    for c in GROUPS[group]:
        total.update(case(c)["count"])
    return total


# ---- planted patterns: the root list of one component, packed ten bits a root, six to the first 64-bit word and two to the second ----
PLANTED = ((7, 8, 40, (5, 6, 7, 8, 9)), (7, 7, 40, (6, 7, 8)), (10, 8, 60, (5, 6, 7, 8, 9)), (10, 7, 60, (6, 7, 8)))   # (m, t, s, the k's; the last is t + 1)
SHIELDED = 3                                                   # the errors of a mixed pattern that lie in the previous block


def pattern(t, s, k, mixed, rng):
    """e[L, s, s] with one component of k errors.  Not mixed: L = 1, all k in row j of block 1 (positions s .. 2 s - 1 of component j of pair 1).
    Mixed: L = 2, SHIELDED of the k in column j of block 1 and the rest in row j of block 2, component j of pair 2.  Pair 1 is decoded before
    pair 2 and would take the errors of block 1 away one by one, so each of their rows carries t more errors in columns of its own: t + 1
    errors, which pair 1 leaves alone (status 2), and which pair 2 then corrects, one per component, in the same step as the planted component.
    -> (e, j)"""
    j = int(rng.integers(s))
    others = [c for c in range(s) if c != j]
    if not mixed:
        e = np.zeros((1, s, s), bool)
        e[0, j, rng.choice(s, k, replace=False)] = True
        return e, j
    e = np.zeros((2, s, s), bool)
    rows = rng.choice(s, SHIELDED, replace=False)
    shield = rng.choice(others, (SHIELDED, t), replace=False)
    for a, cols in zip(rows, shield):
        e[0, a, j] = True
        e[0, a, cols] = True
    e[1, j, rng.choice(s, k - SHIELDED, replace=False)] = True
    return e, j


@functools.lru_cache(maxsize=None)
def planted(m, t, s, mixed):
    """One run, one chain per k of PLANTED -> (the case dict, [(k, j, the planted component's positions)], the memo of decided components)."""
    ks = next(p[3] for p in PLANTED if p[:3] == (m, t, s))
    rng = np.random.default_rng(28000 + 100 * m + 10 * t + mixed)
    L = 2 if mixed else 1
    e, info = np.zeros((1, len(ks), L, s, s), bool), []
    for c, k in enumerate(ks):
        e[0, c], j = pattern(t, s, k, mixed, rng)
        word = np.concatenate([e[0, c, 0].T[j], e[0, c, 1][j]]) if mixed else np.concatenate([np.zeros(s, bool), e[0, c, 0][j]])
        info.append((k, j, tuple(int(p) for p in np.nonzero(word)[0])))
    c = Case(f"planted-{m}-{t}-{s}-{'mixed' if mixed else 'row'}", m, t, s, L, L, 3, 12, 5, 1, len(ks), 0.0, 0, 3)
    llr, bits = frame(28500 + 100 * m + 10 * t + mixed, s, L, c.w, c.t0, 1, len(ks), 3, e)
    memo = {}
    return _decoded(c, llr, bits, memo), info, memo

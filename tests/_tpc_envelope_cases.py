"""The cases of tests/test_tpc_envelope_gpu.py and of the TPC part of tests/test_ref_fec_envelope_host.py: what vaeq_tpc_decode (include/vaeq.h)
accepts and the cases of its feature commit (tests/_tpc_cases.py) leave out, with what model (1) of tests/_ref_tpc.py makes of them.

The LLR recipe is _tpc_cases.tensors's, restated over this module's CODES (that one looks its codes up in _tpc_cases.CODES and needs C >= 2):
2 y / sigma^2 of BPSK + AWGN, every third block rounded to integers, block 0 of run 1 noiseless where C >= 2, per run one block with a NaN, a +0,
a -0, a +inf and a -inf, every entry outside the blocks loud and wrong.  A Case adds to _tpc_cases.Case its own schedules (alpha, beta: a
number is that value throughout, None is Pyndiah's), the spare symbols behind the blocks (0: the frame fits exactly) and `plant`: whole
degenerate blocks, see tensors().

GROUPS, by the items of the issue:
  schedule  iters = 16 on e16 x e16 at sigma 0.95 (blocks that run all 32 half-iterations: alpha[32], beta[32], half_err rows of 32) and
            iters = 8 cases with a stop at an even h >= 2;
  rows      long words along the rows: (column x row) 8 x 200, 8 x 256 (four lane slots on the 4-wave instantiation), 4 x 129, 8 x 65, and
            150 x 8, 192 x 8 along the columns;
  smallest  3 x 3 with p = 3 = n and K1 = K2 = 1; 3 x 256 and 256 x 3;
  waves     65 x 64 = 4160 bits, just above the 4-wave boundary of 4096, and 256 x 17: 17 column words for 16 waves;
  columns   both codes 60 seeded distinct ten-bit columns that include 1 and 1023: most syndromes have no position;
  widths    w in {2, 3, 5, 7, 13, 64}; at w = 7 the frame fits exactly, t0 w + C n = N w;
  corners   alpha = 16 and alpha = 0 throughout, beta = 0 throughout, beta = FLT_MAX (the product with the scale overflows to +inf and the
            clip catches it), and scales of 0, a negative number, NaN and +inf per run;
  clips     clip = 2^96 and clip = 2^-20, each with planted blocks of zeros, of infinities and of one magnitude;
  grid      40 runs of one block with a scale of its own per run.
STRIDE is the grid-stride path of the 16-wave instantiation: 1027 blocks of 65 x 64 at w = 1, five distinct blocks repeated."""
import collections
import functools

import numpy as np

import _ref_chase as X
import _ref_tpc as T
import _tpc_cases as K

F = np.float32
FLT_MAX = float(np.finfo(F).max)
Case = collections.namedtuple("Case", "name col row p iters w t0 R C sigma clip scale K1 K2 seed alpha beta spare plant",
                              defaults=(None, None, 3, False))


def _random60(seed):
    rest = np.random.default_rng(seed).choice(np.arange(2, 1023), 58, replace=False)
    return np.random.default_rng(seed + 1).permutation(np.concatenate([[1, 1023], rest])).astype(np.int64), 10


CODES = {"h3": X.hamming_cols(2, False), "e4": X.hamming_cols(2), "e8": X.hamming_cols(3), "h7": X.hamming_cols(3, False), "e16": X.hamming_cols(4),
         "e17": X.hamming_cols(5, n=17), "e64": X.hamming_cols(6), "e256": X.hamming_cols(8), "r60a": _random60(600), "r60b": _random60(610),
         **{f"e{n}": X.hamming_cols(8, n=n) for n in (65, 129, 150, 192, 200)}}
BIG = 2.0 ** 60
ZEROS, INFS, EQUAL = 1, 2, 3                                   # the planted blocks of a run (block 0 stays as the recipe makes it)


def n_of(case):
    return len(CODES[case.col][0]), len(CODES[case.row][0])


def _k(case_code):
    cols, r = CODES[case_code]
    return len(cols) - r


def _c(name, col, row, p, iters, w, t0, R, C, sigma, clip, scale, seed, payload=True, **kw):
    n1, n2 = len(CODES[col][0]), len(CODES[row][0])
    K1, K2 = (max(1, _k(col)), max(1, _k(row))) if payload else (n1, n2)
    return Case(name, col, row, p, iters, w, t0, R, C, sigma, clip, scale, K1, K2, seed, **kw)


NAN, INF = float("nan"), float("inf")
S2, S2C, S3, S3C = (0.5, 2.0), (0.7, 9.0), (0.5, 2.0, 1.0), (0.7, 9.0, 1.3)    # the scales of _tpc_cases: beside the big clip, beside the clip of 6
#                 name, col, row, p, iters, w, t0, R, C, sigma, clip, scale, seed
GROUPS = {
    "schedule": (_c("e16xe16-i16", "e16", "e16", 4, 16, 4, 5, 1, 6, 0.95, BIG, None, 40001),
                 _c("e16xe16-i8", "e16", "e16", 4, 8, 12, 0, 2, 6, 0.9, BIG, (1.0, 2.0), 40002),
                 _c("h7xe16-i8", "h7", "e16", 3, 8, 1, 5, 2, 6, 0.85, 6.0, (0.7, 1.3), 40003)),
    "rows": (_c("e8xe200", "e8", "e200", 4, 2, 12, 5, 2, 2, 0.55, BIG, S2, 40101),
             _c("e8xe256", "e8", "e256", 2, 2, 4, 0, 2, 2, 0.55, 6.0, S2C, 40102),
             _c("e4xe129", "e4", "e129", 4, 2, 1, 5, 2, 2, 0.6, BIG, None, 40103),
             _c("e8xe65", "e8", "e65", 3, 3, 12, 0, 2, 2, 0.6, 6.0, S2C, 40104),
             _c("e150xe8", "e150", "e8", 4, 2, 4, 5, 2, 2, 0.6, BIG, S2, 40105),
             _c("e192xe8", "e192", "e8", 2, 2, 12, 0, 2, 2, 0.6, 6.0, S2C, 40106)),
    "smallest": (_c("h3xh3-p3", "h3", "h3", 3, 2, 4, 5, 3, 3, 0.8, BIG, S3, 40201),
                 _c("h3xh3-p0", "h3", "h3", 0, 2, 12, 0, 3, 3, 0.8, 6.0, S3C, 40202),
                 _c("h3xe256", "h3", "e256", 3, 2, 12, 5, 2, 2, 0.6, BIG, S2, 40203),
                 _c("e256xh3", "e256", "h3", 3, 2, 4, 0, 2, 2, 0.6, 6.0, S2C, 40204)),
    "waves": (_c("e65xe64", "e65", "e64", 2, 2, 12, 5, 2, 2, 0.55, BIG, S2, 40301),
              _c("e256xe17", "e256", "e17", 2, 2, 4, 0, 2, 2, 0.6, 6.0, S2C, 40302),
              _c("e256xe17-p1", "e256", "e17", 1, 1, 1, 5, 1, 2, 0.6, BIG, None, 40303, payload=False)),
    "columns": (_c("r60xr60-p2", "r60a", "r60b", 2, 2, 12, 5, 2, 2, 0.45, BIG, S2, 40401),
                _c("r60xr60-p4", "r60a", "r60b", 4, 2, 4, 0, 2, 2, 0.45, 6.0, S2C, 40402),
                _c("r60xr60-p0", "r60b", "r60a", 0, 1, 1, 5, 2, 2, 0.45, BIG, None, 40403)),
    "widths": tuple(_c(f"h7xe16-w{w}", "h7", "e16", 4, 2, w, (5, 0)[i % 2], 2, 3, 0.8, (BIG, 6.0)[i % 2], (S2, S2C)[i % 2], 40500 + w,
                       spare=0 if w == 7 else 3) for i, w in enumerate((2, 3, 5, 7, 13, 64))),
    "corners": (_c("alpha16", "h7", "e16", 2, 3, 4, 5, 3, 3, 0.8, BIG, S3, 40601, alpha=16.0),
                _c("alpha16-clip6", "e16", "e16", 4, 3, 12, 0, 3, 3, 0.8, 6.0, S3C, 40602, alpha=16.0),
                _c("alpha0", "h7", "e16", 2, 3, 4, 5, 3, 3, 0.8, BIG, S3, 40603, alpha=0.0),
                _c("beta0", "h7", "e16", 2, 3, 4, 5, 3, 3, 0.8, BIG, S3, 40604, beta=0.0),
                _c("betamax", "h7", "e16", 2, 3, 4, 5, 3, 3, 0.8, BIG, S3, 40605, beta=FLT_MAX),
                _c("betamax-clip6", "e16", "h7", 1, 3, 12, 0, 3, 3, 0.8, 6.0, (0.7, 9.0, 1e-38), 40606, beta=FLT_MAX),
                _c("scales", "h7", "e16", 2, 3, 4, 5, 5, 3, 0.8, BIG, (0.0, -1.5, NAN, INF, -0.0), 40607),
                _c("scales-clip6", "e16", "e16", 1, 3, 12, 0, 5, 3, 0.8, 6.0, (INF, NAN, -INF, 0.0, 1e-42), 40608),
                _c("scales-beta0", "h7", "e16", 2, 2, 4, 5, 2, 3, 0.8, BIG, (INF, NAN), 40609, beta=0.0)),
    "clips": tuple(_c(f"{col}x{row}-clip{name}", col, row, p, 3, w, t0, 2, 4, 0.8, clip, S2C, 40700 + i, plant=True) for i, (col, row, p, w, t0, clip, name)
                   in enumerate((("h7", "e16", 4, 4, 5, 2.0 ** 96, "2^96"), ("e16", "e16", 2, 12, 0, 2.0 ** 96, "2^96"), ("h7", "e16", 4, 4, 5, 2.0 ** -20, "2^-20"),
                                 ("e16", "e16", 2, 12, 0, 2.0 ** -20, "2^-20"), ("e16", "h7", 3, 1, 5, 6.0, "6")))),
    "grid": (_c("h7xe16-R40-C1", "h7", "e16", 3, 2, 4, 5, 40, 1, 0.8, BIG, tuple(0.25 * (r + 1) for r in range(40)), 40801),),
}
STRIDE = _c("e65xe64-stride", "e65", "e64", 1, 1, 1, 0, 1, 5, 0.55, BIG, (1.0,), 40901, spare=0)
STRIDE_BLOCKS = 1027                                           # the launch caps the grid at 1024 workgroups: three decode two blocks on one LDS


def cols(case):
    return CODES[case.col][0], CODES[case.row][0]


def schedules(case):
    """-> (alpha[2 iters], beta[2 iters]) float32."""
    one = lambda v, default: T.schedule(default, case.iters) if v is None else np.full(2 * case.iters, v, F)
    return one(case.alpha, T.ALPHA), one(case.beta, T.BETA)


def scale_of(case):
    return None if case.scale is None else np.array(case.scale, F)


@functools.lru_cache(maxsize=None)
def tensors(case):
    """-> (llr[R, w, N] float32, bits[R, w, N] int8).  plant: instead of the five special values, block ZEROS of every run holds only +0 and -0,
    block INFS only +-inf and block EQUAL one magnitude, with one and five scattered wrong bits and a rectangle of four."""
    n1, n2 = n_of(case)
    n = n1 * n2
    rng = np.random.default_rng(case.seed)
    R, C, w = case.R, case.C, case.w
    N = case.t0 + -(-C * n // w) + case.spare
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    llr = (2.0 * ((1.0 - 2.0 * bits) + case.sigma * rng.standard_normal((R, w, N))) / case.sigma ** 2).astype(F)
    g = np.arange(C * n).reshape(C, n)
    sym, plane = case.t0 + g // w, g % w
    for r in range(R):
        for c in range(C):
            if (r * C + c) % 3 == 1:
                llr[r, plane[c], sym[c]] = np.rint(llr[r, plane[c], sym[c]])
        if r == 1 and C > 1:
            llr[r, plane[0], sym[0]] = (2.0 * (1.0 - 2.0 * bits[r, plane[0], sym[0]]) / case.sigma ** 2).astype(F)
        if case.plant:
            tx = lambda c: bits[r, plane[c], sym[c]].astype(bool)

            def wrong(k):                                      # k scattered wrong bits and a rectangle of four: two rows and two columns with two each
                e = np.isin(np.arange(n), rng.choice(n, k, replace=False)).reshape(n1, n2)
                e[np.ix_(rng.choice(n1, 2, replace=False), rng.choice(n2, 2, replace=False))] ^= True
                return e.ravel()

            llr[r, plane[ZEROS], sym[ZEROS]] = np.array([0.0, -0.0], F)[rng.integers(0, 2, n)]
            llr[r, plane[INFS], sym[INFS]] = np.where(tx(INFS) ^ wrong(1), -np.inf, np.inf).astype(F)
            llr[r, plane[EQUAL], sym[EQUAL]] = np.where(tx(EQUAL) ^ wrong(5), F(-2.5), F(2.5))
        elif n >= 5:
            c = 1 + r % (C - 1) if C > 1 else 0                # never block 0 of a run of several, which is run 1's noiseless one
            pos = rng.choice(n, 5, replace=False)
            llr[r, plane[c, pos], sym[c, pos]] = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], F)
            if r == 0:
                bits[r, plane[c, pos[3]], sym[c, pos[3]]] = 1
    used = np.zeros((w, N), bool)
    used[plane, sym] = True
    llr[:, ~used] = np.where(bits[:, ~used] == 1, K.LOUD, -K.LOUD)
    llr.setflags(write=False)
    bits.setflags(write=False)
    return llr, bits


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (out[R, C, 8], stream llr[R, C n], stream bits[R, C n], ext[R, C, n], half_err[R, C, 2 iters], the Counter) of model (1)."""
    llr, bits = tensors(case)
    alpha, beta = schedules(case)
    with np.errstate(over="ignore", invalid="ignore"):         # beta_h scale may overflow to +inf or be 0 inf = NaN: the rule says what follows
        return T.decode(llr, bits, *cols(case), case.p, case.iters, alpha, beta, scale_of(case), F(case.clip), case.K1, case.K2, case.t0, case.C)


@functools.lru_cache(maxsize=None)
def stride():
    """-> (llr[1, 1, 1027 n], bits, and the model's expectation, decoded for the five distinct blocks and repeated)."""
    llr, bits = tensors(STRIDE)
    n1, n2 = n_of(STRIDE)
    n, reps = n1 * n2, -(-STRIDE_BLOCKS // STRIDE.C)
    assert llr.shape == (1, 1, STRIDE.C * n)
    out, s_llr, s_bits, ext, half, count = expected(STRIDE)
    big = lambda x, per: np.ascontiguousarray(np.concatenate([x] * reps, axis=-1)[..., :STRIDE_BLOCKS * per])
    blocks = lambda x: np.concatenate([x] * reps, axis=1)[:, :STRIDE_BLOCKS]
    return big(llr, n), big(bits, n), (blocks(out), big(s_llr, n), big(s_bits, n), blocks(ext), blocks(half), count)

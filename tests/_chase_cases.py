"""The cases of tests/test_ref_chase_host.py and tests/test_chase_gpu.py, built once: device-layout tensors with everything the specification of
vaeq_chase_decode (include/vaeq.h) distinguishes, and what tests/_ref_chase.py makes of them.

The codes: the perfect (7, 4) Hamming code (r = 3: every syndrome is a column, so no pattern is ever without a candidate and status 2 never
occurs -- PERFECT says so and the host test asserts it), (15, 11) (perfect too), the extended (16, 11) code, the extended code of r = 6 shortened
to 20, of r = 8 shortened to 100 (a ragged second slot of 64 lanes) and whole (128, 120), the extended (256, 247) code of r = 9, and 200 seeded
distinct columns of 10 bits.  Every code meets patterns 0, 1, 3 and 6; w in {1, 4, 12} (codewords start inside a symbol wherever n % w != 0),
depth in {0, 2 (a ragged last group of the C = 7 codewords), C}, K < n and K = n, both spreads, t0 in {0, 5} and sigma in {0.45, 0.6} rotate over
the 32 cases so that every (w, depth) pair and every (K, spread) pair occurs.  R = 3, C = 7.

The LLRs: 2 y / sigma^2 of BPSK + AWGN in float32; every third codeword rounded to integers, so that equal |llr| (ties among the least reliable
positions) and equal metrics (ties between candidates) are the common case there; per run one codeword with a NaN, a +0, a -0, a +inf and a -inf
at seeded positions, the +inf against a TX bit 1 in run 0 (an error of infinite reliability: a candidate of infinite metric); every entry outside
the codewords -- in front of t0, behind the last codeword, the unused planes of the interleaver -- loud and wrong.
"""
import collections
import functools

import numpy as np

import _ref_chase as X
import _ref_ldpc_il as IL

F = np.float32
R_, C_ = 3, 7
LOUD = F(50.0)
COUNTERS = ("status0", "status1", "status2", "no-candidate", "v-cancelled", "winner-T>0", "metric-tie", "reliability-tie", "miscorrected",
            "undetected", "inf-metric")

CODES = {
    "h7": X.hamming_cols(3, False), "h15": X.hamming_cols(4, False), "e16": X.hamming_cols(4), "e20": X.hamming_cols(5, n=20),
    "e100": X.hamming_cols(7, n=100), "e128": X.hamming_cols(7), "e256": X.hamming_cols(8),
    "r200": (np.random.default_rng(200).choice(np.arange(1, 1024), 200, replace=False).astype(np.int64), 10),
}
PERFECT = ("h7", "h15")                                        # n = 2^r - 1: status 2 and a pattern without a candidate never occur
PATTERNS = (0, 1, 3, 6)

Case = collections.namedtuple("Case", "name code p w t0 depth K spread sigma R C seed")


def _cases():
    out = []
    for ci, code in enumerate(CODES):
        n, r = len(CODES[code][0]), CODES[code][1]
        for pi, p in enumerate(PATTERNS):
            i = 4 * ci + pi
            w, depth = (1, 4, 12)[i % 3], (0, 2, C_)[(i // 3) % 3]
            full, spread = (i + i // 8) % 2, (i // 2) % 2
            out.append(Case(f"{code}-p{p}-w{w}-d{depth}-{'Kn' if full else 'K'}-s{spread}", code, p, w, (0, 5)[(i + ci) % 2], depth,
                            n if full else n - r, spread, (0.45, 0.6)[(i // 4 + pi) % 2], R_, C_, 9000 + i))
    return out


CASES = _cases()
# the grid-stride path: a workgroup decodes tiles of 8 codewords (at n = 256) of one run and the launch caps the grid at 2048 workgroups, so with
# R ceil(C / 8) = 2253 tiles some workgroups decode two tiles on the same LDS, and the last tile of every run is ragged (3 codewords)
STRIDE = Case("e256-stride", "e256", 1, 4, 0, 0, 247, 1, 0.6, 3, 6003, 9900)
# more codewords than a tile holds (32, or 8 at n = 256): tiles that cut through the interleaver's groups of 5 with a ragged last group of one
# codeword and a ragged last tile of 7, and the bit-packed map with a tile boundary inside a symbol
TILES = (Case("e20-tiles-d5", "e20", 3, 12, 5, 5, 14, 0, 0.45, 2, 71, 9902), Case("e256-tiles", "e256", 3, 12, 0, 0, 247, 1, 0.45, 2, 37, 9903))
# the fixed-seed AWGN statement of tests/test_ref_chase_host.py: 300 words of the extended (128, 120) code near a word BER of 1.3e-2
AWGN = Case("e128-awgn", "e128", 6, 1, 0, 0, 120, 0, 0.45, 1, 300, 9901)


def bit_map(case, n):
    """-> (sym[C, n], plane[C, n]): where bit j of codeword c lies in a run's [w, N] tensors."""
    if case.depth:
        return IL.il_map(case.t0, case.C, n, case.w, case.depth)
    g = np.arange(case.C * n).reshape(case.C, n)
    return case.t0 + g // case.w, g % case.w


@functools.lru_cache(maxsize=None)
def tensors(case, plain=False):
    """-> (llr[R, w, N] float32, bits[R, w, N] int8); plain: the AWGN LLRs alone, nothing rounded, planted or made loud."""
    n = len(CODES[case.code][0])
    rng = np.random.default_rng(case.seed)
    R, C, w = case.R, case.C, case.w
    N = case.t0 + C * IL.symbols_per_codeword(n, w) if case.depth else case.t0 + -(-C * n // w) + 3
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    llr = (2.0 * ((1.0 - 2.0 * bits) + case.sigma * rng.standard_normal((R, w, N))) / case.sigma ** 2).astype(F)
    if plain:
        return llr, bits
    sym, plane = bit_map(case, n)
    for r in range(R):
        for c in range(C):
            if (r * C + c) % 3 == 1:
                llr[r, plane[c], sym[c]] = np.rint(llr[r, plane[c], sym[c]])
        c = (r + 1) % C
        pos = rng.choice(n, 5, replace=False)
        llr[r, plane[c, pos], sym[c, pos]] = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], F)
        if r == 0:
            bits[r, plane[c, pos[3]], sym[c, pos[3]]] = 1
    used = np.zeros((w, N), bool)
    used[plane, sym] = True
    llr[:, ~used] = np.where(bits[:, ~used] == 1, LOUD, -LOUD)
    return llr, bits


@functools.lru_cache(maxsize=None)
def expected(case, plain=False, p=None):
    """-> (out[R, C, 6], stream llr[R, C K], stream bits[R, C K], the Counter) of the model; p: other than the case's."""
    llr, bits = tensors(case, plain)
    return X.decode(llr, bits, CODES[case.code][0], case.p if p is None else p, case.K, case.t0, case.C, case.depth, case.spread)

"""The cases of tests/test_chase_envelope_gpu.py and of the Chase part of tests/test_ref_fec_envelope_host.py: what vaeq_chase_decode
(include/vaeq.h) accepts and the cases of its feature commit (tests/_chase_cases.py) leave out, with what tests/_ref_chase.py makes of them.

The Case tuple, the bit map and the LLR recipe are _chase_cases's.  Its tensors() looks the code up in _chase_cases.CODES, whose exact content
tests/test_ref_chase_host.py asserts, so the recipe is restated here over this module's CODES; it also takes a run of one codeword and a code of fewer
than five bits (which gets no planted NaN, zeros and infinities), and plants whole codewords where `degenerate` is set.

GROUPS, by the items of the issue:
  smallest  n = 3, r = 2 (the perfect code of columns 1, 2, 3) with p = 0 and p = 3 = n, K = 1 and K = 3, at w = 64 with 21 codewords inside one
            symbol; n = 4, r = 3 with p = 0 and p = 4 = n;
  slots     n in {64, 65, 129, 192, 193, 255} of the extended code of r = 9 (one lane slot exactly, one bit into the second, three slots, which
            no feature case has, and one bit under four), p in {2, 4, 5};
  top       r = 10, n = 256: seeded distinct columns that include 1 and 1023, the two ends of the syndrome table;
  tiles     n in {64, 65, 100, 129, 200}, tiles of 32, 31, 20, 15, 10 codewords: two full tiles and a ragged one, contiguous and interleaved at
            depths 3 and 7 (4 and 7 at the tile of 15: none divides its tile), both spreads, K < n;
  widths    w in {2, 3, 5, 7, 13, 64}, the bit-packed map and the interleaver at depth 1 and depth C;
  payload   K = 1 and K = n - 1 under both spreads;
  grid      40 runs of one codeword; one run of one codeword of 256 bits (a tile of one word);
  degenerate  whole codewords planted, see DEGENERATE."""
import functools

import numpy as np

import _chase_cases as K
import _ref_chase as X
import _ref_ldpc_il as IL

F = np.float32
Case = K.Case


def _top():
    rest = np.random.default_rng(1023).choice(np.arange(2, 1023), 254, replace=False)
    return np.random.default_rng(1024).permutation(np.concatenate([[1, 1023], rest])).astype(np.int64), 10


CODES = {"h3": X.hamming_cols(2, False), "e4": X.hamming_cols(2), "e20": X.hamming_cols(5, n=20), "e100": X.hamming_cols(7, n=100),
         "e256": X.hamming_cols(8), "r256": _top(), **{f"e{n}": X.hamming_cols(8, n=n) for n in (64, 65, 129, 192, 193, 200, 255)}}
TILE_WORDS = {64: 32, 65: 31, 100: 20, 129: 15, 200: 10}       # chase_tile_words(n) = min(32, 2048 // n)
TILE_C = {64: 79, 65: 76, 100: 50, 129: 37, 200: 25}           # two full tiles and a ragged one; no depth used divides C either


def n_of(case):
    return len(CODES[case.code][0])


def _tiles():
    out = []
    for i, (n, tw) in enumerate(TILE_WORDS.items()):
        C = TILE_C[n]
        for v, (depth, spread) in enumerate(((0, 0), (4 if tw % 3 == 0 else 3, 1), (7, 0), (0, 1))):
            out.append(Case(f"e{n}-tiles-C{C}-d{depth}-s{spread}", f"e{n}", 2, (12, 5)[v % 2], (5, 0)[(i + v) % 2], depth, n - 9, spread, 0.5, 1, C,
                            31000 + 10 * i + v))
    return tuple(out)


GROUPS = {
    "smallest": (Case("h3-p0-K1-w64", "h3", 0, 64, 0, 0, 1, 1, 0.8, 2, 21, 30001), Case("h3-p3-K3-w64", "h3", 3, 64, 5, 0, 3, 0, 0.8, 2, 21, 30002),
                 Case("h3-p3-K1-w4-d2", "h3", 3, 4, 5, 2, 1, 0, 0.8, 3, 7, 30003), Case("h3-p0-K3-w1", "h3", 0, 1, 0, 0, 3, 1, 0.8, 3, 7, 30004),
                 Case("e4-p0-K1-w64", "e4", 0, 64, 5, 0, 1, 1, 0.8, 2, 16, 30005), Case("e4-p4-K3-w12-d7", "e4", 4, 12, 0, 7, 3, 0, 0.8, 3, 7, 30006)),
    "slots": tuple(Case(f"e{n}-p{p}-w{w}-d{depth}", f"e{n}", p, w, t0, depth, n - 9 if i % 2 else n, i % 2, (0.45, 0.6)[i % 2], 3, 7, 30100 + i)
                   for i, (n, p, w, depth, t0) in enumerate(((64, 2, 1, 0, 5), (65, 4, 12, 2, 0), (129, 5, 4, 0, 5), (192, 2, 12, 7, 0),
                                                            (193, 4, 1, 2, 5), (255, 5, 12, 0, 0), (129, 2, 4, 7, 0), (193, 5, 12, 0, 5)))),
    "top": (Case("r256-p4-w12", "r256", 4, 12, 5, 0, 246, 1, 0.5, 3, 7, 30201), Case("r256-p0-w4-d2", "r256", 0, 4, 0, 2, 256, 0, 0.5, 3, 7, 30202)),
    "tiles": _tiles(),
    "widths": tuple(Case(f"e20-w{w}-d{depth}", "e20", 3, w, (5, 0)[(i + j) % 2], depth, 14, (i + j) % 2, 0.6, 2, 7, 30300 + 10 * i + j)
                    for i, w in enumerate((2, 3, 5, 7, 13, 64)) for j, depth in enumerate((0, 1, 7))),
    "payload": tuple(Case(f"e65-K{Kp}-s{spread}", "e65", 3, 12, 5, (0, 2)[spread], Kp, spread, 0.5, 2, 7, 30400 + Kp + spread)
                     for Kp in (1, 64) for spread in (0, 1)),
    "grid": (Case("e20-R40-C1", "e20", 3, 4, 5, 0, 14, 1, 0.6, 40, 1, 30501), Case("e256-R1-C1", "e256", 3, 12, 0, 0, 247, 0, 0.5, 1, 1, 30502),
             Case("e20-R40-C1-d1", "e20", 3, 4, 0, 1, 14, 0, 0.6, 40, 1, 30503)),
}
# whole codewords planted: codeword 0 of every run holds only +0, -0 and NaN (every key ties, the order falls to the position; erased = n);
# codeword 1 only +-inf with two wrong bits (every metric is 0 or inf: candidates tie at infinity); codeword 2 one non-zero |llr| everywhere,
# with one, two or three wrong bits by the run
DEGENERATE = tuple(Case(f"{code}-p{p}-d{depth}-degenerate", code, p, 12, 5, depth, max(1, n - 6), 1, 0.6, 2, 5, 30600 + i) for i, (code, n, p, depth)
                   in enumerate((("e20", 20, 4, 0), ("e20", 20, 6, 2), ("e129", 129, 6, 0), ("e129", 129, 3, 5), ("h3", 3, 3, 0))))
ZEROS, INFS, EQUAL = 0, 1, 2


@functools.lru_cache(maxsize=None)
def tensors(case, degenerate=False):
    """_chase_cases.tensors over this module's codes -> (llr[R, w, N] float32, bits[R, w, N] int8)."""
    n = n_of(case)
    rng = np.random.default_rng(case.seed)
    R, C, w = case.R, case.C, case.w
    N = case.t0 + C * IL.symbols_per_codeword(n, w) if case.depth else case.t0 + -(-C * n // w) + 3
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    llr = (2.0 * ((1.0 - 2.0 * bits) + case.sigma * rng.standard_normal((R, w, N))) / case.sigma ** 2).astype(F)
    sym, plane = K.bit_map(case, n)
    for r in range(R):
        for c in range(C):
            if (r * C + c) % 3 == 1:
                llr[r, plane[c], sym[c]] = np.rint(llr[r, plane[c], sym[c]])
        if degenerate:
            llr[r, plane[ZEROS], sym[ZEROS]] = np.array([0.0, -0.0, np.nan], F)[rng.integers(0, 3, n)]
            wrong = np.zeros(n, bool)
            wrong[rng.choice(n, 2, replace=False)] = True
            llr[r, plane[INFS], sym[INFS]] = np.where(bits[r, plane[INFS], sym[INFS]].astype(bool) ^ wrong, -np.inf, np.inf).astype(F)
            wrong = np.zeros(n, bool)
            wrong[rng.choice(n, 1 + r % 3, replace=False)] = True
            llr[r, plane[EQUAL], sym[EQUAL]] = np.where(bits[r, plane[EQUAL], sym[EQUAL]].astype(bool) ^ wrong, F(-2.5), F(2.5))
        elif n >= 5:
            c = (r + 1) % C
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
def expected(case, degenerate=False):
    """-> (out[R, C, 6], stream llr[R, C K], stream bits[R, C K], the Counter) of the model."""
    llr, bits = tensors(case, degenerate)
    return X.decode(llr, bits, CODES[case.code][0], case.p, case.K, case.t0, case.C, case.depth, case.spread)

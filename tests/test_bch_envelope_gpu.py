"""vaeq_bch_outer over its whole envelope against the integer model tests/_ref_bch.py: every field m = 4 .. 13, a ladder of t, three shortenings,
and the grid-stride loop in which a wave decodes one codeword after another on the same LDS scratch and registers.

No tolerance: out[R, C_o, 4], loc[R, C_o, t] and the derived figures are asserted with np.array_equal against _ref_bch.outer, as in
tests/test_bch_gpu.py (whose helpers, tests/_bch_cases.py, plant the patterns through the stream map and the TX-bit map).  Every test prints its
figures before it asserts, and every condition on the model is asserted before the first GPU call; the conditions alone are also tests without
the gpu mark, so that a host without a device checks them with the same seeds.

Codes: per m, t in {1, 2, t_max // 2, t_max} with t_max the largest t <= 16 that leaves parity(m, t) < 2^m - 1 (7 at m = 4 and 15 at m = 5, the
repetition codes; 16 from m = 6 on), and per (m, t) the lengths 2^m - 1, parity + 1 (k = 1: nearly every locator root falls on a shortened
position) and one length between them that is no multiple of 64 and, where 2^m - 1 > 256, whose count of 64-lane iterations is no multiple of 4,
so that the four-deep unrolled walk ends in clamped iterations.  m = 9 .. 12 build the tables with 2, 4, 8 and 16 exponents per thread, the last
thread's chunk across e == q.
Geometry per code: C in {5, 3, 4} LDPC codewords of n <= 8200 bits with a payload K < n, C_o in {7, 5, 3} outer codewords per run with C_o n_o <
C K, so that stream bits are left over; those and every bit past the payload are in error with probability 1/2 and must not count.  The options
rotate over the codes of one m as a half fraction of depth in {None, 2} x spread in {0, 1} x post in {float32, int16} x t0 in {0, 11}.
Patterns per code, one per outer codeword: three seeded random ones of every weight 0 .. 2t + 2; a non-zero codeword of the shortened code; a
single error at p = 0 and one at p = n_o - 1; errors on both sides of the last seam between two 64-lane iterations; t errors inside the last,
ragged iteration; t errors with p = 0 and p = n_o - 1 among them; for a shortened code t + 1 errors in the top 64 positions; weight t + 1 for
what is left of the last run.
Conditions: per m, over its codes together, status 0, 1 and 2, a root count short of L, a root at a shortened position and an undetected error
(the planted codeword) occur; over the file a miscorrection and L > t.  Whatever the model says, a pattern of weight 1 .. t is corrected with loc
its sorted positions, among them the single errors at both ends with [1, 1, 0, 1].

The grid-stride path: the launch caps the grid at WAVES = 8192 waves, so with R C_o > 3 x 8192 codewords, a total that is neither a multiple of
4 nor of 8192, every wave decodes three or four codewords and the last pass leaves a workgroup partly idle.  (a) BchCode(4, 2) on n = 42,
C = 5, K = 42, C_o = 13, R = 1901, spread on, bit-packed, int16; (b) BchCode(8, 4) on n = 744, C = 5, K = 620, four lane iterations per
codeword, R = 2235, spread off, depth 2, float32 -- with C_o = 11 of the 12 codewords that fit, because a C_o of 12 makes every total a multiple
of 4.  Each codeword's weight is drawn uniformly from 0 .. 2t + 2; (b) draws its patterns from a seeded pool of 32 per weight and the model
memoises them.  Conditions over the successive codewords g, g + 8192 of every wave: all nine (status, next status) pairs occur, a corrected
codeword is followed by a corrected one with fewer flips, and a codeword with status 1 or 2 by one without errors -- a stale ballot, a stale
locator coefficient, a counter kept across codewords or a missing wave sync at the loop's end would each show there."""
import collections
import functools
import os
import re
import time

import numpy as np
import pytest

import _ref_bch as B
from _bch_cases import _check, _run, plant_case

WAVES = 8192                                               # BCH_GRID * BCH_WAVES of csrc/vaeq_bch.hip: the most waves a launch starts
FIELDS = tuple(range(4, 14))
PER_M = ("status0", "status1", "status2", "roots<L", "shortened-root", "undetected")
OPTIONS = tuple((depth, spread, i16, (0, 11)[(depth is not None) ^ spread ^ i16])           # a half fraction of the 2^4 product
                for i16 in (0, 1) for spread in (0, 1) for depth in (None, 2))


def ladder(m):
    """-> the values of t for field m, ascending."""
    q = (1 << m) - 1
    t_max = max(t for t in range(1, 17) if B.parity(m, t) < q)
    return sorted({1, 2, t_max // 2, t_max})


def lengths(m, t):
    """-> the values of n_o for (m, t): the full length, the shortest, one between them where there is one."""
    q, lo = (1 << m) - 1, B.parity(m, t) + 1
    between = [x for x in sorted(range(lo + 1, q), key=lambda x: abs(x - (lo + q) // 2)) if x % 64 and (q <= 256 or -(-x // 64) % 4)][:1]
    return list(dict.fromkeys([q, lo] + between))


def patterns(m, t, n_o, rng):
    """-> [(tag, positions ascending)], the planted patterns of one code."""
    q = (1 << m) - 1
    draw = lambda lo, hi, k: sorted((lo + rng.choice(hi - lo, min(k, hi - lo), replace=False)).tolist())  # noqa: E731
    P = [(f"w{wt}", draw(0, n_o, wt)) for wt in range(2 * t + 3) for _ in range(3)]
    P.append(("codeword", B.codeword_of(m, t, n_o)))
    P += [("first", [0]), ("last", [n_o - 1])]
    k = (n_o - 1) // 64                                        # the last k with 64 k < n_o
    if k >= 1:
        P += [("seam", [64 * k - 1, 64 * k])] if t >= 2 else [("seam", [64 * k - 1]), ("seam", [64 * k])]
    P.append(("ragged", draw(64 * k, n_o, t)))
    if t >= 2:
        P.append(("ends", [0] + draw(1, n_o - 1, t - 2) + [n_o - 1]))
    if n_o < q:
        P.append(("top", draw(max(0, n_o - 64), n_o, t + 1)))
    return P


@functools.lru_cache(maxsize=None)
def cases(m):
    """-> the codes of field m, each a dict with its geometry, options, planted patterns, tensors and the model's out, loc and counters."""
    out = []
    for j, (t, n_o) in enumerate((t, n_o) for t in ladder(m) for n_o in lengths(m, t)):
        rng = np.random.default_rng(1000000 * m + 1000 * t + j)
        P = patterns(m, t, n_o, rng)
        assert all(p is not None and all(0 <= x < n_o for x in p) for _, p in P)
        C, C_o = (5, 3, 4)[j % 3], 7 if n_o <= 64 else 5 if n_o <= 1024 else 3
        while len(P) % C_o:
            P.append(("fill", sorted(rng.choice(n_o, t + 1, replace=False).tolist())))
        R, K = len(P) // C_o, -(-(C_o * n_o + 4) // C)
        n, w = K + 1 + j % 5, (12, 8)[(j >> 1) & 1]
        depth, spread, i16, t0 = OPTIONS[j % len(OPTIONS)]
        assert C_o * n_o < C * K and K < n <= 64 * 512
        post, bits = plant_case(77000 + 100 * m + j, R, C, n, w, t0, depth, (m, t, n_o), K, spread, C_o, [p for _, p in P], bool(i16), special=not i16)
        t_0 = time.perf_counter()
        want_out, want_loc, count = B.outer(post, bits, m, t, n_o, C_o, K, spread, t0, depth)
        out.append(dict(code=(m, t, n_o), R=R, C=C, n=n, K=K, C_o=C_o, w=w, t0=t0, depth=depth, spread=spread, i16=i16, P=P, post=post, bits=bits,
                        want_out=want_out.reshape(-1, 4), want_loc=want_loc.reshape(-1, t), count=count, model_s=time.perf_counter() - t_0))
    return out


def conditions(m):
    """The conditions of field m on the model alone; -> its cases."""
    cs = cases(m)
    total = collections.Counter()
    for c in cs:
        total.update(c["count"])
        (_, t, n_o), out, loc = c["code"], c["want_out"], c["want_loc"]
        print(f"code={c['code']} R={c['R']} C={c['C']} n={c['n']} K={c['K']} C_o={c['C_o']} w={c['w']} t0={c['t0']} depth={c['depth']} spread={c['spread']} "
              f"int16={c['i16']}: {len(c['P'])} patterns, model {c['model_s']:.2f} s, {dict(c['count'])}")
        for g, (tag, pos) in enumerate(c["P"]):             # what the deterministic patterns must give, whatever the model says
            if len(pos) <= t:
                assert out[g].tolist() == [int(len(pos) > 0), len(pos), 0, len(pos)], (c["code"], tag, pos, out[g])
                assert loc[g].tolist() == pos + [-1] * (t - len(pos)), (c["code"], tag, pos, loc[g])
            if tag in ("first", "last"):
                assert out[g].tolist() == [1, 1, 0, 1] and loc[g, 0] == pos[0] == (0 if tag == "first" else n_o - 1)
    print(f"m={m}: t in {ladder(m)}, {len(cs)} codes, {dict(total)}")
    for k in PER_M:
        assert total[k] > 0, (m, k)
    for k, values in enumerate(((None, 2), (0, 1), (0, 1), (0, 11))):
        assert {OPTIONS[j % len(OPTIONS)][k] for j in range(len(cs))} == set(values)      # every value of every option occurs in this field
    assert [c["code"][1:] for c in cs] == [(t, n_o) for t in ladder(m) for n_o in lengths(m, t)]
    return cs


@pytest.mark.parametrize("m", FIELDS)
def test_field_conditions_hold_on_the_model(m):
    conditions(m)


def test_file_conditions_hold_on_the_model():
    total = collections.Counter()
    for m in FIELDS:
        for c in cases(m):
            total.update(c["count"])
    print(dict(total))
    assert total["miscorrected"] > 0 and total["L>t"] > 0
    assert [ladder(m)[-1] for m in FIELDS] == [7, 15] + [16] * 8       # (what the rule comes out as; the tests take it from parity())
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vae_equalizer_amd", "csrc", "vaeq_bch.hip")).read()
    assert int(re.search(r"BCH_GRID = (\d+) / BCH_WAVES;", src).group(1)) == WAVES


@pytest.mark.gpu
@pytest.mark.parametrize("m", FIELDS)
def test_field_against_the_model(m):
    for c in conditions(m):
        r = _run(c["post"], c["bits"], c["code"], c["n"], c["C_o"], t0=c["t0"], depth=c["depth"], payload=c["K"], spread=bool(c["spread"]))
        shape = (c["R"], c["C_o"], -1)
        _check(r, c["want_out"].reshape(shape), c["want_loc"].reshape(shape), c["code"][2], f"code={c['code']}")


# ------------------------------------------------------------------ the grid-stride path
STRIDE = dict(a=dict(code=(4, 2, 15), n=42, C=5, K=42, C_o=13, R=1901, w=12, t0=11, depth=None, spread=1, i16=True, pool=None),
              b=dict(code=(8, 4, 255), n=744, C=5, K=620, C_o=11, R=2235, w=12, t0=11, depth=2, spread=0, i16=False, pool=32))


@functools.lru_cache(maxsize=None)
def stride_case(name):
    """-> (the case's dict, post, bits, want_out, want_loc, the model's seconds)."""
    c = STRIDE[name]
    (m, t, n_o), total = c["code"], c["R"] * c["C_o"]
    rng = np.random.default_rng(31000 + ord(name))
    wt = rng.integers(0, 2 * t + 3, total)                  # uniform in 0 .. 2t + 2 per codeword, independent of its place
    if c["pool"]:
        pool = [[sorted(rng.choice(n_o, k, replace=False).tolist()) for _ in range(c["pool"])] for k in range(2 * t + 3)]
        P = [pool[k][i] for k, i in zip(wt.tolist(), rng.integers(0, c["pool"], total).tolist())]
    else:
        P = [sorted(rng.choice(n_o, k, replace=False).tolist()) for k in wt.tolist()]
    post, bits = plant_case(32000 + ord(name), c["R"], c["C"], c["n"], c["w"], c["t0"], c["depth"], c["code"], c["K"], c["spread"], c["C_o"], P, c["i16"])
    t_0 = time.perf_counter()
    want_out, want_loc, count = B.outer(post, bits, m, t, n_o, c["C_o"], c["K"], c["spread"], c["t0"], c["depth"], memo={})
    return c, post, bits, want_out, want_loc, time.perf_counter() - t_0, count


def stride_conditions(name):
    c, post, bits, want_out, want_loc, seconds, count = stride_case(name)
    total, flat = c["R"] * c["C_o"], want_out.reshape(-1, 4)
    print(f"{name}: code={c['code']} R={c['R']} C_o={c['C_o']}: {total} codewords = {total // WAVES} x {WAVES} + {total % WAVES}, model {seconds:.2f} s, {dict(count)}")
    assert total > 3 * WAVES and total % 4 and total % WAVES and c["C_o"] * c["code"][2] < c["C"] * c["K"]
    a, b = flat[:-WAVES], flat[WAVES:]                      # codeword g and the next one of its wave, g + WAVES: every successive pair
    pairs = collections.Counter(zip(a[:, 0].tolist(), b[:, 0].tolist()))
    fewer = int(((a[:, 0] == 1) & (b[:, 0] == 1) & (b[:, 3] < a[:, 3])).sum())
    clean = int(((a[:, 0] >= 1) & (b[:, 1] == 0)).sum())
    print(f"{name}: (status, next status) {sorted(pairs.items())}; corrected then corrected with fewer flips {fewer}; status 1 or 2 then no error {clean}")
    assert set(pairs) == {(x, y) for x in range(3) for y in range(3)}
    assert fewer > 0 and clean > 0
    return c, post, bits, want_out, want_loc


@pytest.mark.parametrize("name", sorted(STRIDE))
def test_stride_conditions_hold_on_the_model(name):
    stride_conditions(name)
    assert {(c["spread"], c["depth"]) for c in STRIDE.values()} == {(1, None), (0, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STRIDE))
def test_several_codewords_per_wave(name):
    c, post, bits, want_out, want_loc = stride_conditions(name)
    t_0 = time.perf_counter()
    r = _run(post, bits, c["code"], c["n"], c["C_o"], t0=c["t0"], depth=c["depth"], payload=c["K"], spread=bool(c["spread"]))
    print(f"{name}: GPU call with its copies {1e3 * (time.perf_counter() - t_0):.1f} ms")
    _check(r, want_out, want_loc, c["code"][2], f"stride {name}")

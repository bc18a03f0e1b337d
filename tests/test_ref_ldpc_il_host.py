"""The interleaver of vaeq_ldpc_decode_il as tests/_ref_ldpc_il.py models it (CPU only): over every case of tests/test_ldpc_il_gpu.py the map
sends the C n codeword bits to distinct (symbol, plane) pairs inside [t0, t0 + C S), and its two degenerate depths are what the header says
they are; the same over the shapes of tests/test_ldpc_envelope_gpu.py (every w, C = 7 at depths 3 and 4, C = 300 at depth 7), whose own
restatement of the permutation is held to the map here.  The decoder behind it is tests/_ref_ldpc.py's, held to its scalar restatement by tests/test_ref_ldpc_host.py."""
import numpy as np
import pytest

import _ref_ldpc as M
import _ref_ldpc_il as IL

SHAPES = sorted({(M.CODES[c][0].shape[1] * M.CODES[c][1], M.C_) for c in M.CODES} | {(5 * 512, 2)})   # (n, C): the codes, the Z = 512 corner
DEPTHS = {5: IL.DEPTHS, 2: (1, 2)}


def _cases():
    for n, C in SHAPES:
        for depth in DEPTHS[C]:
            for t0 in (0, 11):
                for w in (12, 8, 6):
                    yield n, C, depth, t0, w
    # tests/test_ldpc_envelope_gpu.py: every w; ragged groups of more than one codeword (C = 7: 4 + 3 and 3 + 3 + 1); the grid (300 = 42 x 7 + 6)
    for n in (42, 960):
        for depth in IL.DEPTHS:
            for t0 in (0, 11):
                for w in (1, 2, 3, 4, 5, 7, 13, 64):
                    yield n, M.C_, depth, t0, w
    for n, w in ((42, 4), (42, 12), (960, 8), (42, 6), (42, 2)):
        for depth in (3, 4, 7):
            yield n, 7, depth, 11, w
    for depth in (1, 7, 300):
        yield 4, 300, depth, 5, 3
    yield 42, 1, 1, 5, 12


@pytest.mark.parametrize("n,C,depth,t0,w", list(_cases()))
def test_no_overlap_and_containment(n, C, depth, t0, w):
    S = IL.symbols_per_codeword(n, w)
    sym, plane = IL.il_map(t0, C, n, w, depth)
    assert sym.shape == plane.shape == (C, n)
    assert len(set(zip(sym.ravel().tolist(), plane.ravel().tolist()))) == C * n
    assert sym.min() >= t0 and sym.max() < t0 + C * S and plane.min() >= 0 and plane.max() < w
    assert np.array_equal(plane, np.broadcast_to(np.arange(n) % w, (C, n)))
    free = IL.unused(t0, C, n, w, depth)
    assert int(free.sum()) == C * (S * w - n) and not free[:, :t0].any()
    if n % w:                                                   # the planes >= n - (S - 1) w of every codeword's last symbol, and nothing else
        last = sym[:, -1]
        assert free[n - (S - 1) * w:, last].all() and not free[:n - (S - 1) * w, last].any()


@pytest.mark.parametrize("n,C,t0,w", sorted({(n, C, t0, w) for n, C, _, t0, w in _cases()}))
def test_degenerate_depths(n, C, t0, w):
    S = IL.symbols_per_codeword(n, w)
    sym, _ = IL.il_map(t0, C, n, w, C)                          # depth = C: symbol u of codeword c is t0 + u C + c
    u = np.arange(n) // w
    assert np.array_equal(sym, t0 + u[None, :] * C + np.arange(C)[:, None])
    sym1, _ = IL.il_map(t0, C, n, w, 1)                         # depth = 1: symbol-aligned contiguous codewords
    assert np.array_equal(sym1, t0 + np.arange(C)[:, None] * S + u[None, :])
    if n % w == 0:                                              # ... which is the bit-packed contiguous form when codewords fill whole symbols
        rng = np.random.default_rng(n + w + t0)
        x = rng.standard_normal((2, w, t0 + C * S + 3)).astype(np.float32)
        assert np.array_equal(IL.codewords_il(x, t0, C, n, 1), M.codewords(x, t0, C, n))


def test_ragged_last_group():
    sym, _ = IL.il_map(3, 5, 42, 12, 2)                         # S = 4: groups of 2, 2, 1 at bases 3, 11, 19
    assert sym[0, :13].tolist() == [3] * 12 + [5] and sym[1, 0] == 4 and sym[2, 0] == 11 and sym[3, 12] == 14
    assert sym[4].tolist() == sorted(sym[4].tolist()) and sym[4, 0] == 19 and sym[4, -1] == 22


def test_ragged_last_groups_of_more_than_one_codeword():
    sym, _ = IL.il_map(11, 7, 42, 12, 4)                        # S = 4: groups of 4 and 3 at bases 11 and 27
    assert sym[:4, 0].tolist() == [11, 12, 13, 14] and sym[:4, 12].tolist() == [15, 16, 17, 18]
    assert sym[4:, 0].tolist() == [27, 28, 29] and sym[4:, 12].tolist() == [30, 31, 32] and sym[6, -1] == 11 + 7 * 4 - 1
    sym, _ = IL.il_map(11, 7, 42, 12, 3)                        # groups of 3, 3 and 1 at bases 11, 23 and 35
    assert sym[3:6, 0].tolist() == [23, 24, 25] and sym[3:6, 12].tolist() == [26, 27, 28] and sym[6, ::12].tolist() == [35, 36, 37, 38]
    sym, _ = IL.il_map(5, 300, 4, 3, 7)                         # S = 2: 42 groups of 7, then six codewords at base 5 + 294 x 2
    assert sym[294:, 0].tolist() == list(range(593, 599)) and sym[294:, 3].tolist() == list(range(599, 605)) and sym.max() == 5 + 300 * 2 - 1


@pytest.mark.parametrize("w", [6, 2])
@pytest.mark.parametrize("depth", [3, 4, 7])
def test_the_envelope_test_s_own_permutation_is_the_map(w, depth):
    """tests/test_ldpc_envelope_gpu.py permutes the symbols back with a restatement of the header's sentence that does not use il_map: the two
    agree, so that test compares what it says it compares."""
    import _ldpc_cases as K
    t0, C, n = 11, 7, 42
    S = n // w
    x = np.random.default_rng(w + depth).standard_normal((2, w, t0 + C * S)).astype(np.float32)
    y = K.deinterleave(x, t0, C, S, depth)
    assert np.array_equal(IL.codewords_il(x, t0, C, n, depth), M.codewords(y, t0, C, n)) and np.array_equal(y[..., :t0], x[..., :t0])
    assert sorted(y[0, 0].tolist()) == sorted(x[0, 0].tolist()) and (depth == 1 or not np.array_equal(x, y))


def test_make_case_il_is_loud_outside_the_codewords():
    llr, bits = IL.make_case_il(5, 42, 0.5, 3, 5, 12, 11, 2)
    assert llr.shape == (3, 12, 11 + 5 * 4)
    free = IL.unused(11, 5, 42, 12, 2)
    assert free.sum() == 5 * 6 and (bits[:, free] == 0).all()
    assert ((llr[:, free] == IL.LOUD).sum(1) == 29).all() and ((llr[:, free] == 0).sum(1) == 1).all()
    assert (IL.codewords_il(llr, 11, 5, 42, 2) == 0).sum() == 3 * 4    # the erasures inside the codewords

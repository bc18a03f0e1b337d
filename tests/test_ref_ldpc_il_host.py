"""The interleaver of vaeq_ldpc_decode_il as tests/_ref_ldpc_il.py models it (CPU only): over every case of tests/test_ldpc_il_gpu.py the map
sends the C n codeword bits to distinct (symbol, plane) pairs inside [t0, t0 + C S), and its two degenerate depths are what the header says
they are.  The decoder behind it is tests/_ref_ldpc.py's, held to its scalar restatement by tests/test_ref_ldpc_host.py."""
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


def test_make_case_il_is_loud_outside_the_codewords():
    llr, bits = IL.make_case_il(5, 42, 0.5, 3, 5, 12, 11, 2)
    assert llr.shape == (3, 12, 11 + 5 * 4)
    free = IL.unused(11, 5, 42, 12, 2)
    assert free.sum() == 5 * 6 and (bits[:, free] == 0).all()
    assert ((llr[:, free] == IL.LOUD).sum(1) == 29).all() and ((llr[:, free] == 0).sum(1) == 1).all()
    assert (IL.codewords_il(llr, 11, 5, 42, 2) == 0).sum() == 3 * 4    # the erasures inside the codewords

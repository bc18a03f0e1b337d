"""The two models of tests/_ref_ebch.py against each other, the reach of tests/_ebch_cases.py, and the turbo-gain statement -- no device.

Model (1) is the specification of vaeq_chase_bch_decode and vaeq_tpc_bch_decode with tests/_ref_bch.py's locator (Berlekamp-Massey and a root
search); model (2) knows a component code only as the list of its codewords and finds candidates and competitors by search.  They must agree in
every counter of out, every decision, every bit of W and the whole half_err profile on the cases whose component codes have n <= 16.  Then: the
cases together reach every counter of model (1) -- the branches a kernel can get wrong -- and model (1) on plain AWGN shows the gain that
double-error-correcting components were added for."""
import collections

import numpy as np
import pytest

import _ebch_cases as K
import _ref_chase as X
import _ref_ebch as E

F = np.float32


def test_codebooks():
    """The lists model (2) works from: 2^k words, minimum distance 5 inside, 6 with the parity bit."""
    for name, k, d in (("b15", 7, 5), ("x16", 7, 6), ("x10", 1, 6)):
        code = K.CODES[name]
        book = np.array([E._extend(code, w) for w in E.codebook(code.m, code.n_i)])
        weights = book.sum(1)
        assert book.shape == (1 << k, code.n) and code.k == k and weights[weights > 0].min() >= d, name
        assert all(E.is_codeword(code, w) and E.in_book(code, w) for w in book)


@pytest.mark.parametrize("case", K.CHASE_TINY, ids=lambda c: c.name)
def test_chase_models_agree(case):
    llr, bits = K.chase_tensors(case)
    out = K.chase_expected(case)[0]
    code = K.CODES[case.code]
    x, tx = X.gather(llr, case.t0, case.C, code.n, case.depth), X.gather(bits, case.t0, case.C, code.n, case.depth)
    for r in range(case.R):
        for c in range(case.C):
            o1, e1 = E.chase_word(code, case.p, case.K, x[r, c], tx[r, c])
            o2, e2 = E.chase_word2(code, case.p, case.K, x[r, c], tx[r, c])
            assert np.array_equal(o1, out[r, c]) and np.array_equal(o2, o1) and np.array_equal(e1, e2), (r, c, o1, o2)


@pytest.mark.parametrize("case", K.TPC_TINY, ids=lambda c: c.name)
def test_tpc_models_agree(case):
    llr, bits = K.tpc_tensors(case)
    out, s_llr, s_bits, ext, half, _ = K.tpc_expected(case)
    c1, c2 = K.CODES[case.col], K.CODES[case.row]
    n = c1.n * c2.n
    alpha, beta = K.schedules(case)
    scale = K.scale_of(case, llr)
    x, tx = E.M.codewords(llr, case.t0, case.C, n), E.M.codewords(bits, case.t0, case.C, n)
    for r in range(case.R):
        for c in range(case.C):
            o2, h2, d2, W2 = E.block2(c1, c2, x[r, c].reshape(c1.n, c2.n), tx[r, c].reshape(c1.n, c2.n), case.p, case.iters, alpha, beta,
                                      F(1.0) if scale is None else scale[r], case.clip, case.K1, case.K2)
            assert np.array_equal(o2, out[r, c]), (r, c, o2, out[r, c])
            assert np.array_equal(h2, half[r, c])
            assert np.array_equal(W2.ravel().view(np.uint32), ext[r, c].view(np.uint32))      # the floats themselves, the sign of a zero included
            assert np.array_equal(np.where(tx[r, c].astype(bool) ^ d2.ravel(), F(-1.0), F(1.0)), s_llr[r, c * n:(c + 1) * n])


def test_cases_reach_every_branch():
    chase, tpc = collections.Counter(), collections.Counter()
    for case in K.CHASE + (K.CHASE_TILES, K.CHASE_STRIDE):
        chase.update(K.chase_expected(case)[3])
    for case in K.TPC + K.TPC_LARGE + K.TPC_TINY[-1:] + (K.TPC_STRIDE,):
        tpc.update(K.tpc_expected(case)[5])
    print("chase:", dict(chase))
    print("tpc:", dict(tpc))
    assert all(chase[k] > 0 for k in K.WORD_COUNTERS + ("miscorrected", "winner-T>0")), [k for k in K.WORD_COUNTERS if not chase[k]]
    assert all(tpc[k] > 0 for k in K.WORD_COUNTERS + K.TPC_COUNTERS), [k for k in K.WORD_COUNTERS + K.TPC_COUNTERS if not tpc[k]]
    tiny = collections.Counter()                               # what model (2) has followed
    for case in K.TPC_TINY:
        tiny.update(K.tpc_expected(case)[5])
    for case in K.CHASE_TINY:
        tiny.update(K.chase_expected(case)[3])
    assert all(tiny[k] > 0 for k in K.WORD_COUNTERS + K.TPC_COUNTERS), [k for k in K.WORD_COUNTERS + K.TPC_COUNTERS if not tiny[k]]
    for case in K.CHASE:                                       # status 2: from p = 0 and from the shortened codes
        out = K.chase_expected(case)[0]
        assert (out[..., 4] >= 3).any()                        # the NaN and both zeros
        if case.p == 0 and case.code in ("x32", "x64", "x128", "x256"):
            assert (out[..., 0] == 2).any(), case.name
    for case in K.TPC + K.TPC_LARGE:
        out, _, _, ext, half, count = K.tpc_expected(case)
        assert np.isfinite(ext).all() and (np.abs(ext) <= F(case.clip)).all()
        if case.clip < 100:
            assert count["clamp-r"] > 0
        if case.R > 1:
            assert out[1, 0].tolist()[:5] == [1, 1, 0, 0, 0]   # the noiseless block costs one half-iteration
        assert ((half >= 0).sum(-1) == out[..., 0]).all()


def test_turbo_gain():
    """Model (1) on four blocks of the extended (32, 21)^2 code, BPSK + AWGN at sigma = 0.85 (12.5 % of the bits wrong; the extended-Hamming
    statement of tests/test_ref_tpc_host.py stands at sigma = 0.66, 6.5 %), p = 4, iters = 4, Pyndiah's schedules, scale = the mean of |llr|,
    clip 2^60, seed 7.  The model's own figures, errors before -> after each half-iteration:
    125 -> 90, 90, 58, 20, 0;  123 -> 104, 56, 26, 0;  131 -> 136, 94, 62, 24, 0;  132 -> 104, 66, 42, 0.
    Every block starts with a row of seven to nine errors (hard decoding of t = 2 words alone fails) and ends on the transmitted codeword."""
    case = K.AWGN
    out, _, _, _, half, count = K.tpc_expected(case, True)
    llr, bits = K.tpc_tensors(case, True)
    e = ((E.M.codewords(llr, 0, case.C, 1024) < 0) ^ E.M.codewords(bits, 0, case.C, 1024).astype(bool))[0].reshape(case.C, 32, 32)
    print("pre_err", out[0, :, 3].tolist(), "worst row", e.sum(2).max(1).tolist(), "half_err", half[0].tolist(), dict(count))
    assert out.shape == (1, 4, 8) and half.shape == (1, 4, 8)
    assert 0.11 < out[0, :, 3].sum() / (4 * 1024) < 0.14
    for c in range(4):
        assert e[c].sum(1).max() > 2 and e[c].sum(0).max() > 2
        assert out[0, c, 2] == 0 and out[0, c, 1] == 1 and out[0, c, 0] <= 8
    assert out[0, :, 3].tolist() == [125, 123, 131, 132] and half[0, 0].tolist() == [90, 90, 58, 20, 0, -1, -1, -1]
    assert half[0, 2].tolist() == [136, 94, 62, 24, 0, -1, -1, -1]

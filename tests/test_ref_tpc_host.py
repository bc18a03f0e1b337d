"""The two models of tests/_ref_tpc.py against each other, the reach of tests/_tpc_cases.py, and the turbo-gain statement -- no device.

Model (1) is the specification of vaeq_tpc_decode with syndrome tables; model (2) knows a component code only as the list of its codewords and
finds candidates and competitors by brute force.  They must agree in every counter of out, every decision, every bit of W and the whole
half_err profile on the cases whose component codes have n' <= 16.  Then: the cases together reach every counter of model (1) -- the branches a
kernel can get wrong -- and model (1) on plain AWGN shows the gain the rule was written for."""
import collections

import numpy as np
import pytest

import _ref_tpc as T
import _tpc_cases as K

F = np.float32


@pytest.mark.parametrize("case", K.TINY, ids=lambda c: c.name)
def test_models_agree(case):
    llr, bits = K.tensors(case)
    out, s_llr, s_bits, ext, half, _ = K.expected(case)
    (c1, r1), (c2, r2) = K.CODES[case.col], K.CODES[case.row]
    n1, n2 = len(c1), len(c2)
    n = n1 * n2
    alpha, beta = K.schedules(case)
    scale = K.scale_of(case, llr)
    x, tx = T.M.codewords(llr, case.t0, case.C, n), T.M.codewords(bits, case.t0, case.C, n)
    for r in range(case.R):
        for c in range(case.C):
            o2, h2, d2, W2 = T.block2(c1, r1, c2, r2, x[r, c].reshape(n1, n2), tx[r, c].reshape(n1, n2), case.p, case.iters, alpha, beta,
                                      F(1.0) if scale is None else scale[r], case.clip, case.K1, case.K2)
            assert np.array_equal(o2, out[r, c]), (r, c, o2, out[r, c])
            assert np.array_equal(h2, half[r, c])
            assert np.array_equal(W2.ravel().view(np.uint32), ext[r, c].view(np.uint32))      # the floats themselves, the sign of a zero included
            assert np.array_equal(np.where(tx[r, c].astype(bool) ^ d2.ravel(), F(-1.0), F(1.0)), s_llr[r, c * n:(c + 1) * n])
            assert np.array_equal(s_bits[r, c * n:(c + 1) * n], tx[r, c])


def test_cases_reach_every_branch():
    total = collections.Counter()
    for case in K.CASES + K.LARGE + (K.STRIDE,):
        count = K.expected(case)[5]
        total.update(count)
        print(case.name, dict(count))
    print("all:", dict(total))
    assert all(total[k] > 0 for k in K.COUNTERS), [k for k in K.COUNTERS if not total[k]]
    for case in K.CASES + K.LARGE:                             # what the docstring of the cases promises of each
        out, _, _, ext, half, count = K.expected(case)
        assert np.isfinite(ext).all() and (np.abs(ext) <= F(case.clip)).all()
        assert (out[..., 4] >= 3).any()                        # the NaN and both zeros
        if case.clip < 100:
            assert count["clamp-r"] > 0
        if case.R > 1:
            assert out[1, 0].tolist()[:5] == [1, 1, 0, 0, 0]   # the noiseless block costs one half-iteration
        assert ((half >= 0).sum(-1) == out[..., 0]).all()
        assert (half[np.arange(out.shape[0])[:, None], np.arange(out.shape[1])[None, :], out[..., 0] - 1] == out[..., 2]).all()


def test_turbo_gain():
    """Model (1) on six blocks of the extended (32, 26)^2 code, BPSK + AWGN at sigma = 0.66 (about 6.5 % of the bits wrong), p = 4, iters = 4,
    Pyndiah's schedules, scale = the mean of |llr|, clip 2^60, seed 7.  The model's own figures, errors before -> after each half-iteration:
    60 -> 46, 30, 24, 20, 8, 0;  70 -> 62, 44, 24, 12, 0;  73 -> 52, 32, 22, 8, 0;  63 -> 48, 24, 16, 12, 0;  55 -> 36, 30, 20, 12, 0;
    68 -> 62, 48, 30, 24, 12, 0.  Every block ends on a product codeword, the transmitted one."""
    out, _, _, _, half, count = K.expected(K.AWGN, True)
    print("pre_err", out[0, :, 3].tolist(), "half_err", half[0].tolist(), dict(count))
    assert out.shape == (1, 6, 8) and half.shape == (1, 6, 8)
    assert 0.055 < out[0, :, 3].sum() / (6 * 1024) < 0.075
    for c in range(6):
        assert half[0, c, 0] < out[0, c, 3]
        assert out[0, c, 2] == 0 and out[0, c, 1] == 1
    assert out[0, :, 3].tolist() == [60, 70, 73, 63, 55, 68] and half[0, 0].tolist() == [46, 30, 24, 20, 8, 0, -1, -1]

"""The two models of vaeq_staircase_decode (tests/_ref_staircase.py) against each other, and the branches the device test's cases take.  CPU only.

(a), the specification on bitmaps with _ref_bch.decode per component, and (b), syndromes per component updated on every flip and decided by
enumeration (_ref_bch.Table), share no code below the schedule: no locator, no root search and no component bits in (b).  They are held to each
other on the two codes small enough for the table, (m, t, s) = (4, 1, 7) and (4, 2, 7), over all fifteen cases of tests/_staircase_cases.py --
every figure, the final error pattern, pos_err and pos_iters.  For (a) alone, at every shape: the counters that keep tests/test_staircase_gpu.py
from passing vacuously."""
import collections

import numpy as np
import pytest

import _ref_bch as B
import _ref_staircase as S
import _staircase_cases as K

SMALL = ((4, 1, 7), (4, 2, 7))


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_bitmap_model_equals_syndrome_model(shape):
    m, t, s = shape
    table = B.Table(m, t, 2 * s)
    for a in range(len(K.LWI)):
        for b in range(len(K.RATES)):
            c = K.case(shape, a, b)
            e, tx, _ = S.errors(c["llr"], c["bits"], c["t0"], K.C_, c["L"], s)
            for r in range(K.R_):
                for ch in range(K.C_):
                    fig, fin, pos_err, pos_iters = S.chain_syn(m, t, s, c["L"], c["W"], c["iters"], e[r, ch], table)
                    want = c["out"][r, ch]
                    assert fig == (want[0], want[1], want[2], want[5], want[6], want[7]), (a, b, r, ch)
                    assert np.array_equal(pos_err, c["pos_err"][r, ch]) and np.array_equal(pos_iters, c["pos_iters"][r, ch])
                    assert np.array_equal(fin.reshape(-1) ^ tx[r, ch], c["hard"][r, ch].astype(bool))


@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_cases_reach_every_branch(shape):
    count = K.counts(shape)
    print(shape, dict(count))
    assert all(count[k] > 0 for k in K.reached(shape)), [k for k in K.reached(shape) if not count[k]]
    if shape == (4, 1, 7):                                     # the perfect code: every non-zero syndrome has its single position
        assert count["roots<L"] == 0 and count["L>t"] == 0


def test_cases_cover_the_frame_layouts():
    seen = {(K.case(K.SHAPES[0], a, b)["w"], K.case(K.SHAPES[0], a, b)["t0"]) for a in range(len(K.LWI)) for b in range(len(K.RATES))}
    assert seen == {(w, t0) for w in K.WS for t0 in K.T0S}
    c = K.case(K.SHAPES[0], 1, 1)
    assert np.isnan(c["llr"]).sum() == K.R_ and (c["llr"] == 0).sum() == 2 * K.R_ and (c["out"][..., 4] > 0).any()
    assert (c["out"][..., 3] > 0).all() and c["pos_iters"].shape[-1] == 1 and K.case(K.SHAPES[0], 3, 1)["pos_iters"].shape[-1] == 4


def test_block_zero_rule():
    """Hand-made patterns: a miscorrection inside block 1, and what pair 1 may not do."""
    m, t, s = 4, 1, 7
    # row 0 of block 1 = positions {s, s + 1}: S_1 = alpha^7 + alpha^8 = alpha^11 (x^4 = x + 1), the single position 11 >= s -- a miscorrection into block 1
    e = np.zeros((1, s, s), bool)
    e[0, 0, :2] = True
    fig, fin, _, _ = S.chain(m, t, s, 1, 1, 4, e)
    assert int(fin.sum()) == 3 and fig[4] == 1 and fig[5] == 1 and fig[1] == 1   # one bad flip made a codeword of weight 3; then clean
    # a pattern whose single position lies below s: pair 1 leaves it alone (status 2), where vaeq_bch_outer's rule alone would flip a bit of block 0
    exp, log = B.tables(m)
    for b1 in range(s):
        for b2 in range(b1 + 1, s):
            p = int(log[exp[s + b1] ^ exp[s + b2]])
            if p < s:
                e = np.zeros((1, s, s), bool)
                e[0, 0, [b1, b2]] = True
                count = collections.Counter()
                fig, fin, _, _ = S.chain(m, t, s, 1, 1, 4, e, count)
                assert count["block0-root"] >= 1 and fig[4] == 0 and fig[1] == 0 and int(fin.sum()) == 2
                return
    raise AssertionError("no pair of positions of the second half sums to a position of the first")

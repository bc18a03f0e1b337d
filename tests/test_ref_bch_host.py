"""tests/_ref_bch.py held to itself, without a device: the field, the generator's degree, the locator model against the restatement that has no
locator (the header's rule by enumeration), every branch of the rule bound by a counted input, and the two stream maps."""
import collections
import itertools
import math

import numpy as np
import pytest

import _ref_bch as B

LIMIT = 3000                                               # patterns per weight, all of them where there are no more


@pytest.mark.parametrize("m", sorted(B.POLY))
def test_alpha_has_order_2m_minus_1(m):
    assert B.order_of_alpha(m) == (1 << m) - 1              # the polynomial is primitive
    exp, log = B.tables(m)
    q = (1 << m) - 1
    assert sorted(exp[:q].tolist()) == list(range(1, q + 1)) and all(log[exp[k]] == k for k in range(q))


def test_parity_values():
    for (m, t), want in B.PARITY.items():
        assert B.parity(m, t) == want, (m, t)
    assert B.parity(4, 8) == 15                             # 2t reaches 2^m - 1: every coset, the one of 0 among them


def _patterns(n_o, wt, rng):
    if math.comb(n_o, wt) <= LIMIT:
        return [list(p) for p in itertools.combinations(range(n_o), wt)]
    return [sorted(rng.choice(n_o, wt, replace=False).tolist()) for _ in range(LIMIT)]


@pytest.mark.parametrize("m,t,n_o", B.SMALL, ids=lambda v: str(v))
def test_model_agrees_with_the_rule_by_enumeration(m, t, n_o):
    table, count, rng = B.Table(m, t, n_o), collections.Counter(), np.random.default_rng(100 * m + 10 * t + n_o)
    for wt in range(0, min(2 * t + 3, n_o) + 1):
        for pos in _patterns(n_o, wt, rng):
            got, want = B.decode(m, t, n_o, pos, count), table.decode(pos)
            assert got == want, (pos, got, want)
            if wt <= t:
                assert got == ((1, pos) if wt else (0, []))  # inside the designed distance: corrected
    print((m, t, n_o), dict(count))
    assert count["status0"] and count["status1"] and count["status2"]               # all three statuses occur in every case


def test_every_branch_binds():
    """Counted over the six small cases: a miscorrection, a locator with L <= t whose root count falls short, a root at a shortened position,
    L > t, and an undetected error from a planted non-zero codeword of the shortened code."""
    count = collections.Counter()
    for m, t, n_o in B.SMALL:
        rng = np.random.default_rng(7 * m + t + n_o)
        for wt in range(t + 1, min(2 * t + 3, n_o) + 1):
            for _ in range(300):
                B.decode(m, t, n_o, sorted(rng.choice(n_o, wt, replace=False).tolist()), count)
        word = B.codeword_of(m, t, n_o, rng)
        if word is not None:
            before = count["undetected"]
            assert B.decode(m, t, n_o, word, count) == (0, []) and count["undetected"] == before + 1 and len(word) >= 2 * t + 1
    print(dict(count))
    for k in ("status1", "status2", "miscorrected", "undetected", "roots<L", "shortened-root", "L>t"):
        assert count[k] > 0, k
    assert B.codeword_of(4, 3, 9) is None                   # 10 parity bits on 9 positions: only the zero word
    assert B.codeword_of(4, 2, 11) is not None


@pytest.mark.parametrize("spread", [0, 1])
@pytest.mark.parametrize("C_o,n_o,K,C", [(8, 15, 28, 5), (23, 9, 42, 5), (12, 255, 620, 5), (1, 8191, 4220, 2)])
def test_stream_maps_are_bijections(C_o, n_o, K, C, spread):
    c, i = B.stream_map(C_o, n_o, K, spread)
    u = (c * K + i).ravel()
    assert c.shape == (C_o, n_o) and sorted(u.tolist()) == list(range(C_o * n_o))   # onto the used bits, each once
    assert c.max() < C and i.max() < K and C_o * n_o <= C * K
    if spread:
        assert np.array_equal(u.reshape(C_o, n_o)[:, 0], np.arange(C_o)) and (C_o == 1 or u.reshape(C_o, n_o)[0, 1] == C_o)
    else:
        assert np.array_equal(u.reshape(C_o, n_o)[0], np.arange(n_o))

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


def _pmul(a, b):
    """The product of two polynomials over GF(2), bit k the coefficient of x^k."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = a << 1, b >> 1
    return r


def _pdivmod(a, b):
    q = 0
    while a.bit_length() >= b.bit_length():
        s = a.bit_length() - b.bit_length()
        q, a = q | 1 << s, a ^ b << s
    return q, a


def _pgcd(a, b):
    while b:
        a, b = b, _pdivmod(a, b)[1]
    return a


def _minimal_polynomial(m, j):
    """The monic polynomial over GF(2) of least degree with the root beta = alpha^j, with no walk over the conjugates: the first power beta^d
    that is a GF(2) combination of 1, beta, .., beta^(d-1) (m-bit vectors, by elimination) gives x^d + that combination."""
    exp, _ = B.tables(m)
    q = (1 << m) - 1
    basis = {}                                              # leading bit -> (reduced vector, the polynomial in beta that produced it)
    for d in range(m + 1):
        v, p = int(exp[j * d % q]), 1 << d
        while v and v.bit_length() - 1 in basis:
            bv, bp = basis[v.bit_length() - 1]
            v, p = v ^ bv, p ^ bp
        if v == 0:
            return p
        basis[v.bit_length() - 1] = (v, p)
    raise AssertionError("m + 1 vectors of m bits are dependent")


def _evaluate(m, poly, j):
    """poly(alpha^j) in GF(2^m)."""
    exp, _ = B.tables(m)
    q, v = (1 << m) - 1, 0
    for k in range(poly.bit_length()):
        if (poly >> k) & 1:
            v ^= int(exp[j * k % q])
    return v


@pytest.mark.parametrize("m", sorted(B.POLY))
def test_parity_over_the_envelope(m):
    """All 16 values of t: parity(m, t) is the degree of the generator, the lcm of the minimal polynomials of alpha^1 .. alpha^2t built by
    polynomial arithmetic over GF(2) -- something that is no coset walk for the three coset walks (this model's, engine.BchCode's and, through
    it and tests/test_abi_refusals_bch_host.py, the entry point's) to answer to -- and BchCode holds that value or refuses the pair."""
    from vae_equalizer_amd.engine import BchCode
    q, g, seen = (1 << m) - 1, 1, []
    for t in range(1, 17):
        for j in (2 * t - 1, 2 * t):
            f = _minimal_polynomial(m, j)
            assert _evaluate(m, f, j) == 0 and f.bit_length() - 1 <= m
            g = _pmul(g, _pdivmod(f, _pgcd(g, f))[0])      # lcm(g, f)
        assert all(_evaluate(m, g, j) == 0 for j in range(1, 2 * t + 1)) and _pdivmod((1 << q) | 1, g)[1] == 0   # g divides x^q + 1
        seen.append(g.bit_length() - 1)
        assert B.parity(m, t) == g.bit_length() - 1, (m, t)
        if B.parity(m, t) < q:
            code = BchCode(m, t)
            assert code.parity == B.parity(m, t) and code.n == q and code.k == q - code.parity
        else:
            with pytest.raises(ValueError):
                BchCode(m, t)
    print(m, seen)
    assert seen == sorted(seen) and seen[0] == m


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

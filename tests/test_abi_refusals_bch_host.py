"""Which error code vaeq_bch_outer returns for which refused arguments, in the style of tests/test_abi_refusals_ldpc_q_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is the LDPC calls' -- empty batch, any NULL pointer (loc
alone may be NULL), the tensor rules with the depth's fit rule, the outer code's own rules, and last the fit of the outer codewords into the
payload, C_o n_o <= C K.  The base call violates that last rule alone (one outer codeword too many), so it never launches on its placeholder
pointers; a case that must be refused for another reason carries a C_o that fits."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 depth n K m t n_o C_o spread post post_i16 bits out loc stream".split()


def _base(**over):
    # 5 bit-packed codewords of 42 bits behind t0 = 11 end in the last of the 29 symbols of 12 bits; 140 payload bits hold 9 words of 15 bits
    d = dict(R=1, C=5, N=-(-5 * 42 // 12) + 11, w=12, t0=11, depth=0, n=42, K=28, m=4, t=2, n_o=15, C_o=10, spread=1, post=P, post_i16=0, bits=P,
             out=P, loc=None, stream=None)
    d.update(over)
    return d


FITS = dict(C_o=9)

CASES = [
    ("empty", _base(R=0, post=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, C=0, m=0, t=0, K=0, depth=-1, spread=7), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("post", "bits", "out")],
    ("null-before-shape", _base(out=None, w=0), NULL), ("null-before-code", _base(post=None, m=3), NULL),
    ("null-before-fit", _base(bits=None), NULL), ("null-before-depth", _base(post=None, depth=-1), NULL),
    # the tensor rules of the LDPC calls (depth 0: the bit-packed fit rule)
    *[(f"{k}={v}", _base(**{**FITS, k: v}), SHAPE)
      for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 6), ("N", 0), ("N", 1 << 30), ("N", 28), ("w", 0), ("w", 65), ("t0", -1), ("t0", 12),
                   ("depth", -1), ("depth", 6), ("n", 1), ("n", 32769), ("n", 44))],
    ("R*C-past-int32", _base(R=1 << 29, C=5, **FITS), SHAPE),
    # the interleaver's fit rule at depth >= 1: 5 codewords of 4 whole symbols need 20 symbols behind t0, the base N has 18
    ("depth=2-symbol-aligned-fit", _base(depth=2, **FITS), SHAPE), ("depth=1-symbol-aligned-fit", _base(depth=1, N=11 + 19, **FITS), SHAPE),
    # one case per rule of the outer code
    *[(f"{k}={v}", _base(**{**FITS, k: v}), SHAPE)
      for k, v in (("K", 0), ("K", 43), ("K", -1), ("m", 3), ("m", 14), ("t", 0), ("t", 17), ("n_o", 16), ("n_o", 8), ("n_o", 0), ("spread", -1),
                   ("spread", 2), ("post_i16", -1), ("post_i16", 2), ("C_o", 0), ("C_o", -1))],
    ("n_o=parity(4,3)", _base(t=3, n_o=10, **FITS), SHAPE), ("parity(4,8)=15-leaves-no-n_o", _base(t=8, n_o=15, **FITS), SHAPE),
    ("R*C_o-past-int32", _base(R=1 << 28, C=5, C_o=9), SHAPE),
    # the last rule alone
    ("fit", _base(), SHAPE), ("fit-spread-off", _base(spread=0), SHAPE), ("fit-K=n", _base(K=42, C_o=15), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_bch_outer
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    return f(*d.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


@pytest.mark.parametrize("over", [dict(), dict(K=1, n_o=15, C_o=1, m=4, t=1), dict(K=42, C_o=15), dict(m=4, t=1, n_o=5, C_o=29), dict(t=3, n_o=11, C_o=13),
                                  dict(m=13, t=16, n_o=8191, C_o=1), dict(m=13, t=16, n_o=209, C_o=1), dict(m=5, t=3, n_o=31, C_o=5),
                                  dict(spread=0), dict(post_i16=1), dict(depth=1, N=11 + 20), dict(depth=5, N=11 + 20), dict(n=2, K=2, C_o=1),
                                  dict(t0=0, N=18), dict(w=64, N=11 + 4), dict(w=1, N=11 + 210)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "base")
def test_the_edges_of_the_ranges_pass_every_rule_but_the_last(over):
    """The edges of the ranges as far as a call without a device can take them: each of these calls asks for one outer codeword more than the
    payload holds (or many more) and ends at the last rule, behind all the others; R == 0 with the same arguments is VAEQ_OK.  That the same
    values with a C_o that fits are accepted and decoded is tests/test_bch_gpu.py's to show."""
    d = _base(**over)
    assert d["C_o"] * d["n_o"] > d["C"] * d["K"]            # by construction: the last rule alone
    assert _call(d) == SHAPE and _call(dict(d, R=0)) == OK
    assert _call(dict(d, m=3)) == SHAPE and _call(dict(d, post=None)) == NULL


@pytest.mark.parametrize("m", range(4, 14))
def test_the_lengths_on_both_sides_of_the_envelope_are_refused(m):
    """Every admissible (m, t): n_o == parity(m, t), which leaves no message bit, and n_o == 2^m, one past the full length, are refused, and
    by the outer code's own rules alone -- one outer codeword on one LDPC codeword of 8192 payload bits, so every other rule passes, the fit
    included.  The entry point's own coset walk is reached in no other way; that n_o == parity + 1 is accepted and decoded is
    tests/test_bch_envelope_gpu.py's to show."""
    import _ref_bch as B
    q, seen = (1 << m) - 1, 0
    for t in range(1, 17):
        par = B.parity(m, t)
        if par >= q:
            continue
        seen += 1
        for n_o in (par, 1 << m):
            d = _base(C=1, n=8192, K=8192, N=-(-8192 // 12), t0=0, m=m, t=t, n_o=n_o, C_o=1)
            assert d["C_o"] * d["n_o"] <= d["C"] * d["K"] and d["t0"] * d["w"] + d["C"] * d["n"] <= d["N"] * d["w"]
            assert _call(d) == SHAPE, (m, t, n_o)
            assert _call(dict(d, R=0)) == OK and _call(dict(d, out=None)) == NULL
    assert seen == {4: 7, 5: 15}.get(m, 16)


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_bch_outer(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t K, int32_t m, int32_t t" in header
    assert "const void *post, int32_t post_i16, const int8_t *bits, int32_t *out, int16_t *loc, void *stream);" in header
    for poly in ("0x13", "0x25", "0x43", "0x89", "0x11D", "0x211", "0x409", "0x805", "0x1053", "0x201B"):
        assert poly in header
    assert "vaeq_bch_outer" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_bch_outer")
    assert "vaeq_bch.hip" in nat.SOURCES and "vaeq_ldpc.h" in nat.HEADERS and "vaeq_fec.h" in nat.HEADERS
    for fn in ("vaeq_ldpc_decode", "vaeq_ldpc_decode_il", "vaeq_ldpc_decode_q"):  # the inner decoders stay beside it
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)

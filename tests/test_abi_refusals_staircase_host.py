"""Which error code vaeq_staircase_decode returns for which refused arguments, in the style of tests/test_abi_refusals_ldpc_sc_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_ldpc_sc_decode's -- empty batch, any NULL pointer
(hard, pos_err and pos_iters may be NULL), shape.  Then the state formula with the two sides of its limit, and the ValueErrors of
engine.StaircaseCode and engine.check_fec, which are raised before anything is allocated."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 m t s L llr bits W iters out hard pos_err pos_iters stream".split()


def _base(**over):
    d = dict(R=1, C=2, N=157, w=12, t0=7, m=5, t=2, s=15, L=4, llr=P, bits=P, W=3, iters=8, out=P, hard=None, pos_err=None, pos_iters=None,
             stream=None)                                   # would be accepted: 2 chains of 4 x 225 bits end in the last symbol, 150 x 12 bits behind t0
    d.update(over)
    return d


CASES = [
    ("empty", _base(R=0, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, m=0, s=0, iters=0, W=0, L=0), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("llr", "bits", "out")],
    ("null-before-shape", _base(out=None, m=11), NULL), ("null-before-fit", _base(llr=None, C=3), NULL),
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 3), ("N", 0), ("N", 1 << 30), ("N", 156), ("w", 0),
                                                        ("w", 65), ("t0", -1), ("t0", 8), ("t0", 158), ("iters", 0), ("iters", 101), ("m", 3),
                                                        ("m", 11), ("t", 0), ("t", 9), ("s", 1), ("s", 16), ("L", 0), ("L", 65536), ("W", 0),
                                                        ("W", 33))],
    ("s=512", _base(m=10, s=512, N=1 << 20), SHAPE), ("m=11-fits", _base(m=11, s=100, N=1 << 20), SHAPE),
    ("2s=2^m", _base(m=6, s=32, N=1 << 20), SHAPE),                                      # 2 s = 64 > 63
    ("parity=2s", _base(s=5, N=100), SHAPE),                                              # parity(5, 2) = 10 = 2 s: no information bit
    ("parity>2s", _base(t=3, s=7, N=100), SHAPE),                                         # parity(5, 3) = 15 > 14
    ("R*C-past-int32", _base(R=1 << 30, C=2), SHAPE),
    ("state-65696", _base(m=10, t=8, s=350, L=2, W=1, N=1 << 20), SHAPE),                 # one step above the largest: s = 349 is 65 520
    ("oversize-state", _base(m=10, s=511, W=32, N=1 << 29), SHAPE),
    # the fit rule where C n_chain passes 2^63: n_chain = 65535 x 349^2 = 7 982 228 535 in an allowed state of 65 520 bytes, and a product
    # formed in int64 wraps negative for every C above 2^63 / n_chain = 1 155 488 344, which would let the call through
    *[(f"fit-past-int64-C={C}", _base(C=C, N=1, w=1, t0=0, m=10, t=8, s=349, L=65535, W=1), SHAPE) for C in (0x7fffffff, 1155488345)],
    ("fit-one-chain-too-long", _base(C=1, N=(1 << 30) - 1, w=7, t0=0, m=10, t=8, s=349, L=65535, W=1), SHAPE),   # 7.52e9 bits of room
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_staircase_decode
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    return f(*d.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_staircase_lds_bytes
    assert f(8, 120, 4) == 4 * 256 + 8 * 5 * 120 * 4 == 20224      # the tables, and W + 1 blocks twice: 120 rows of 4 words
    assert f(4, 7, 1) == 64 + 8 * 2 * 7 * 1 and f(7, 33, 3) == 512 + 8 * 4 * 33 * 2    # a row below a word; a row that crosses one
    assert f(10, 349, 1) == 65520 <= 64 * 1024 < f(10, 350, 1) == 65696                # the two sides of the limit
    assert f(10, 511, 32) > 64 * 1024
    for bad in ((3, 7, 1), (11, 100, 1), (8, 1, 4), (10, 512, 1), (8, 128, 4), (4, 8, 1), (8, 120, 0), (8, 120, 33)):
        assert f(*bad) == SHAPE


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_staircase_decode(" in header and "int64_t vaeq_staircase_lds_bytes(" in header
    for fn in ("vaeq_staircase_decode", "vaeq_staircase_lds_bytes"):
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)
    assert "vaeq_staircase.hip" in nat.SOURCES


def test_staircase_code():
    from vae_equalizer_amd.engine import BchCode, StaircaseCode
    c = StaircaseCode(BchCode(8, 3, n=240), 8)
    assert (c.s, c.L, c.n, c.component.parity) == (120, 8, 115200, 24) and c.rate == 1 - 24 / 120
    assert StaircaseCode(BchCode(5, 2, n=12), 1).rate < 0    # a decoder test, not a code
    for bad in (lambda: StaircaseCode(BchCode(8, 3, n=241), 8), lambda: StaircaseCode(BchCode(11, 3, n=240), 8),
                lambda: StaircaseCode(BchCode(10, 9, n=1000), 8), lambda: StaircaseCode(BchCode(8, 3, n=240), 0),
                lambda: StaircaseCode(BchCode(8, 3, n=240), 65536), lambda: StaircaseCode(BchCode(8, 3, n=240), 2.5),
                lambda: StaircaseCode((8, 3, 240), 8), lambda: StaircaseCode(BchCode(8, 3, n=240), True)):
        with pytest.raises(ValueError):
            bad()


def test_check_fec():
    from vae_equalizer_amd.engine import BchCode, StaircaseCode, array_code, check_fec, fec_figures, sc_array_code
    code = StaircaseCode(BchCode(5, 2, n=30), 4)
    check_fec(dict(code=code, window=3))
    check_fec(dict(code=code, window=3, t0=7, iters=4))
    for bad in (dict(code=code), dict(code=code, window=None), dict(code=code, window=3, max_iter=8), dict(code=code, window=3, alpha=0.75),
                dict(code=code, window=3, test=1), dict(code=code, window=3, depth=2), dict(code=code, window=3, quant=dict(bits=5)),
                dict(code=code, window=3, fixed=dict(bits=5)), dict(code=code, window=3, outer=dict(code=BchCode(8, 2))),
                dict(code=code, window=3, chains=1), dict(code=code, wnidow=3)):
        with pytest.raises(ValueError):
            check_fec(bad)
        with pytest.raises(ValueError):                     # before anything is allocated: the LLRs are never looked at
            fec_figures(None, bad)
    check_fec(None)                                         # every other code: what it was
    check_fec(dict(code=array_code(4, 24, 31), max_iter=8))
    check_fec(dict(code=sc_array_code(2, 4, 31, 12), window=5))
    for bad in (dict(code=array_code(4, 24, 31), window=5), dict(code=sc_array_code(2, 4, 31, 12)), dict(window=3)):
        with pytest.raises(ValueError):
            check_fec(bad)

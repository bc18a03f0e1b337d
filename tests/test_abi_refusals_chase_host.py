"""Which error code vaeq_chase_decode returns for which refused arguments, in the style of tests/test_abi_refusals_staircase_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_ldpc_decode's -- empty batch, any NULL pointer
(the two stream pointers come as a pair or not at all), shape, and last the table of columns, which is the only thing read through a pointer
(cols_host is host memory).  Then the ValueErrors of engine.HammingCode, engine.hamming_code and engine.check_fec's inner=, which are raised
before anything is allocated."""
import ctypes

import numpy as np
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 depth n r cols_host llr bits p K spread out llr_out bits_out stream".split()
_KEEP = []                                                 # the column arrays stay alive while the case list does


def _cols(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32))
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


GOOD = _cols(np.arange(15) + 1)


def _base(**over):
    d = dict(R=1, C=8, N=17, w=12, t0=7, depth=0, n=15, r=4, cols_host=GOOD, llr=P, bits=P, p=4, K=11, spread=1, out=P, llr_out=None,
             bits_out=None, stream=None)                    # would be accepted: 8 words of 15 bits end in the last symbol, 10 x 12 bits behind t0
    d.update(over)
    return d


CASES = [
    ("empty", _base(R=0, cols_host=None, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, n=0, r=0, p=9, K=0, llr_out=P), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("cols_host", "llr", "bits", "out")],
    ("llr_out-alone", _base(llr_out=P), NULL), ("bits_out-alone", _base(bits_out=P), NULL),
    ("null-before-shape", _base(out=None, n=2), NULL), ("stream-pair-before-shape", _base(llr_out=P, r=11), NULL),
    ("null-before-table", _base(llr=None, cols_host=_cols([1] * 15)), NULL),
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 9), ("N", 0), ("N", 1 << 30), ("N", 16), ("w", 0),
                                                        ("w", 65), ("t0", -1), ("t0", 8), ("t0", 18), ("depth", -1), ("depth", 9), ("n", 2),
                                                        ("n", 257), ("r", 1), ("r", 11), ("p", -1), ("p", 7), ("K", 0), ("K", 16), ("spread", -1),
                                                        ("spread", 2))],
    ("p>n", _base(n=5, p=6, K=3), SHAPE), ("p=n=5-table", _base(n=5, p=5, K=3, cols_host=_cols([1, 2, 3, 4, 4])), SHAPE),   # p = n passes, its table does not
    ("il-fit", _base(depth=2, N=22), SHAPE),                                             # 8 words of ceil(15 / 12) = 2 symbols behind t0 = 7 need 23
    ("il-fit-depth-C", _base(depth=8, N=22), SHAPE),
    ("R*C-past-int32", _base(R=1 << 28, C=8), SHAPE),
    ("C*K-past-stream", _base(C=1 << 29, N=0x3fffffff, w=4, t0=0, n=3, r=2, p=0, K=3, cols_host=_cols([1, 2, 3]), llr_out=P, bits_out=P), SHAPE),
    ("C*K-at-limit-table", _base(C=0x3fffffff // 3, N=0x3fffffff, w=1, t0=0, n=3, r=2, p=0, K=3, cols_host=_cols([1, 2, 2]), llr_out=P, bits_out=P),
     SHAPE),                                                                              # C K = 0x3fffffff passes the stream bound: the table refuses
    ("shape-before-table", _base(n=16, cols_host=_cols([0] * 16), C=9), SHAPE),
    ("duplicate-column", _base(cols_host=_cols(list(range(1, 15)) + [14])), SHAPE),
    ("zero-column", _base(cols_host=_cols([0] + list(range(2, 16)))), SHAPE),
    ("negative-column", _base(cols_host=_cols([-1] + list(range(2, 16)))), SHAPE),
    ("column=2^r", _base(cols_host=_cols(list(range(1, 15)) + [16])), SHAPE),
    ("column=2^r-r10", _base(r=10, cols_host=_cols(list(range(1, 15)) + [1024])), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_chase_decode
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    return f(*d.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_chase_decode(" in header
    assert "vaeq_chase_decode" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_chase_decode")
    assert "vaeq_chase.hip" in nat.SOURCES and "vaeq_ldpc.h" in nat.HEADERS and "vaeq_fec.h" in nat.HEADERS


def test_hamming_code():
    from vae_equalizer_amd.engine import HammingCode, hamming_code
    c = hamming_code(7)
    assert (c.n, c.r, c.k, c.rank) == (128, 8, 120, 8) and c.cols.dtype == np.int32 and c.cols.tolist() == [(j << 1) | 1 for j in range(128)]
    c = hamming_code(3, extended=False)
    assert (c.n, c.r, c.k) == (7, 3, 4) and c.cols.tolist() == [1, 2, 3, 4, 5, 6, 7] and c.rate == 4 / 7
    assert (hamming_code(8).n, hamming_code(8).r, hamming_code(8).k) == (256, 9, 247)
    c = hamming_code(7, n=100)
    assert (c.n, c.r, c.k) == (100, 8, 92) and c.cols.tolist() == [(j << 1) | 1 for j in range(100)]
    assert hamming_code(7, n=3).k == 0                       # columns 1, 3, 5: rank 3
    c = HammingCode([1, 2, 4, 8], 4)
    assert (c.n, c.r, c.rank, c.k) == (4, 4, 4, 0) and HammingCode([1, 2, 3], 2).k == 1
    for bad in (lambda: HammingCode([1, 2], 2), lambda: HammingCode(list(range(1, 258)), 10), lambda: HammingCode([1, 2, 3], 1),
                lambda: HammingCode([1, 2, 3], 11), lambda: HammingCode([1, 2, 2], 2), lambda: HammingCode([0, 1, 2], 2),
                lambda: HammingCode([1, 2, 4], 2), lambda: HammingCode([1, 2, -3], 2), lambda: HammingCode([1.0, 2.0, 3.0], 2),
                lambda: HammingCode([[1, 2, 3]], 2), lambda: HammingCode([1, 2, 3], 2.0), lambda: HammingCode([1, 2, 3], True),
                lambda: hamming_code(0), lambda: hamming_code(10), lambda: hamming_code(11, extended=False), lambda: hamming_code(7, n=129),
                lambda: hamming_code(7, n=2), lambda: hamming_code(7, extended=False, n=128), lambda: hamming_code(7.0), lambda: hamming_code(7, n=64.0),
                lambda: hamming_code(8, extended=False, n=0)):
        with pytest.raises(ValueError):
            bad()
    assert hamming_code(8, extended=False, n=255).n == 255 and hamming_code(10, extended=False, n=256).r == 10


def test_check_fec_inner():
    from vae_equalizer_amd.engine import BchCode, StaircaseCode, array_code, chase_decode, check_fec, fec_figures, hamming_code
    code, ham = StaircaseCode(BchCode(5, 1, n=24), 3), hamming_code(4)
    check_fec(dict(code=code, window=2, inner=dict(code=ham)))
    check_fec(dict(code=code, window=2, t0=3, iters=4, inner=dict(code=ham, patterns=6, depth=2, payload=11, spread=False)))
    check_fec(dict(code=code, window=2, inner=None))         # as absent
    for inner in (dict(), dict(patterns=4), dict(code=BchCode(5, 1)), dict(code=(16, 11)), dict(code=ham, patterns=7), dict(code=ham, patterns=-1),
                  dict(code=ham, patterns=2.0), dict(code=ham, payload=0), dict(code=ham, payload=17), dict(code=ham, depth=0),
                  dict(code=ham, codewords=4), dict(code=ham, t0=3), dict(code=hamming_code(4, n=3)), dict(code=hamming_code(4, n=5), patterns=6),
                  ham, 4):
        bad = dict(code=code, window=2, inner=inner)
        with pytest.raises(ValueError):
            check_fec(bad)
        with pytest.raises(ValueError):                     # before anything is allocated: the LLRs are never looked at
            fec_figures(None, bad)
    for other in (dict(code=array_code(4, 24, 31), inner=dict(code=ham)), dict(code=BchCode(5, 1), inner=dict(code=ham)),
                  dict(code=ham, window=2), dict(inner=dict(code=ham), window=2)):
        with pytest.raises(ValueError):                     # inner belongs to a StaircaseCode
            check_fec(other)
    with pytest.raises(ValueError):
        chase_decode(None, None, BchCode(5, 1))

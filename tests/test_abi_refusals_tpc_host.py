"""Which error code vaeq_tpc_decode returns for which refused arguments, in the style of tests/test_abi_refusals_chase_host.py: every argument set
below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_chase_decode's -- empty batch, any NULL pointer (the
two stream pointers come as a pair or not at all; scale, ext and half_err may be NULL), shape, the LDS bound, and last the two tables of columns.
The two tables and the two schedules are the only things read through a pointer (host memory).  The fit rule: with C an int32 and n at most 2^16
the product C n stays below 2^47, so it cannot pass 2^63 inside this ABI; the largest C there is is refused by the rule all the same.  Then
vaeq_tpc_lds_bytes, and the ValueErrors of engine.ProductCode, engine.tpc_decode and engine.check_fec, raised before anything is allocated."""
import ctypes

import numpy as np
import pytest

OK, NULL, SHAPE, LDS = 0, -1, -2, -3
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = ("R C N w t0 n1 r1 cols1_host n2 r2 cols2_host llr bits p iters alpha_host beta_host scale clip K1 K2 out llr_out bits_out ext half_err "
         "stream").split()
_KEEP = []                                                 # the host arrays stay alive while the case list does


def _host(values, dtype):
    a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _cols(values):
    return _host(values, np.int32)


def _sched(values):
    return _host(values, np.float32)


H7, E16 = _cols(np.arange(7) + 1), _cols(2 * np.arange(16) + 1)
E256, E128 = _cols(2 * np.arange(256) + 1), _cols(2 * np.arange(128) + 1)
ALPHA, BETA = _sched([0, .2, .3, .5] + [1] * 28), _sched([.2, .4, .6, .8] + [1] * 28)


def _base(**over):
    d = dict(R=1, C=3, N=33, w=12, t0=5, n1=7, r1=3, cols1_host=H7, n2=16, r2=5, cols2_host=E16, llr=P, bits=P, p=4, iters=2, alpha_host=ALPHA,
             beta_host=BETA, scale=None, clip=ctypes.c_float(2.0 ** 60), K1=4, K2=11, out=P, llr_out=None, bits_out=None, ext=None, half_err=None,
             stream=None)                                   # would be accepted: 3 blocks of 112 bits end in the last symbol, 28 x 12 bits behind t0
    d.update(over)
    if not isinstance(d["clip"], ctypes.c_float):
        d["clip"] = ctypes.c_float(d["clip"])
    return d


CASES = [
    ("empty", _base(R=0, cols1_host=None, cols2_host=None, llr=None, bits=None, alpha_host=None, beta_host=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, n1=0, r2=0, p=9, K1=0, llr_out=P, clip=0.0), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("cols1_host", "cols2_host", "llr", "bits", "alpha_host", "beta_host", "out")],
    ("llr_out-alone", _base(llr_out=P), NULL), ("bits_out-alone", _base(bits_out=P), NULL),
    ("null-before-shape", _base(out=None, n1=2), NULL), ("stream-pair-before-shape", _base(llr_out=P, r1=11), NULL),
    ("null-before-lds", _base(llr=None, n1=256, r1=9, cols1_host=E256, n2=256, r2=9, cols2_host=E256), NULL),
    ("null-before-table", _base(bits=None, cols1_host=_cols([1] * 7)), NULL),
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 4), ("N", 0), ("N", 1 << 30), ("N", 32), ("w", 0),
                                                        ("w", 65), ("t0", -1), ("t0", 6), ("t0", 34), ("n1", 2), ("n1", 257), ("n2", 2),
                                                        ("n2", 257), ("r1", 1), ("r1", 11), ("r2", 1), ("r2", 11), ("p", -1), ("p", 7),
                                                        ("iters", 0), ("iters", 17), ("clip", 0.0), ("clip", -1.0), ("clip", float("nan")),
                                                        ("clip", float("inf")), ("clip", 2.0 ** 97), ("K1", 0), ("K1", 8), ("K2", 0), ("K2", 17))],
    ("p>n1", _base(n1=5, p=6, K1=3), SHAPE), ("p>n2", _base(n2=5, p=6, K2=3), SHAPE),
    ("p=n1=5-table", _base(n1=5, p=5, K1=3, C=4, cols1_host=_cols([1, 2, 3, 4, 4])), SHAPE),       # p = n1 passes, the table does not
    *[(f"alpha[{h}]={v}", _base(alpha_host=_sched([0.0] * h + [v] + [0.0] * 8)), SHAPE) for h, v in ((0, -0.5), (3, 16.5), (1, np.nan), (2, np.inf))],
    *[(f"beta[{h}]={v}", _base(beta_host=_sched([0.0] * h + [v] + [0.0] * 8)), SHAPE) for h, v in ((0, -0.5), (3, np.inf), (1, np.nan))],
    ("alpha-past-2-iters-unread", _base(alpha_host=_sched([0, 0, 0, 0, np.nan]), cols2_host=_cols([0] * 16)), SHAPE),   # alpha[4] is not the refusal: the table is
    ("clip=2^96-table", _base(clip=2.0 ** 96, cols1_host=_cols([1] * 7)), SHAPE),
    ("largest-C-fit", _base(C=0x7fffffff, N=0x3fffffff, w=64, t0=0, n1=256, r1=9, cols1_host=E256, n2=256, r2=9, cols2_host=E256), SHAPE),
    ("fit-before-lds", _base(C=4, n1=256, r1=9, cols1_host=E256, n2=256, r2=9, cols2_host=E256), SHAPE),
    ("R*C-past-int32", _base(R=1 << 30, C=3), SHAPE),
    ("C*n-past-stream", _base(C=1 << 26, N=0x3fffffff, w=4, t0=0, n1=3, r1=2, n2=6, r2=3, p=0, K1=1, K2=1, cols1_host=_cols([1, 2, 3]),
                              cols2_host=_cols([1, 2, 3, 4, 5, 6]), llr_out=P, bits_out=P), SHAPE),                   # C n = 18 * 2^26 > 0x3fffffff
    ("C*n-at-limit-table", _base(C=0x3fffffff // 9, N=0x3fffffff, w=1, t0=0, n1=3, r1=2, n2=3, r2=2, p=0, K1=1, K2=1, cols1_host=_cols([1, 2, 2]),
                                 cols2_host=_cols([1, 2, 3]), llr_out=P, bits_out=P), SHAPE),                         # passes the stream bound: the table refuses
    ("lds", _base(C=1, N=1 << 20, t0=0, n1=256, r1=9, cols1_host=E256, n2=256, r2=9, cols2_host=E256, K1=1, K2=1), LDS),
    ("lds-256x64", _base(C=1, N=1 << 20, t0=0, n1=256, r1=9, cols1_host=E256, n2=64, r2=7, cols2_host=E128, K1=1, K2=1), LDS),
    ("shape-before-lds", _base(C=1, N=1 << 20, t0=0, n1=256, r1=9, cols1_host=E256, n2=256, r2=9, cols2_host=E256, K1=257), SHAPE),
    ("lds-before-table", _base(C=1, N=1 << 20, t0=0, n1=256, r1=9, cols1_host=_cols([0] * 256), n2=256, r2=9, cols2_host=E256, K1=1, K2=1), LDS),
    ("shape-before-table", _base(cols1_host=_cols([0] * 7), C=4), SHAPE),
    ("duplicate-column-1", _base(cols1_host=_cols([1, 2, 3, 4, 5, 6, 6])), SHAPE), ("duplicate-column-2", _base(cols2_host=_cols([1] * 16)), SHAPE),
    ("zero-column", _base(cols1_host=_cols([0, 2, 3, 4, 5, 6, 7])), SHAPE), ("negative-column", _base(cols2_host=_cols([-1] + list(range(2, 17)))), SHAPE),
    ("column=2^r1", _base(cols1_host=_cols([1, 2, 3, 4, 5, 6, 8])), SHAPE), ("column=2^r2", _base(cols2_host=_cols(list(range(1, 16)) + [32])), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_tpc_decode
    assert len(NAMES) == len(f.argtypes) and list(d) == list(NAMES)
    return f(*d.values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_tpc_decode(" in header and "int64_t vaeq_tpc_lds_bytes(" in header
    assert {"vaeq_tpc_decode", "vaeq_tpc_lds_bytes"} <= set(nat.EXPORTS) and hasattr(nat.lib(), "vaeq_tpc_decode")
    assert "vaeq_tpc.hip" in nat.SOURCES


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_tpc_lds_bytes

    def formula(n1, r1, n2, r2):
        cells, waves = n1 * (n2 | 1), 16 if n1 * n2 > 4096 else 4
        return 8 * cells + (cells + 3) // 4 * 4 + 4 * waves * max(n1, n2) + (2 * (n1 + n2) + 3) // 4 * 4 + 2 * ((1 << r1) + (1 << r2))

    assert f(128, 8, 128, 8) == formula(128, 8, 128, 8) == 158336 <= 156 * 1024          # the extended (128, 120)^2 block fits
    assert f(256, 9, 256, 9) == LDS and formula(256, 9, 256, 9) > 160 * 1024
    assert f(256, 9, 60, 7) == formula(256, 9, 60, 7) <= 156 * 1024 and f(256, 9, 64, 7) == LDS
    for shape in ((7, 3, 16, 5), (20, 6, 100, 8), (32, 6, 32, 6), (64, 7, 64, 7), (3, 2, 3, 2), (7, 3, 7, 3), (64, 7, 65, 8)):
        assert f(*shape) == formula(*shape), shape
    for shape in ((2, 3, 16, 5), (257, 9, 16, 5), (7, 1, 16, 5), (7, 11, 16, 5), (7, 3, 2, 5), (7, 3, 257, 5), (7, 3, 16, 1), (7, 3, 16, 11)):
        assert f(*shape) == SHAPE, shape


def test_product_code_and_value_errors():
    from vae_equalizer_amd.engine import BchCode, ProductCode, StaircaseCode, check_fec, fec_figures, hamming_code, resolve_tpc, tpc_decode
    h7, e16, e128 = hamming_code(3, extended=False), hamming_code(4), hamming_code(7)
    code = ProductCode(h7, e16)
    assert (code.n, code.k, code.rate, code.col, code.row) == (112, 44, 44 / 112, h7, e16)
    big = ProductCode(e128, e128)
    assert (big.n, big.k) == (16384, 14400)
    for bad in (lambda: ProductCode(h7, (16, 11)), lambda: ProductCode(BchCode(5, 1), e16), lambda: ProductCode(hamming_code(8), hamming_code(8)),
                lambda: ProductCode(h7, None)):
        with pytest.raises(ValueError):
            bad()
    prm = resolve_tpc(code)
    assert prm["iters"] == 4 and prm["patterns"] == 4 and prm["clip"] == 2.0 ** 60 and prm["payload"] == (4, 11)
    assert prm["alpha"].dtype == np.float32 and prm["alpha"].tolist() == np.array([0, .2, .3, .5, .7, .9, 1, 1], np.float32).tolist()
    assert prm["beta"].tolist() == np.array([.2, .4, .6, .8, 1, 1, 1, 1], np.float32).tolist()
    assert resolve_tpc(code, iters=6)["alpha"].tolist()[8:] == [1.0] * 4 and resolve_tpc(code, iters=1)["beta"].tolist() == np.array([.2, .4], np.float32).tolist()
    check_fec(dict(code=code))
    check_fec(dict(code=code, t0=3, iters=2, patterns=6, alpha=[0, .5, 1, 1], beta=(1, 1, 1, 1), scale=2.0, clip=64.0))
    check_fec(dict(code=code, iters=None, alpha=None))       # as absent
    for extra in (dict(window=2), dict(max_iter=20), dict(outer=dict(code=BchCode(5, 1))), dict(inner=dict(code=e16)), dict(depth=2), dict(payload=(4, 11)),
                  dict(blocks=2), dict(iters=0), dict(iters=17), dict(iters=2.0), dict(patterns=7), dict(patterns=-1), dict(patterns=True),
                  dict(alpha=[0, .2]), dict(alpha=[0] * 7 + [17]), dict(alpha=[0] * 7 + [float("nan")]), dict(beta=[-1] + [0] * 7), dict(beta="x"),
                  dict(beta=[0] * 7 + [float("inf")]), dict(clip=0), dict(clip=-1.0), dict(clip=float("inf")), dict(clip=2.0 ** 97), dict(clip="big")):
        bad = dict(code=code, **extra)
        with pytest.raises(ValueError):
            check_fec(bad)
        with pytest.raises(ValueError):                     # before anything is allocated: the LLRs are never looked at
            fec_figures(None, bad)
    for other in (dict(code=StaircaseCode(BchCode(5, 1, n=24), 3), window=2, patterns=4), dict(code=StaircaseCode(BchCode(5, 1, n=24), 3), window=2, beta=[1]),
                  dict(patterns=4), dict(code=e16, patterns=4)):
        with pytest.raises(ValueError):                     # the product decoder's keys belong to a ProductCode
            check_fec(other)
    for bad in (lambda: tpc_decode(None, None, e16), lambda: tpc_decode(None, None, code, payload=(0, 11)), lambda: tpc_decode(None, None, code, payload=(4, 17)),
                lambda: tpc_decode(None, None, code, payload=4), lambda: tpc_decode(None, None, code, patterns=7)):
        with pytest.raises(ValueError):
            bad()

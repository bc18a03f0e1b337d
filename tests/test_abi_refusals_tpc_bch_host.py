"""Which error code vaeq_chase_bch_decode and vaeq_tpc_bch_decode return for which refused arguments, in the style of
tests/test_abi_refusals_tpc_host.py: every argument set below is refused on the host before any HIP call, so no device is needed.  The order is
their siblings' -- empty batch, any NULL pointer (the two stream pointers come as a pair or not at all; scale, ext and half_err may be NULL), shape
(the envelope of the codes in the place of the tables' dimensions), and for the product the LDS bound last: there is no table to validate.  Then
vaeq_tpc_bch_lds_bytes at the extended (128, 113)^2 fit and at the first shapes above the bound, and the ValueErrors of engine.EbchCode,
engine.ProductCode, engine.chase_decode, engine.resolve_inner and engine.check_fec, raised before anything is allocated."""
import ctypes

import numpy as np
import pytest

OK, NULL, SHAPE, LDS = 0, -1, -2, -3
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call
_KEEP = []


def _sched(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


ALPHA, BETA = _sched([0, .2, .3, .5] + [1] * 28), _sched([.2, .4, .6, .8] + [1] * 28)

# ---- vaeq_chase_bch_decode ----

CHASE_NAMES = "R C N w t0 depth m n ext llr bits p K spread out llr_out bits_out stream".split()


def _chase(**over):
    d = dict(R=1, C=3, N=13, w=12, t0=5, depth=0, m=5, n=32, ext=1, llr=P, bits=P, p=4, K=21, spread=1, out=P, llr_out=None, bits_out=None,
             stream=None)                                   # would be accepted: 3 words of 32 bits are the 8 x 12 bits behind t0
    d.update(over)
    return d


CHASE_CASES = [
    ("empty", _chase(R=0, llr=None, bits=None, out=None), OK), ("empty-bad-shape", _chase(R=0, m=3, n=0, p=9, K=0, llr_out=P), OK),
    *[(f"null-{k}", _chase(**{k: None}), NULL) for k in ("llr", "bits", "out")],
    ("llr_out-alone", _chase(llr_out=P), NULL), ("bits_out-alone", _chase(bits_out=P), NULL),
    ("null-before-shape", _chase(out=None, m=9), NULL), ("stream-pair-before-shape", _chase(llr_out=P, n=5), NULL),
    *[(f"{k}={v}", _chase(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", 4), ("N", 0), ("N", 1 << 30), ("N", 12), ("w", 0), ("w", 65),
                                                         ("t0", -1), ("t0", 6), ("t0", 14), ("depth", -1), ("depth", 4), ("m", 3), ("m", 9),
                                                         ("ext", -1), ("ext", 2), ("n", 11), ("n", 33), ("p", -1), ("p", 7), ("K", 0), ("K", 33),
                                                         ("spread", -1), ("spread", 2))],
    ("n_i=2m", _chase(n=10, ext=0, K=1), SHAPE), ("n_i=2^m-plain", _chase(n=32, ext=0), SHAPE),
    ("m=4-n=9-ext", _chase(m=4, n=9, ext=1, K=1), SHAPE), ("m=8-n=257", _chase(m=8, n=257, ext=1, C=1, N=1 << 10), SHAPE),
    ("il-fit", _chase(depth=1, N=13), SHAPE),               # behind the interleaver a word takes ceil(32 / 12) = 3 symbols: 5 + 9 > 13
    ("R*C-past-int32", _chase(R=1 << 30, C=3), SHAPE),
    ("C*K-past-stream", _chase(C=1 << 26, N=0x3fffffff, w=4, t0=0, K=21, llr_out=P, bits_out=P), SHAPE),
]

# ---- vaeq_tpc_bch_decode ----

TPC_NAMES = ("R C N w t0 m1 n1 ext1 m2 n2 ext2 llr bits p iters alpha_host beta_host scale clip K1 K2 out llr_out bits_out ext half_err "
             "stream").split()


def _tpc(**over):
    d = dict(R=1, C=3, N=45, w=12, t0=5, m1=4, n1=10, ext1=1, m2=4, n2=16, ext2=1, llr=P, bits=P, p=4, iters=2, alpha_host=ALPHA, beta_host=BETA,
             scale=None, clip=ctypes.c_float(2.0 ** 60), K1=1, K2=7, out=P, llr_out=None, bits_out=None, ext=None, half_err=None,
             stream=None)                                   # would be accepted: 3 blocks of 160 bits are the 40 x 12 bits behind t0
    d.update(over)
    if not isinstance(d["clip"], ctypes.c_float):
        d["clip"] = ctypes.c_float(d["clip"])
    return d


BIG = dict(C=1, N=1 << 20, t0=0, m1=8, n1=256, ext1=1, m2=8, n2=256, ext2=1, K1=1, K2=1)
TPC_CASES = [
    ("empty", _tpc(R=0, llr=None, bits=None, alpha_host=None, beta_host=None, out=None), OK),
    ("empty-bad-shape", _tpc(R=0, m1=0, n2=0, p=9, K1=0, llr_out=P, clip=0.0), OK),
    *[(f"null-{k}", _tpc(**{k: None}), NULL) for k in ("llr", "bits", "alpha_host", "beta_host", "out")],
    ("llr_out-alone", _tpc(llr_out=P), NULL), ("bits_out-alone", _tpc(bits_out=P), NULL),
    ("null-before-shape", _tpc(out=None, m1=3), NULL), ("stream-pair-before-shape", _tpc(llr_out=P, ext2=2), NULL),
    ("null-before-lds", _tpc(llr=None, **BIG), NULL),
    *[(f"{k}={v}", _tpc(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", 4), ("N", 0), ("N", 1 << 30), ("N", 44), ("w", 0), ("w", 65),
                                                       ("t0", -1), ("t0", 6), ("t0", 46), ("m1", 3), ("m1", 9), ("m2", 3), ("m2", 9), ("ext1", -1),
                                                       ("ext1", 2), ("ext2", -1), ("ext2", 2), ("n1", 9), ("n1", 17), ("n2", 9), ("n2", 17),
                                                       ("p", -1), ("p", 7), ("iters", 0), ("iters", 17), ("clip", 0.0), ("clip", -1.0),
                                                       ("clip", float("nan")), ("clip", float("inf")), ("clip", 2.0 ** 97), ("K1", 0), ("K1", 11),
                                                       ("K2", 0), ("K2", 17))],
    ("n1-plain-2m", _tpc(n1=8, ext1=0), SHAPE), ("n2-plain-2^m", _tpc(n2=16, ext2=0), SHAPE),
    *[(f"alpha[{h}]={v}", _tpc(alpha_host=_sched([0.0] * h + [v] + [0.0] * 8)), SHAPE) for h, v in ((0, -0.5), (3, 16.5), (1, np.nan), (2, np.inf))],
    *[(f"beta[{h}]={v}", _tpc(beta_host=_sched([0.0] * h + [v] + [0.0] * 8)), SHAPE) for h, v in ((0, -0.5), (3, np.inf), (1, np.nan))],
    ("largest-C-fit", _tpc(**{**BIG, "C": 0x7fffffff, "N": 0x3fffffff, "w": 64}), SHAPE),
    ("fit-before-lds", _tpc(**{**BIG, "C": 4, "N": 33, "w": 12, "t0": 5}), SHAPE),
    ("R*C-past-int32", _tpc(R=1 << 30, C=3), SHAPE),
    ("C*n-past-stream", _tpc(C=1 << 23, N=0x3fffffff, w=4, t0=0, llr_out=P, bits_out=P), SHAPE),      # C n = 160 * 2^23 > 0x3fffffff
    ("lds", _tpc(**BIG), LDS), ("lds-256x64", _tpc(**{**BIG, "m2": 6, "n2": 64}), LDS),
    ("shape-before-lds", _tpc(**{**BIG, "K1": 257}), SHAPE),
]


def _call(name, names, d):
    from vae_equalizer_amd import _native as nat
    f = getattr(nat.lib(), name)
    assert len(names) == len(f.argtypes) and list(d) == list(names)
    return f(*d.values())


@pytest.mark.parametrize("case", CHASE_CASES, ids=lambda c: c[0])
def test_chase_bch_refusal_code(case):
    assert _call("vaeq_chase_bch_decode", CHASE_NAMES, case[1]) == case[2]


@pytest.mark.parametrize("case", TPC_CASES, ids=lambda c: c[0])
def test_tpc_bch_refusal_code(case):
    assert _call("vaeq_tpc_bch_decode", TPC_NAMES, case[1]) == case[2]


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_chase_bch_decode(" in header and "int vaeq_tpc_bch_decode(" in header and "int64_t vaeq_tpc_bch_lds_bytes(" in header
    assert {"vaeq_chase_bch_decode", "vaeq_tpc_bch_decode", "vaeq_tpc_bch_lds_bytes"} <= set(nat.EXPORTS)
    assert hasattr(nat.lib(), "vaeq_chase_bch_decode") and hasattr(nat.lib(), "vaeq_tpc_bch_decode")


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_tpc_bch_lds_bytes

    def formula(m1, n1, ext1, m2, n2, ext2):
        cells, waves = n1 * (n2 | 1), 16 if n1 * n2 > 4096 else 4
        return 8 * cells + (cells + 3) // 4 * 4 + 4 * waves * max(n1, n2) + (6 << m1) + (0 if m1 == m2 else 6 << m2)

    assert f(7, 128, 1, 7, 128, 1) == formula(7, 128, 1, 7, 128, 1) == 157568 <= 156 * 1024      # the extended (128, 113)^2 block fits
    assert f(8, 256, 1, 8, 256, 1) == LDS and formula(8, 256, 1, 8, 256, 1) > 160 * 1024          # (256, 239)^2 does not
    assert f(8, 128, 1, 7, 128, 1) == formula(8, 128, 1, 7, 128, 1) == 157568 + 768 + 768        # another field: its own tables, still below
    n2 = next(n for n in range(17, 257) if formula(8, 256, 1, 7, n, 1) > 156 * 1024)             # the first row length above the bound
    assert f(8, 256, 1, 7, n2, 1) == LDS and f(8, 256, 1, 7, n2 - 1, 1) == formula(8, 256, 1, 7, n2 - 1, 1) <= 156 * 1024
    print("256 rows:", n2 - 1, "columns fit with", formula(8, 256, 1, 7, n2 - 1, 1), "bytes;", n2, "need", formula(8, 256, 1, 7, n2, 1))
    for shape in ((4, 10, 1, 4, 16, 1), (4, 15, 0, 5, 32, 1), (5, 32, 1, 5, 32, 1), (7, 65, 1, 6, 64, 1), (8, 256, 1, 5, 17, 1), (8, 200, 0, 8, 17, 0)):
        assert f(*shape) == formula(*shape), shape
    for shape in ((3, 10, 1, 4, 16, 1), (9, 10, 1, 4, 16, 1), (4, 9, 1, 4, 16, 1), (4, 17, 1, 4, 16, 1), (4, 10, 2, 4, 16, 1), (4, 10, 1, 4, 8, 0),
                  (4, 10, 1, 4, 16, 0), (4, 10, 1, 4, 16, -1), (4, 10, 1, 9, 16, 1)):
        assert f(*shape) == SHAPE, shape


def test_codes_and_value_errors():
    from vae_equalizer_amd.engine import (BchCode, EbchCode, ProductCode, StaircaseCode, chase_decode, check_fec, ebch_code, fec_figures, hamming_code,
                                          resolve_inner, resolve_tpc, tpc_decode)
    for m in range(4, 9):                                      # parity(m, 2) = 2 m for these m: 8, 10, 12, 14, 16
        assert BchCode(m, 2).n - BchCode(m, 2).k == 2 * m
        c = ebch_code(m)
        assert (c.m, c.n, c.n_i, c.extended, c.k, c.rate) == (m, 1 << m, (1 << m) - 1, True, (1 << m) - 1 - 2 * m, ((1 << m) - 1 - 2 * m) / (1 << m))
    x32, b15, x10 = ebch_code(5), ebch_code(4, extended=False), EbchCode(4, 10)
    assert (b15.n, b15.n_i, b15.k, b15.extended) == (15, 15, 7, False) and (x10.n, x10.n_i, x10.k) == (10, 9, 1)
    assert (ebch_code(8, n=201).n_i, ebch_code(8, extended=False, n=200).n_i, ebch_code(7).k) == (200, 200, 113)
    for bad in (lambda: EbchCode(3), lambda: EbchCode(9), lambda: EbchCode(4.0), lambda: EbchCode(True), lambda: EbchCode(4, 9), lambda: EbchCode(4, 17),
                lambda: EbchCode(4, 8, extended=False), lambda: EbchCode(4, 16, extended=False), lambda: EbchCode(5, 10.0), lambda: ebch_code(8, n=258)):
        with pytest.raises(ValueError):
            bad()
    code = ProductCode(x10, x32)
    assert code.bch and (code.n, code.k, code.rate, code.col, code.row) == (320, 21, 21 / 320, x10, x32)
    assert not ProductCode(hamming_code(4), hamming_code(4)).bch
    big = ProductCode(ebch_code(7), ebch_code(7))
    assert (big.n, big.k) == (16384, 113 * 113)
    for bad in (lambda: ProductCode(x32, hamming_code(5)), lambda: ProductCode(hamming_code(5), x32), lambda: ProductCode(ebch_code(8), ebch_code(8)),
                lambda: ProductCode(x32, None), lambda: ProductCode(BchCode(5, 2), x32)):
        with pytest.raises(ValueError):                     # mixed kinds are out of scope; (256, 239)^2 passes the LDS bound
            bad()
    prm = resolve_tpc(code)
    assert prm["iters"] == 4 and prm["patterns"] == 4 and prm["payload"] == (1, 21)
    check_fec(dict(code=code))
    check_fec(dict(code=code, t0=3, iters=2, patterns=6, alpha=[0, .5, 1, 1], beta=(1, 1, 1, 1), scale=2.0, clip=64.0))
    for extra in (dict(window=2), dict(max_iter=20), dict(inner=dict(code=x32)), dict(depth=2), dict(payload=(1, 21)), dict(blocks=2), dict(iters=0),
                  dict(patterns=7), dict(alpha=[0, .2]), dict(beta="x"), dict(clip=0)):
        bad = dict(code=code, **extra)
        with pytest.raises(ValueError):
            check_fec(bad)
        with pytest.raises(ValueError):                     # before anything is allocated: the LLRs are never looked at
            fec_figures(None, bad)
    stair = StaircaseCode(BchCode(5, 1, n=24), 3)
    assert resolve_inner(dict(code=x32)) == dict(code=x32, patterns=4, depth=None, payload=21, spread=True)
    check_fec(dict(code=stair, window=2, inner=dict(code=x32, patterns=6, payload=32, depth=2, spread=False)))
    for inner in (dict(code=x32, patterns=7), dict(code=x32, payload=33), dict(code=x32, payload=0), dict(code=x32, depth=0), dict(code=x32, iters=2),
                  dict(code=(32, 21)), dict(code=code), dict(code=x10, patterns=-1)):
        with pytest.raises(ValueError):
            check_fec(dict(code=stair, window=2, inner=inner))
    for bad in (lambda: chase_decode(None, None, (32, 21)), lambda: chase_decode(None, None, code), lambda: tpc_decode(None, None, x32),
                lambda: tpc_decode(None, None, code, payload=(11, 21)), lambda: tpc_decode(None, None, code, patterns=7)):
        with pytest.raises(ValueError):
            bad()

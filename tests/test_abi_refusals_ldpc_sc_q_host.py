"""Which error code vaeq_ldpc_sc_decode_q returns for which refused arguments, in the style of tests/test_abi_refusals_ldpc_sc_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_ldpc_sc_decode's -- empty batch, any NULL pointer
(post, pos_err and pos_iters may be NULL), shape -- with the quantiser's rules where vaeq_ldpc_decode_q puts them: behind the shape rules and in
front of the table's, which come last.  An accepted neighbour of a refused argument set would launch, so it is shown where that needs no device:
the refusal moves on to a rule further down the order."""
import ctypes as C

import numpy as np
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 ms mb nb Z Lc components llr bits W T qbits abits scale num beta iters out post pos_err pos_iters stream".split()


def _comp(ms, mb, nb, Z, **cells):
    d, c = np.arange(ms + 1)[:, None, None], np.arange(nb)[None, None, :]
    s = np.ascontiguousarray(np.broadcast_to((2 ** d * (2 * c + 1)) % Z, (ms + 1, mb, nb)).astype(np.int32))
    for k, v in cells.items():
        dd, l, cc = (int(x) for x in k[1:].split("_"))
        s[dd, l, cc] = v
    return s


def _keep(ms, mb, nb, Z, keep):
    """Component d keeps its first keep[d] blocks in every row."""
    s = _comp(ms, mb, nb, Z)
    for d, k in enumerate(keep):
        s[d, :, k:] = -1
    return s


BAD_TABLE = dict(components=_comp(2, 1, 4, 31, s2_0_3=31))  # refused last: whatever passes every earlier rule still ends as SHAPE without a launch


def _base(ms=2, mb=1, nb=4, Z=31, Lc=12, **over):
    n = Lc * nb * Z
    d = dict(R=1, C=2, N=-(-2 * n // 12) + 7, w=12, t0=7, ms=ms, mb=mb, nb=nb, Z=Z, Lc=Lc, components=_comp(ms, mb, nb, Z), llr=P, bits=P, W=5, T=3,
             qbits=5, abits=7, scale=1.0, num=6, beta=0, iters=10, out=P, post=None, pos_err=None, pos_iters=None,
             stream=None)                                  # would be accepted: the 2 chains end in the last symbol
    d.update(over)
    return d


CASES = [
    ("empty", _base(R=0, components=None, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, ms=0, Z=1, iters=0, W=0, qbits=0, scale=-1.0), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("components", "llr", "bits", "out")],
    ("null-before-shape", _base(out=None, mb=5), NULL), ("null-before-quantiser", _base(bits=None, qbits=9), NULL),
    ("null-before-table", _base(llr=None, **BAD_TABLE), NULL),
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 3), ("N", 0), ("N", 1 << 30), ("N", 254), ("w", 0),
                                                        ("w", 65), ("t0", -1), ("t0", 8), ("iters", 0), ("iters", 101), ("ms", 0), ("mb", 0),
                                                        ("nb", 1), ("Z", 1), ("Lc", 0), ("Lc", 65536), ("W", 2), ("W", 33), ("T", 0), ("T", 6))],
    ("ms=8", _base(ms=8, W=9, components=_comp(8, 1, 4, 31)), SHAPE), ("mb=5", _base(mb=5, components=_comp(2, 5, 4, 31)), SHAPE),
    ("nb=33", _base(nb=33, N=40000, components=_comp(2, 1, 33, 31)), SHAPE),
    ("Z=513", _base(Z=513, N=40000, components=_comp(2, 1, 4, 513)), SHAPE),
    ("R*C-past-int32", _base(R=1 << 30, C=2), SHAPE),
    ("C*Lc-past-int32", _base(C=40000, Lc=65535, nb=2, Z=2, N=(1 << 30) - 1, components=_comp(2, 1, 2, 2)), SHAPE),
    # ms = 1, nb = 9, W = 3: 132 Z bytes; Z = 496 is 65 472 (tests/test_ldpc_sc_q_gpu.py decodes it), Z = 497 is 65 604
    ("state-65604", _base(ms=1, nb=9, Z=497, Lc=4, W=3, T=2, N=4000, components=_comp(1, 1, 9, 497)), SHAPE),
    ("oversize-state", _base(ms=7, mb=4, nb=32, Z=512, W=32, N=1 << 29, components=_comp(7, 4, 32, 512)), SHAPE),
    # the quantiser's rules: each refused value, then its accepted neighbours in front of a table that is refused (no launch either way)
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("qbits", 1), ("qbits", 9), ("qbits", 0), ("abits", 4), ("abits", 16), ("scale", 0.0),
                                                        ("scale", -1.0), ("scale", float("inf")), ("scale", float("nan")), ("num", 0), ("num", 9),
                                                        ("beta", -1), ("beta", 128))],
    ("abits-below-qbits", _base(qbits=8, abits=7), SHAPE),
    *[(f"accepted-{k}={v}-then-table", _base(**{k: v}, **BAD_TABLE), SHAPE) for k, v in (("abits", 5), ("abits", 15), ("scale", 1e-30), ("scale", 1e30),
                                                                                         ("num", 1), ("num", 8), ("beta", 127))],
    ("accepted-qbits=2-then-table", _base(qbits=2, abits=2, **BAD_TABLE), SHAPE), ("accepted-qbits=8-then-table", _base(qbits=8, abits=8, **BAD_TABLE), SHAPE),
    ("shift=Z", _base(**BAD_TABLE), SHAPE), ("shift=-2", _base(components=_comp(2, 1, 4, 31, s1_0_0=-2)), SHAPE),
    ("row-weight-33", _base(nb=11, N=4000, components=_comp(2, 1, 11, 31)), SHAPE),
    ("head-row-weight-1", _base(components=_keep(2, 1, 4, 31, (1, 4, 4))), SHAPE),          # row block 0 has component 0 alone
    ("tail-row-weight-1", _base(components=_keep(2, 1, 4, 31, (4, 4, 1))), SHAPE),          # the last row block has component ms alone
    ("row-weight-0", _base(components=_keep(2, 1, 4, 31, (0, 0, 0))), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_ldpc_sc_decode_q
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    keep = d["components"]                                  # (alive during the call)
    args = [keep.ctypes.data_as(C.c_void_p) if k == "components" and keep is not None else v for k, v in d.items()]
    return f(*args)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f, g = nat.lib().vaeq_ldpc_sc_q_lds_bytes, nat.lib().vaeq_ldpc_sc_lds_bytes
    assert f(2, 1, 4, 31, 5) == 2 * 7 * 124 + 7 * 124 + 8 * 5 * 31                 # a ring of W + ms column blocks: L as int16, the TX bits as bytes; 8 bytes per check of W row blocks
    assert f(1, 2, 3, 7, 2) == 128 + 64 + 8 * 2 * 14                               # 63 values: 126 and 63 bytes, each padded to whole words
    assert f(3, 1, 6, 101, 8) == 26464 and g(3, 1, 6, 101, 8) == 46260             # the probe's shape, against the float window decoder's
    assert f(1, 1, 9, 496, 3) == 65472 <= 64 * 1024 < f(1, 1, 9, 497, 3) == 65604   # the two sides of the limit
    assert f(1, 1, 6, 391, 3) < 64 * 1024 < g(1, 1, 6, 391, 3)                     # a shape the float window decoder refuses
    assert f(7, 4, 32, 512, 32) > 64 * 1024
    for bad in ((0, 1, 4, 31, 5), (8, 1, 4, 31, 9), (2, 0, 4, 31, 5), (2, 5, 4, 31, 5), (2, 1, 1, 31, 5), (2, 1, 33, 31, 5), (2, 1, 4, 1, 5),
                (2, 1, 4, 513, 5), (2, 1, 4, 31, 2), (2, 1, 4, 31, 33)):
        assert f(*bad) == SHAPE


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_ldpc_sc_decode_q(" in header and "int64_t vaeq_ldpc_sc_q_lds_bytes(" in header
    for fn in ("vaeq_ldpc_sc_decode_q", "vaeq_ldpc_sc_q_lds_bytes"):
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)
    assert "vaeq_ldpc_sc.hip" in nat.SOURCES and "vaeq_ldpc_rule.h" in nat.HEADERS and "vaeq_ldpc_sc.h" in nat.HEADERS   # (the float window decoder's file holds it)

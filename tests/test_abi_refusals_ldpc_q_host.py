"""Which error code vaeq_ldpc_decode_q returns for which refused arguments, in the style of tests/test_abi_refusals_ldpc_host.py: every
argument set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_ldpc_decode's -- empty batch, any NULL
pointer (post alone may be NULL), shape -- with the fixed-point decoder's own rules (qbits, abits, scale, num, beta, depth) among the shape
rules and the table's rules last.  The base call carries a table with a shift equal to Z, so that it never launches; the cases that must be
refused for another reason carry a good table."""
import ctypes as C
import math

import numpy as np
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 depth mb nb Z shifts llr bits qbits abits scale num beta max_iter out post stream".split()
BAD_TABLE = "s2_5"                                         # a shift equal to Z in the last block: the check after every shape rule


def _table(mb, nb, Z, **cells):
    s = (np.outer(np.arange(mb), np.arange(nb)) % Z).astype(np.int32)
    for k, v in cells.items():
        l, c = (int(x) for x in k[1:].split("_"))
        s[l, c] = v
    return s


def _holes(mb, nb, Z, keep):
    """Every block row keeps its first `keep` blocks."""
    s = _table(mb, nb, Z)
    s[:, keep:] = -1
    return s


def _base(mb=3, nb=6, Z=7, **over):
    n = nb * Z
    d = dict(R=1, C=5, N=-(-5 * n // 12) + 11, w=12, t0=11, depth=0, mb=mb, nb=nb, Z=Z, shifts=_table(mb, nb, Z, **({BAD_TABLE: Z} if mb > 2 and nb > 5 else {})),
             llr=P, bits=P, qbits=5, abits=7, scale=1.0, num=6, beta=0, max_iter=20, out=P, post=None, stream=None)
    d.update(over)                                         # passes every shape rule (the 5 bit-packed codewords end in the last symbol), then is
    return d                                               # refused for its table: no launch


GOOD = dict(shifts=_table(3, 6, 7))

CASES = [
    ("empty", _base(R=0, shifts=None, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, mb=0, Z=1, max_iter=0, qbits=0, depth=-1), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("shifts", "llr", "bits", "out")],
    ("null-before-shape", _base(out=None, mb=9), NULL), ("null-before-table", _base(llr=None, shifts=_table(3, 6, 7, s0_0=7)), NULL),
    ("null-before-qbits", _base(bits=None, qbits=9), NULL), ("null-before-depth", _base(llr=None, depth=-1), NULL),
    ("null-before-scale", _base(out=None, scale=0.0), NULL),
    # the float decoder's refusals, carried over (depth 0: its bit-packed fit rule)
    *[(f"{k}={v}", _base(**{k: v}, **GOOD), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 6), ("N", 0), ("N", 1 << 30), ("N", 28), ("w", 0),
                                                                ("w", 65), ("t0", -1), ("t0", 12), ("max_iter", 0), ("max_iter", 101), ("mb", 0),
                                                                ("nb", 1), ("Z", 1))],
    ("mb=9", _base(mb=9, shifts=_table(9, 6, 7)), SHAPE), ("nb=65", _base(nb=65, Z=67, N=4000, shifts=_table(3, 65, 67)), SHAPE),
    ("Z=513", _base(nb=2, Z=513, N=4000, shifts=_table(3, 2, 513)), SHAPE),
    ("R*C-past-int32", _base(R=1 << 29, C=5, **GOOD), SHAPE),
    ("shift=Z", _base(shifts=_table(3, 6, 7, s2_5=7)), SHAPE), ("shift=-2", _base(shifts=_table(3, 6, 7, s1_0=-2)), SHAPE),
    ("row-weight-1", _base(shifts=_holes(3, 6, 7, 1)), SHAPE), ("row-weight-0", _base(shifts=_holes(3, 6, 7, 0)), SHAPE),
    ("row-weight-33", _base(mb=2, nb=33, Z=37, N=4000, shifts=_table(2, 33, 37)), SHAPE),
    ("oversize-state", _base(mb=8, nb=64, Z=512, N=40000, shifts=_table(8, 64, 512)), SHAPE),
    # nb = 64 next to the 64 KiB: 3 n + 8 m = 208 Z at mb = 2, so Z = 315 is 65 520 bytes (tests/test_ldpc_envelope_gpu.py decodes it) and Z = 316 is
    # 65 728; the table is good (32 blocks per row), bit-packed and behind the interleaver
    ("state-65728-at-nb=64", _base(mb=2, nb=64, Z=316, N=9000, shifts=_holes(2, 64, 316, 32)), SHAPE),
    ("state-65728-at-nb=64-depth=5", _base(mb=2, nb=64, Z=316, N=9000, depth=5, shifts=_holes(2, 64, 316, 32)), SHAPE),
    ("row-weight-64-at-nb=64", _base(mb=2, nb=64, Z=315, N=9000, shifts=_table(2, 64, 315)), SHAPE),
    # the interleaver's fit rule at depth >= 1: 5 codewords of S = 4 symbols need 20 symbols behind t0, the base N has 18
    ("depth=2-symbol-aligned-fit", _base(depth=2, **GOOD), SHAPE), ("depth=1-symbol-aligned-fit", _base(depth=1, N=11 + 19, **GOOD), SHAPE),
    # one case per rule of the fixed-point decoder
    *[(f"{k}={v}", _base(**{k: v}, **GOOD), SHAPE)
      for k, v in (("qbits", 1), ("qbits", 9), ("qbits", 0), ("abits", 4), ("abits", 16), ("scale", 0.0), ("scale", -1.0), ("scale", math.inf),
                   ("scale", math.nan), ("num", 0), ("num", 9), ("beta", -1), ("beta", 128), ("depth", -1), ("depth", 6))],
    ("abits-below-qbits=8", _base(qbits=8, abits=7, **GOOD), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_ldpc_decode_q
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    keep = d["shifts"]                                      # (alive during the call)
    args = [keep.ctypes.data_as(C.c_void_p) if k == "shifts" and keep is not None else v for k, v in d.items()]
    return f(*args)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


@pytest.mark.parametrize("over", [dict(), dict(qbits=2, abits=2), dict(qbits=8, abits=15), dict(qbits=8, abits=8), dict(num=1, beta=127), dict(num=8),
                                  dict(scale=1e-30), dict(scale=3e38), dict(depth=1, N=11 + 20), dict(depth=5, N=11 + 20)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "base")
def test_the_edges_of_the_ranges_pass_every_shape_rule(over):
    """The edges of the new ranges, as far as a call without a device can take them: with the base's bad table the call ends at the check behind
    all shape rules (a good table would launch on pointers that are none); that these values are accepted and decoded is
    tests/test_ldpc_q_gpu.py's to show.  Empty, the same arguments are VAEQ_OK."""
    assert _call(_base(**over)) == SHAPE                                          # the table's refusal, by construction
    assert _call(_base(**over, R=0)) == OK
    assert _call(_base(**{**over, "max_iter": 0}, **GOOD)) == SHAPE


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f, g = nat.lib().vaeq_ldpc_q_lds_bytes, nat.lib().vaeq_ldpc_lds_bytes
    assert f(4, 24, 211) == 2 * 5064 + 5064 + 8 * 844 == 21944                    # L as int16, the TX bits as bytes, two dwords per check
    assert f(3, 6, 7) == 84 + 44 + 8 * 21                                         # (the 42 bytes padded to whole words)
    assert f(1, 3, 7) == 44 + 24 + 8 * 7                                          # (the 42 bytes of L and the 21 of the bits, both padded)
    assert f(3, 32, 512) == 61440 <= 64 * 1024 < g(3, 32, 512)                    # a code the float decoder must refuse
    assert f(8, 64, 512) > 64 * 1024
    assert f(2, 64, 315) == 208 * 315 == 65520 <= 64 * 1024 < f(2, 64, 316) == 65728   # the two sides of the limit at the most block columns
    assert g(2, 64, 186) == 65472 and f(2, 64, 186) == 208 * 186
    for bad in ((0, 6, 7), (9, 6, 7), (3, 1, 7), (3, 65, 7), (3, 6, 1), (3, 6, 513)):
        assert f(*bad) == SHAPE


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_ldpc_decode_q(" in header and "int64_t vaeq_ldpc_q_lds_bytes(" in header
    assert "int32_t qbits, int32_t abits, float scale, int32_t num" in header and "int16_t *post" in header
    for fn in ("vaeq_ldpc_decode_q", "vaeq_ldpc_q_lds_bytes"):
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)
    assert "vaeq_ldpc.hip" in nat.SOURCES and "vaeq_ldpc_rule.h" in nat.HEADERS and "vaeq_ldpc.h" in nat.HEADERS    # (the float decoder's file holds it)
    for fn in ("vaeq_ldpc_decode", "vaeq_ldpc_decode_il", "vaeq_ldpc_lds_bytes"):  # the float entry points stay beside it
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)

"""Which error code vaeq_ldpc_decode_il returns for which refused arguments, in the pattern of tests/test_abi_refusals_ldpc_host.py: every
argument set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_ldpc_decode's -- empty batch, any
NULL pointer (post alone may be NULL), shape -- with the interleaver's two rules: 1 <= depth <= C, and the symbol-aligned fit t0 + C S <= N with
S = ceil(n / w).  The base call carries a table with a shift equal to Z, the one refusal behind every shape rule, so that it never launches;
the cases that must be refused for another reason carry a good table."""
import ctypes as C

import numpy as np
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 depth mb nb Z shifts llr bits alpha max_iter out post stream".split()
BAD_TABLE = "s2_5"                                         # a shift equal to Z in the last block: the check after every shape rule


def _table(mb, nb, Z, **cells):
    s = (np.outer(np.arange(mb), np.arange(nb)) % Z).astype(np.int32)
    for k, v in cells.items():
        l, c = (int(x) for x in k[1:].split("_"))
        s[l, c] = v
    return s


def _base(mb=3, nb=6, Z=7, **over):
    n = nb * Z
    d = dict(R=1, C=5, N=11 + 5 * -(-n // 12), w=12, t0=11, depth=2, mb=mb, nb=nb, Z=Z, shifts=_table(mb, nb, Z, **({BAD_TABLE: Z} if mb > 2 and nb > 5 else {})), llr=P, bits=P,
             alpha=0.75, max_iter=20, out=P, post=None, stream=None)   # passes every shape rule (5 codewords of S = 4 symbols end in the last symbol),
    d.update(over)                                                      # then is refused for its table: no launch
    return d


CASES = [
    ("empty", _base(R=0, shifts=None, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, mb=0, Z=1, max_iter=0, depth=0), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("shifts", "llr", "bits", "out")],
    ("null-before-shape", _base(out=None, mb=9), NULL), ("null-before-depth", _base(llr=None, depth=0), NULL),
    ("null-before-fit", _base(bits=None, N=30), NULL),
    *[(f"{k}={v}", _base(**{k: v}, shifts=_table(3, 6, 7)), SHAPE)
      for k, v in (("depth", 0), ("depth", -1), ("depth", 6), ("R", -1), ("C", 0), ("C", 1), ("C", 6), ("N", 0), ("N", 1 << 30), ("N", 30), ("w", 0),
                   ("w", 65), ("t0", -1), ("t0", 12), ("max_iter", 0), ("max_iter", 101), ("mb", 0), ("nb", 1), ("Z", 1))],
    ("mb=9", _base(mb=9, shifts=_table(9, 6, 7)), SHAPE), ("Z=513", _base(nb=2, Z=513, N=4000, shifts=_table(3, 2, 513)), SHAPE),
    ("R*C-past-int32", _base(R=1 << 29, C=5, shifts=_table(3, 6, 7)), SHAPE),
    ("oversize-state", _base(mb=8, nb=32, Z=512, N=40000, shifts=_table(8, 32, 512)), SHAPE),
]


def _call(d, name="vaeq_ldpc_decode_il"):
    from vae_equalizer_amd import _native as nat
    f = getattr(nat.lib(), name)
    d = dict(d) if name == "vaeq_ldpc_decode_il" else {k: v for k, v in d.items() if k != "depth"}
    assert len(d) == len(f.argtypes) and [k for k in NAMES if k in d] == list(d)
    keep = d["shifts"]                                      # (alive during the call)
    args = [keep.ctypes.data_as(C.c_void_p) if k == "shifts" and keep is not None else v for k, v in d.items()]
    return f(*args)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_the_fit_rule_is_the_symbol_aligned_one():
    """N = t0 + C S - 1 is refused with a good table.  N = t0 + C S with a good table would launch (on pointers that are none), so here it
    is only taken as far as the check behind all shape rules, the table's; that it is accepted and decoded is tests/test_ldpc_il_gpu.py's to
    show, where every case has exactly N = t0 + C S."""
    assert _call(_base(N=11 + 20 - 1, shifts=_table(3, 6, 7))) == SHAPE
    assert _call(_base(N=11 + 20)) == SHAPE
    assert _call(_base(N=11 + 20 - 1, R=0, shifts=_table(3, 6, 7))) == OK


def test_bit_packed_fit_is_not_enough():
    """n = 42, w = 12, C = 5, N = t0 + 18: 210 bits fill 17.5 symbols, so vaeq_ldpc_decode's fit rule holds; symbol-aligned the codewords need
    5 x 4 = 20 symbols, and vaeq_ldpc_decode_il refuses the call."""
    assert 11 * 12 + 5 * 42 <= (11 + 18) * 12 and 11 + 5 * 4 > 11 + 18
    assert _call(_base(N=11 + 18, shifts=_table(3, 6, 7))) == SHAPE
    assert _call(_base(N=11 + 17, shifts=_table(3, 6, 7)), "vaeq_ldpc_decode") == SHAPE   # the old rule's own edge: 17 symbols hold 204 bits


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_ldpc_decode_il(" in header and "int64_t t0, int32_t depth, int32_t mb" in header
    assert "vaeq_ldpc_decode_il" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_ldpc_decode_il")
    assert "int vaeq_ldpc_decode(" in header and "vaeq_ldpc_decode" in nat.EXPORTS    # the old entry point stays beside it

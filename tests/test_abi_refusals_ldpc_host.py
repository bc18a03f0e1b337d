"""Which error code vaeq_ldpc_decode returns for which refused arguments, in the style of tests/test_abi_refusals_llr_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is vaeq_dp_epilogue_llr's -- empty batch, any NULL
pointer (post alone may be NULL), shape; the table of shifts is host memory and is validated on every call."""
import ctypes as C

import numpy as np
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R C N w t0 mb nb Z shifts llr bits alpha max_iter out post stream".split()


def _table(mb, nb, Z, **cells):
    s = (np.outer(np.arange(mb), np.arange(nb)) % Z).astype(np.int32)
    for k, v in cells.items():
        l, c = (int(x) for x in k[1:].split("_"))
        s[l, c] = v
    return s


def _base(mb=3, nb=6, Z=7, **over):
    n = nb * Z
    d = dict(R=1, C=5, N=-(-5 * n // 12) + 11, w=12, t0=11, mb=mb, nb=nb, Z=Z, shifts=_table(mb, nb, Z), llr=P, bits=P, alpha=0.75, max_iter=20,
             out=P, post=None, stream=None)                # would be accepted: the 5 codewords end in the last symbol
    d.update(over)
    return d


def _holes(mb, nb, Z, keep):
    """Every block row keeps its first `keep` blocks."""
    s = _table(mb, nb, Z)
    s[:, keep:] = -1
    return s


CASES = [
    ("empty", _base(R=0, shifts=None, llr=None, bits=None, out=None), OK),
    ("empty-bad-shape", _base(R=0, mb=0, Z=1, max_iter=0), OK),
    *[(f"null-{k}", _base(**{k: None}), NULL) for k in ("shifts", "llr", "bits", "out")],
    ("null-before-shape", _base(out=None, mb=9), NULL), ("null-before-table", _base(llr=None, shifts=_table(3, 6, 7, s0_0=7)), NULL),
    *[(f"{k}={v}", _base(**{k: v}), SHAPE) for k, v in (("R", -1), ("C", 0), ("C", -1), ("C", 6), ("N", 0), ("N", 1 << 30), ("N", 28), ("w", 0),
                                                        ("w", 65), ("t0", -1), ("t0", 12), ("max_iter", 0), ("max_iter", 101), ("mb", 0),
                                                        ("nb", 1), ("Z", 1))],
    ("mb=9", _base(mb=9, shifts=_table(9, 6, 7)), SHAPE), ("nb=65", _base(nb=65, Z=67, N=4000, shifts=_table(3, 65, 67)), SHAPE),
    ("Z=513", _base(nb=2, Z=513, N=4000, shifts=_table(3, 2, 513)), SHAPE),
    ("R*C-past-int32", _base(R=1 << 29, C=5), SHAPE),
    ("shift=Z", _base(shifts=_table(3, 6, 7, s2_5=7)), SHAPE), ("shift=-2", _base(shifts=_table(3, 6, 7, s1_0=-2)), SHAPE),
    ("row-weight-1", _base(shifts=_holes(3, 6, 7, 1)), SHAPE), ("row-weight-0", _base(shifts=_holes(3, 6, 7, 0)), SHAPE),
    ("row-weight-33", _base(mb=2, nb=33, Z=37, N=4000, shifts=_table(2, 33, 37)), SHAPE),
    ("oversize-state", _base(mb=8, nb=32, Z=512, N=40000, shifts=_table(8, 32, 512)), SHAPE),
    # nb = 64 next to the 64 KiB: Z = 186 is 65 472 bytes (tests/test_ldpc_envelope_gpu.py decodes it), Z = 187 is 65 824; the table is good (32 blocks per row)
    ("state-65824-at-nb=64", _base(mb=2, nb=64, Z=187, N=5000, shifts=_holes(2, 64, 187, 32)), SHAPE),
    ("row-weight-64-at-nb=64", _base(mb=2, nb=64, Z=186, N=5000, shifts=_table(2, 64, 186)), SHAPE),
]


def _call(d):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_ldpc_decode
    assert len(NAMES) == len(f.argtypes) and list(d) == NAMES
    keep = d["shifts"]                                      # (alive during the call)
    args = [keep.ctypes.data_as(C.c_void_p) if k == "shifts" and keep is not None else v for k, v in d.items()]
    return f(*args)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    assert _call(case[1]) == case[2]


def test_lds_bytes():
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_ldpc_lds_bytes
    assert f(4, 24, 211) == 4 * 5064 + 5064 + 16 * 844                            # L, the TX bits as bytes, 16 bytes per check
    assert f(3, 6, 7) == 4 * 42 + 44 + 16 * 21                                    # (the bytes padded to whole words)
    assert f(8, 32, 512) > 64 * 1024 >= f(2, 8, 512)
    assert f(2, 64, 186) == 65472 <= 64 * 1024 < f(2, 64, 187) == 65824            # the two sides of the limit at the most block columns
    for bad in ((0, 6, 7), (9, 6, 7), (3, 1, 7), (3, 65, 7), (3, 6, 1), (3, 6, 513)):
        assert f(*bad) == SHAPE


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_ldpc_decode(" in header and "int64_t vaeq_ldpc_lds_bytes(" in header
    for fn in ("vaeq_ldpc_decode", "vaeq_ldpc_lds_bytes"):
        assert fn in nat.EXPORTS and hasattr(nat.lib(), fn)
    assert "vaeq_ldpc.hip" in nat.SOURCES

"""Which error code vaeq_cma_epilogue_info returns for which refused arguments, in the style of tests/test_abi_refusals_info_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is the established one -- empty batch, NULL, shape,
n_lev dispatch."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R N n_lev y tx amp P var nu_sc shift_c r_c shift_q r_q info counts stream".split()
POINTERS = NAMES[3:15]
BASE = (1, 4000, 4) + (P,) * 12 + (None,)                  # would be accepted

CASES = [
    ("empty", dict(R=0, **{k: None for k in POINTERS}), OK),
    ("empty-bad-shape", dict(R=0, n_lev=3, N=1), OK),
    *[(f"null-{k}", {k: None}, NULL) for k in POINTERS],
    ("null-before-shape", dict(P=None, n_lev=3), NULL), ("null-before-shape-N", dict(r_q=None, N=10), NULL),
    ("null-before-shape-R", dict(counts=None, R=-1), NULL),
    *[(f"{k}={v}", {k: v}, SHAPE) for k, v in (("R", -1), ("N", 42), ("N", 0), ("N", (1 << 30)), ("n_lev", 3), ("n_lev", 16), ("n_lev", 0))],
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    _, change, expected = case
    f = nat.lib().vaeq_cma_epilogue_info
    assert len(NAMES) == len(BASE) == len(f.argtypes)
    args = list(BASE)
    for k, v in change.items():
        args[NAMES.index(k)] = v
    assert f(*args) == expected


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    assert "vaeq_cma_epilogue_info" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_cma_epilogue_info")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    assert "int vaeq_cma_epilogue_info(int32_t R, int64_t N, int32_t n_lev, const float *y," in header

"""Which error code vaeq_dp_epilogue_info returns for which refused arguments, in the style of tests/test_abi_refusals_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is the established one -- empty batch, NULL, shape,
n_lev dispatch -- with one rule of its own: exactly one of q and y is given (both or neither is a NULL refusal, reported before any shape)."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R N n_lev batch_len q y tx amp P var nu_sc shift rflag info counts stream".split()
Q_MODE = (1, 4000, 4, 0, P, None, P, P, P, None, None, P, P, P, P, None)       # would be accepted: var / nu_sc belong to the demapper of y-mode
Y_MODE = (1, 4000, 4, 0, None, P, P, P, P, P, P, P, P, P, P, None)

CASES = [
    ("empty", Q_MODE, dict(R=0, q=None, tx=None, amp=None, P=None, shift=None, rflag=None, info=None, counts=None), OK),
    ("empty-bad-shape", Q_MODE, dict(R=0, n_lev=3, N=1), OK),
    ("both", Q_MODE, dict(y=P, var=P, nu_sc=P), NULL), ("neither", Q_MODE, dict(q=None), NULL),
    ("both-before-shape", Y_MODE, dict(q=P, n_lev=3), NULL), ("neither-before-shape", Y_MODE, dict(y=None, N=10), NULL),
    *[(f"q-null-{k}", Q_MODE, {k: None}, NULL) for k in ("tx", "amp", "P", "shift", "rflag", "info", "counts")],
    *[(f"y-null-{k}", Y_MODE, {k: None}, NULL) for k in ("tx", "P", "var", "nu_sc", "counts")],
    ("null-before-shape", Q_MODE, dict(P=None, n_lev=3), NULL), ("null-before-shape-y", Y_MODE, dict(var=None, batch_len=7), NULL),
    *[(f"q-{k}={v}", Q_MODE, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("R", -1), ("N", 42), ("N", 1 << 30), ("batch_len", -1),
                                                         ("batch_len", 7))],
    *[(f"y-{k}={v}", Y_MODE, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("N", 10), ("batch_len", 7))],
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    _, base, change, expected = case
    f = nat.lib().vaeq_dp_epilogue_info
    assert len(NAMES) == len(base) == len(f.argtypes)
    args = list(base)
    for k, v in change.items():
        args[NAMES.index(k)] = v
    assert f(*args) == expected


def test_declared_and_exported():
    from vae_equalizer_amd import _native as nat
    assert "vaeq_dp_epilogue_info" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_dp_epilogue_info")

"""Which error code vaeq_dp_epilogue_llr and vaeq_awgn_llr return for which refused arguments, in the style of
tests/test_abi_refusals_info_host.py: every argument set below is refused on the host before any HIP call, so no device is needed.  The order
is vaeq_dp_epilogue_info's resp. vaeq_awgn_info's -- empty batch, exactly one of q and y (both or neither is a NULL refusal, reported before
any shape), any other NULL pointer, shape, n_lev dispatch."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

DP_NAMES = "R N n_lev batch_len q y amp var nu_sc shift rflag hyp llr stream".split()
DP_Q = (1, 4000, 4, 0, P, None, P, None, None, P, P, P, P, None)               # would be accepted: var / nu_sc belong to the demapper of y-mode
DP_Y = (1, 4000, 4, 0, None, P, P, P, P, P, P, P, P, None)

DP_CASES = [
    ("empty", DP_Q, dict(R=0, q=None, amp=None, shift=None, rflag=None, hyp=None, llr=None), OK),
    ("empty-bad-shape", DP_Q, dict(R=0, n_lev=3, N=1), OK),
    ("both", DP_Q, dict(y=P, var=P, nu_sc=P), NULL), ("neither", DP_Q, dict(q=None), NULL),
    ("both-before-shape", DP_Y, dict(q=P, n_lev=3), NULL), ("neither-before-shape", DP_Y, dict(y=None, N=10), NULL),
    *[(f"q-null-{k}", DP_Q, {k: None}, NULL) for k in ("amp", "shift", "rflag", "hyp", "llr")],
    *[(f"y-null-{k}", DP_Y, {k: None}, NULL) for k in ("amp", "var", "nu_sc", "hyp", "llr")],
    ("null-before-shape", DP_Q, dict(hyp=None, n_lev=3), NULL), ("null-before-shape-y", DP_Y, dict(var=None, batch_len=7), NULL),
    *[(f"q-{k}={v}", DP_Q, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("R", -1), ("N", 42), ("N", 1 << 30), ("batch_len", -1),
                                                       ("batch_len", 7))],
    *[(f"y-{k}={v}", DP_Y, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("N", 10), ("batch_len", 7))],
]

AWGN_NAMES = "R N n_lev q y amp amp_mean var shift hyp llr stream".split()
AWGN_Q = (1, 4000, 4, P, None, P, None, None, P, P, P, None)                   # would be accepted: amp_mean / var belong to the demapper of y-mode
AWGN_Y = (1, 4000, 4, None, P, P, P, P, P, P, P, None)

AWGN_CASES = [
    ("empty", AWGN_Q, dict(R=0, q=None, amp=None, shift=None, hyp=None, llr=None), OK),
    ("empty-bad-shape", AWGN_Q, dict(R=0, n_lev=3, N=0), OK),
    ("both", AWGN_Q, dict(y=P, amp_mean=P, var=P), NULL), ("neither", AWGN_Q, dict(q=None), NULL),
    ("both-before-shape", AWGN_Y, dict(q=P, n_lev=3), NULL), ("neither-before-shape", AWGN_Y, dict(y=None, N=0), NULL),
    *[(f"q-null-{k}", AWGN_Q, {k: None}, NULL) for k in ("amp", "shift", "hyp", "llr")],
    *[(f"y-null-{k}", AWGN_Y, {k: None}, NULL) for k in ("amp", "amp_mean", "var", "hyp", "llr")],
    ("null-before-shape", AWGN_Q, dict(llr=None, n_lev=3), NULL), ("null-before-shape-y", AWGN_Y, dict(var=None, N=0), NULL),
    *[(f"q-{k}={v}", AWGN_Q, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("R", -1), ("N", 0), ("N", -5), ("N", 1 << 30))],
    *[(f"y-{k}={v}", AWGN_Y, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("N", 0))],
]


def _check(fn, names, case):
    from vae_equalizer_amd import _native as nat
    _, base, change, expected = case
    f = getattr(nat.lib(), fn)
    assert len(names) == len(base) == len(f.argtypes)
    args = list(base)
    for k, v in change.items():
        args[names.index(k)] = v
    assert f(*args) == expected


@pytest.mark.parametrize("case", DP_CASES, ids=lambda c: c[0])
def test_dp_refusal_code(case):
    _check("vaeq_dp_epilogue_llr", DP_NAMES, case)


@pytest.mark.parametrize("case", AWGN_CASES, ids=lambda c: c[0])
def test_awgn_refusal_code(case):
    _check("vaeq_awgn_llr", AWGN_NAMES, case)


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    for fn in ("vaeq_dp_epilogue_llr", "vaeq_awgn_llr"):
        assert f"int {fn}(" in header and fn in nat.EXPORTS and hasattr(nat.lib(), fn)

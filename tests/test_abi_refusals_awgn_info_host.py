"""Which error code vaeq_awgn_info returns for which refused arguments, in the style of tests/test_abi_refusals_info_host.py: every argument
set below is refused on the host before any HIP call, so no device is needed.  The order is the established one -- empty batch, NULL, shape,
n_lev dispatch -- with the rule of the info kernels: exactly one of q and y is given (both or neither is a NULL refusal, reported before any
shape)."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

NAMES = "R N n_lev q y data amp P amp_mean var shift info counts stream".split()
Q_MODE = (1, 4000, 4, P, None, P, P, P, None, None, P, P, P, None)             # would be accepted: amp_mean / var belong to the demapper of y-mode
Y_MODE = (1, 4000, 4, None, P, P, P, P, P, P, P, P, P, None)

CASES = [
    ("empty", Q_MODE, dict(R=0, q=None, data=None, amp=None, P=None, shift=None, info=None, counts=None), OK),
    ("empty-bad-shape", Q_MODE, dict(R=0, n_lev=3, N=0), OK),
    ("empty-null-bad-shape", Y_MODE, dict(R=0, y=None, data=None, amp=None, P=None, amp_mean=None, var=None, shift=None, info=None, counts=None,
                                          n_lev=5, N=-1), OK),
    ("both", Q_MODE, dict(y=P, amp_mean=P, var=P), NULL), ("neither", Q_MODE, dict(q=None), NULL),
    ("both-before-shape", Y_MODE, dict(q=P, n_lev=3), NULL), ("neither-before-shape", Y_MODE, dict(y=None, N=0), NULL),
    *[(f"q-null-{k}", Q_MODE, {k: None}, NULL) for k in ("data", "amp", "P", "shift", "info", "counts")],
    *[(f"y-null-{k}", Y_MODE, {k: None}, NULL) for k in ("data", "amp", "P", "amp_mean", "var", "shift", "info", "counts")],
    ("null-before-shape", Q_MODE, dict(P=None, n_lev=3), NULL), ("null-before-shape-y", Y_MODE, dict(var=None, N=0), NULL),
    *[(f"q-{k}={v}", Q_MODE, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("n_lev", 0), ("R", -1), ("N", 0), ("N", -5), ("N", 1 << 30))],
    *[(f"y-{k}={v}", Y_MODE, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("N", 0), ("N", 1 << 30), ("R", -2))],
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    _, base, change, expected = case
    f = nat.lib().vaeq_awgn_info
    assert len(NAMES) == len(base) == len(f.argtypes)
    args = list(base)
    for k, v in change.items():
        args[NAMES.index(k)] = v
    assert f(*args) == expected


V_NAMES = "R N sps M n_lev n_shift x W amp amp_mean var data y_ws ser shift stream".split()
V_BASE = (1, 60, 2, 25, 4, 21, P, P, P, P, P, P, P, P, P, None)              # would be accepted: a row under the 64 symbols of vaeq_awgn_validate
V_CASES = [
    ("empty", dict(R=0, x=None, W=None, ser=None, N=5), OK),
    *[(f"null-{k}", {k: None}, NULL) for k in ("x", "W", "amp", "amp_mean", "var", "data", "y_ws", "ser")],
    ("null-before-shape", dict(x=None, N=64), NULL),
    *[(f"{k}={v}", {k: v}, SHAPE) for k, v in (("N", 64), ("N", 2000), ("N", 32), ("N", 0), ("R", -1), ("M", 24), ("sps", 0), ("n_shift", 0), ("n_shift", 33),
                                               ("n_lev", 3))],
    ("N=38-n_shift=32", dict(N=38, n_shift=32), SHAPE),                        # 23 + 32 // 2 = 39
]


@pytest.mark.parametrize("case", V_CASES, ids=lambda c: c[0])
def test_validate_short_refusal_code(case):
    """vaeq_awgn_validate_short refuses what vaeq_awgn_validate refuses, and every N outside 23 + n_shift / 2 <= N < 64."""
    from vae_equalizer_amd import _native as nat
    _, change, expected = case
    f = nat.lib().vaeq_awgn_validate_short
    assert len(V_NAMES) == len(V_BASE) == len(f.argtypes)
    args = list(V_BASE)
    for k, v in change.items():
        args[V_NAMES.index(k)] = v
    assert f(*args) == expected
    assert "vaeq_awgn_validate_short" in nat.EXPORTS


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    assert "vaeq_awgn_info" in nat.EXPORTS and hasattr(nat.lib(), "vaeq_awgn_info")
    assert "vaeq_awgn_info.hip" in nat.SOURCES and "vaeq_info.h" in nat.HEADERS
    with open(os.path.join(nat._ROOT, "include", "vaeq.h")) as fh:
        assert "int vaeq_awgn_info(int32_t R, int64_t N, int32_t n_lev, const float *q, const float *y, const void *data_f16" in fh.read()

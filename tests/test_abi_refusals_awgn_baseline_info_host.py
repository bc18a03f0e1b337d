"""Which error code vaeq_awgn_track_info and vaeq_awgn_dfe_soft return for which refused arguments, in the style of
tests/test_abi_refusals_awgn_info_host.py: every argument set below is refused on the host before any HIP call, so no device is needed.  The
order is the established one -- empty batch, NULL, shape, n_lev dispatch."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

T_NAMES = "R Nz Nd n_lev edge interleaved z data amp P var shift info counts stream".split()
T_BASE = (1, 4001, 4000, 4, 31, 1, P, P, P, P, P, P, P, P, None)               # would be accepted: an LMMSE output against its data
T_PTRS = ("z", "data", "amp", "P", "var", "shift", "info", "counts")
T_CASES = [
    ("empty", dict(R=0, **{k: None for k in T_PTRS}), OK),
    ("empty-bad-shape", dict(R=0, n_lev=3, Nd=0, Nz=7, edge=-1, interleaved=2), OK),
    *[(f"null-{k}", {k: None}, NULL) for k in T_PTRS],
    ("null-before-shape", dict(P=None, n_lev=3), NULL), ("null-before-shape-Nz", dict(var=None, Nz=4002), NULL),
    ("null-before-shape-R", dict(z=None, R=-1), NULL),
    *[(f"{k}={v}", {k: v}, SHAPE) for k, v in (("R", -1), ("Nd", 0), ("Nd", -5), ("Nz", 3999), ("Nz", 4002), ("edge", -1), ("interleaved", 2),
                                               ("interleaved", -1), ("n_lev", 3), ("n_lev", 16), ("n_lev", 0))],
    ("Nz=2^30", dict(Nz=1 << 30, Nd=1 << 30), SHAPE), ("Nz=2^30-from-Nd+1", dict(Nz=1 << 30, Nd=(1 << 30) - 1), SHAPE),
    ("Nd=0-Nz=1", dict(Nd=0, Nz=1), SHAPE),
]

S_NAMES = "R N n_lev K2 ff fb dec amp z stream".split()
S_BASE = (1, 4000, 4, 4, P, P, P, P, P, None)
S_PTRS = ("ff", "fb", "dec", "amp", "z")
S_CASES = [
    ("empty", dict(R=0, **{k: None for k in S_PTRS}), OK),
    ("empty-bad-shape", dict(R=0, n_lev=5, N=0, K2=0), OK),
    *[(f"null-{k}", {k: None}, NULL) for k in S_PTRS],
    ("null-before-shape", dict(fb=None, K2=11), NULL), ("null-before-shape-N", dict(z=None, N=0), NULL),
    *[(f"{k}={v}", {k: v}, SHAPE) for k, v in (("R", -1), ("N", 0), ("N", -1), ("N", 1 << 30), ("n_lev", 3), ("n_lev", 16), ("K2", 0), ("K2", 11),
                                               ("K2", -1))],
]


def _call(f, names, base, change):
    assert len(names) == len(base) == len(f.argtypes)
    args = list(base)
    for k, v in change.items():
        args[names.index(k)] = v
    return f(*args)


@pytest.mark.parametrize("case", T_CASES, ids=lambda c: c[0])
def test_track_info_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    assert _call(nat.lib().vaeq_awgn_track_info, T_NAMES, T_BASE, case[1]) == case[2]


@pytest.mark.parametrize("case", S_CASES, ids=lambda c: c[0])
def test_dfe_soft_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    assert _call(nat.lib().vaeq_awgn_dfe_soft, S_NAMES, S_BASE, case[1]) == case[2]


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    for name in ("vaeq_awgn_track_info", "vaeq_awgn_dfe_soft"):
        assert name in nat.EXPORTS and hasattr(nat.lib(), name)
    assert "vaeq_awgn_track_info.hip" in nat.SOURCES and "vaeq_info.h" in nat.HEADERS and "vaeq_awgn_eval.h" in nat.HEADERS
    with open(os.path.join(nat._ROOT, "include", "vaeq.h")) as fh:
        text = fh.read()
    assert "int vaeq_awgn_track_info(int32_t R, int64_t Nz, int64_t Nd, int32_t n_lev, int32_t edge, int32_t interleaved, const float *z," in text
    assert "int vaeq_awgn_dfe_soft(int32_t R, int64_t N, int32_t n_lev, int32_t K2, const float *ff, const float *fb, const int8_t *dec" in text

"""Which error code vaeq_cma_epilogue_llr and vaeq_awgn_track_llr return for which refused arguments, in the style of
tests/test_abi_refusals_llr_host.py: every argument set below is refused on the host before any HIP call, so no device is needed.  The order is
vaeq_cma_epilogue_info's resp. vaeq_awgn_track_info's -- empty batch, any NULL pointer (hyp and llr among them) before any shape rule, shape,
n_lev dispatch."""
import pytest

OK, NULL, SHAPE = 0, -1, -2
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

CMA_NAMES = "R N n_lev y tx amp var nu_sc shift_c r_c shift_q r_q hyp llr stream".split()
CMA_PTRS = CMA_NAMES[3:14]
CMA = (1, 4000, 4) + (P,) * 11 + (None,)                   # would be accepted

CMA_CASES = [
    ("empty", CMA, dict(R=0, **{k: None for k in CMA_PTRS}), OK),
    ("empty-bad-shape", CMA, dict(R=0, n_lev=3, N=1), OK),
    *[(f"null-{k}", CMA, {k: None}, NULL) for k in CMA_PTRS],
    *[(f"null-{k}-before-shape", CMA, {k: None, **bad}, NULL) for k, bad in (("hyp", dict(n_lev=3)), ("llr", dict(N=10)), ("tx", dict(R=-1)))],
    *[(f"{k}={v}", CMA, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("n_lev", 0), ("R", -1), ("N", 42), ("N", 0), ("N", -5),
                                                    ("N", 1 << 30))],
]

TRACK_NAMES = "R Nz Nd n_lev edge interleaved z data amp var shift hyp llr stream".split()
TRACK_PTRS = TRACK_NAMES[6:13]
TRACK = (1, 4000, 4000, 4, 11, 0) + (P,) * 7 + (None,)     # would be accepted
TRACK_IL = (1, 4001, 4000, 8, 31, 1) + (P,) * 7 + (None,)  # the LMMSE output: one sample more, interleaved

TRACK_CASES = [
    ("empty", TRACK, dict(R=0, **{k: None for k in TRACK_PTRS}), OK),
    ("empty-bad-shape", TRACK, dict(R=0, n_lev=3, Nd=0, Nz=7, edge=-1, interleaved=2), OK),
    *[(f"null-{k}", TRACK, {k: None}, NULL) for k in TRACK_PTRS],
    *[(f"il-null-{k}", TRACK_IL, {k: None}, NULL) for k in ("hyp", "llr")],
    *[(f"null-{k}-before-shape", TRACK, {k: None, **bad}, NULL) for k, bad in (("hyp", dict(n_lev=3)), ("llr", dict(Nz=3999)), ("z", dict(edge=-1)))],
    *[(f"{k}={v}", TRACK, {k: v}, SHAPE) for k, v in (("n_lev", 3), ("n_lev", 16), ("R", -1), ("Nz", 3999), ("Nz", 4002), ("edge", -1),
                                                      ("interleaved", 2), ("interleaved", -1))],
    ("Nd=0", TRACK, dict(Nd=0, Nz=0), SHAPE), ("Nd=-1", TRACK, dict(Nd=-1, Nz=0), SHAPE), ("Nz-too-long", TRACK, dict(Nd=1 << 30, Nz=1 << 30), SHAPE),
    ("il-Nz-too-long", TRACK_IL, dict(Nd=(1 << 30) - 1, Nz=1 << 30), SHAPE), ("il-n_lev=3", TRACK_IL, dict(n_lev=3), SHAPE),
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


@pytest.mark.parametrize("case", CMA_CASES, ids=lambda c: c[0])
def test_cma_refusal_code(case):
    _check("vaeq_cma_epilogue_llr", CMA_NAMES, case)


@pytest.mark.parametrize("case", TRACK_CASES, ids=lambda c: c[0])
def test_track_refusal_code(case):
    _check("vaeq_awgn_track_llr", TRACK_NAMES, case)


def test_declared_and_exported():
    import os
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaeq.h")).read()
    for fn in ("vaeq_cma_epilogue_llr", "vaeq_awgn_track_llr"):
        assert f"int {fn}(" in header and fn in nat.EXPORTS and hasattr(nat.lib(), fn)

"""The input-gradient entry points of include/vaeq.h (vaeq_dp_forward_bwd_x, vaeq_dp_loss_bwd_x, vaeq_awgn_forward_bwd_x, vaeq_awgn_loss_bwd_x,
vaeq_nn_enc_backward_x) on a host without a GPU: they are declared, exported and bound, and they refuse in the library's order -- an empty
batch owns no memory, then NULL before SHAPE -- with every shape check made on the host before any HIP call."""
import ctypes as C
import os
import re

import pytest

OK, NULL, SHAPE, LDS = 0, -1, -2, -3
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (parameter names, an argument set that would be accepted)
SIG = {
    "vaeq_dp_forward_bwd_x": ("R N sps M n_lev W q y gq gy amp var gx stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_dp_loss_bwd_x": ("R B sps M n_lev q x h amp g_up gx stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, None)),
    "vaeq_awgn_forward_bwd_x": ("R N sps M n_lev x W amp amp_mean var gq gy gx stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_loss_bwd_x": ("R B sps M n_lev q x h amp g_up gx stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, None)),
    "vaeq_nn_enc_backward_x": ("R L sps n_lev k1 k2 batch_norm training x theta q gq bn_stats g gx stream",
                               (1, 128, 2, 4, 25, 3, 1, 1, P, P, P, P, P, P, P, None)),
}
FIR = ["vaeq_dp_forward_bwd_x", "vaeq_awgn_forward_bwd_x"]
LOSS = ["vaeq_dp_loss_bwd_x", "vaeq_awgn_loss_bwd_x"]
OPTIONAL = {"gy", "stream"}                                # pointers that may be NULL (bn_stats: only without BatchNorm)


def _lib():
    from vae_equalizer_amd import _native as nat
    return nat.lib()


def _call(name, **over):
    names, args = SIG[name][0].split(), list(SIG[name][1])
    for k, v in over.items():
        args[names.index(k)] = v
    return int(getattr(_lib(), name)(*args))


def test_header_exports_and_bindings_agree():
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "vaeq.h")).read()
    L = _lib()
    for name, (params, args) in SIG.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/vaeq.h"
        declared = [re.sub(r"[\s*]+", " ", a).split()[-1] for a in m.group(1).split(",")]
        assert len(declared) == len(args), (name, declared)
        assert name in nat.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(args) and getattr(L, name).restype is C.c_int
    assert L.vaeq_version() == 100


@pytest.mark.parametrize("name", sorted(SIG))
def test_empty_batch_owns_no_memory(name):
    names = SIG[name][0].split()
    nothing = {k: None for k, v in zip(names, SIG[name][1]) if v == P}
    assert _call(name, R=0, **nothing) == OK
    assert _call(name, R=0, **nothing, **({"M": 24} if "M" in names else {"k1": 24})) == OK


@pytest.mark.parametrize("name", sorted(SIG))
def test_every_required_pointer_is_checked(name):
    names = SIG[name][0].split()
    for k, v in zip(names, SIG[name][1]):
        if v == P and k not in OPTIONAL:
            assert _call(name, **{k: None}) == NULL, (name, k)
    if "gy" in names:                                      # the upstream gradient on `out` is optional: NULL gets past the pointer check
        assert _call(name, gy=None, M=24) == SHAPE
    if name == "vaeq_nn_enc_backward_x":                   # Net has no statistics
        assert _call(name, bn_stats=None, batch_norm=0, k1=24) == SHAPE


@pytest.mark.parametrize("name", sorted(SIG))
def test_null_is_reported_before_shape(name):
    names = SIG[name][0].split()
    bad = {"M": 24} if "M" in names else {"k1": 24}
    assert _call(name, gx=None, **bad) == NULL
    assert _call(name, gx=None, sps=0) == NULL
    assert _call(name, **bad) == SHAPE


@pytest.mark.parametrize("name", FIR + LOSS)
@pytest.mark.parametrize("over", [dict(M=24), dict(M=0), dict(M=65), dict(M=64), dict(M=-1), dict(sps=0), dict(sps=-2), dict(n_lev=3), dict(n_lev=16),
                                  dict(n_lev=0), dict(R=-1)])
def test_fir_and_loss_shapes(name, over):
    assert _call(name, **over) == SHAPE


@pytest.mark.parametrize("name", FIR)
def test_fir_needs_a_symbol(name):
    assert _call(name, N=0) == SHAPE and _call(name, N=-5) == SHAPE
    assert _call(name, M=63, N=1, n_lev=3) == SHAPE        # (M = 63 and N = 1 are fine: only n_lev is refused)


@pytest.mark.parametrize("name", LOSS)
def test_loss_needs_more_symbols_than_taps(name):
    for B, M in ((24, 25), (8, 9), (62, 63), (0, 1), (-3, 1)):
        assert _call(name, B=B, M=M) == SHAPE, (B, M)      # B <= 2 (M // 2)
    assert _call(name, B=25, M=25, n_lev=3) == SHAPE       # (B = 2 (M // 2) + 1 passes the length check: only n_lev is refused)


@pytest.mark.parametrize("name,B,code", [("vaeq_dp_loss_bwd_x", 2546, SHAPE), ("vaeq_dp_loss_bwd_x", 2547, LDS),
                                         ("vaeq_awgn_loss_bwd_x", 4806, SHAPE), ("vaeq_awgn_loss_bwd_x", 4807, LDS),
                                         ("vaeq_dp_forward_bwd_x", 10190, SHAPE), ("vaeq_dp_forward_bwd_x", 10191, LDS),
                                         ("vaeq_awgn_forward_bwd_x", 9600, SHAPE), ("vaeq_awgn_forward_bwd_x", 9601, LDS)])
def test_lds_is_reported_before_n_lev(name, B, code):
    """sps 2, M 25.  The loss kernels keep their siblings' working set (160 KiB all dynamic for DP: 4 (8 B + 4 nm + 10 M + 64); 150 KiB beside
    the static arrays for AWGN: 4 (4 B + 2 nm)); the DP FIR keeps dL/dout and the taps, 4 (4 N + 8 M) <= 160 KiB; the AWGN FIR y and dL/dy,
    16 N <= 150 KiB.  With an n_lev no kernel exists for, the largest admitted size reaches the dispatch (SHAPE) and one more is refused
    for its size (LDS) -- all on the host."""
    key = "B" if "loss" in name else "N"
    assert _call(name, n_lev=3, **{key: B}) == code


@pytest.mark.parametrize("over", [dict(k1=24), dict(k1=65), dict(k1=0), dict(k2=2), dict(k2=11), dict(k2=0), dict(sps=0), dict(sps=9), dict(n_lev=3),
                                  dict(n_lev=16), dict(L=0), dict(L=-1), dict(R=-1)])
def test_encoder_shapes(over):
    assert _call("vaeq_nn_enc_backward_x", **over) == SHAPE


def test_encoder_length_past_the_layout_arithmetic():
    assert _call("vaeq_nn_enc_backward_x", L=(1 << 20) + 1) == LDS

"""vaeq_ldpc_decode_q (the fixed-point QC-LDPC decoder: q-bit LLRs and messages, saturating a-posteriori values) against the integer model
tests/_ref_ldpc_q.py, through engine.ldpc_decode(quant=...).

No tolerance: behind its quantiser the decoder is integer arithmetic and the header fixes every rounding, clamp and tie, so the five counters
and every final L have to be the model's.  tests/test_ref_ldpc_q_host.py pins the model to an independent scalar restatement, shows that every
rule binds in these cases and that they reach iters == 0, several iterations and max_iter without success.

Cases: tests/test_ldpc_gpu.py's (R = 3 runs of C = 5 codewords, t0 in {0, 11}, w in {12, 8, 6}, three noise levels, max_iter in {1, 20}; Z = 7
below a wave, Z = 80 across two) under parameter set A, with ties of the rounding, one +inf and one NaN planted per run; sets B to E at w = 12,
t0 = 11; depth in {1, 2, 5} on tests/_ref_ldpc_il.py's inputs (not one symbol to spare, loud unused planes) under A and B; then the corners of
the envelope, among them a code whose state the float decoder must refuse.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import _ref_ldpc as M
import _ref_ldpc_il as IL
import _ref_ldpc_q as Q
from _ldpc_cases import _check_q as _check, _counters, _decode

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t0", [0, 11])
@pytest.mark.parametrize("w", [12, 8, 6])
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_against_the_model(code, w, t0):
    shifts, Z = M.CODES[code]
    for level in range(3):
        llr, bits = Q.case(code, w, t0, level, "A")
        assert np.isnan(llr).sum() == M.R_ and np.isinf(llr).sum() == M.R_
        dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
        for max_iter in (1, 20):
            want_out, want_post = Q.expected(code, w, t0, level, "A", max_iter)
            r = _decode(shifts, Z, dl, db, t0=t0, codewords=M.C_, max_iter=max_iter, quant=Q.SETS["A"])
            _check(r, want_out, want_post, shifts.shape[1] * Z, f"{code} w={w} t0={t0} sigma={M.SIGMAS[level]} max_iter={max_iter} set A")
            assert r["quant"] == Q.SETS["A"]


@pytest.mark.parametrize("name", ["B", "C", "D", "E"])
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_the_other_parameter_sets(code, name):
    shifts, Z = M.CODES[code]
    for level in range(3):
        llr, bits = Q.case(code, 12, 11, level, name)
        want_out, want_post = Q.expected(code, 12, 11, level, name, 20)
        r = _decode(shifts, Z, llr, bits, t0=11, codewords=M.C_, quant=Q.SETS[name])
        _check(r, want_out, want_post, shifts.shape[1] * Z, f"{code} sigma={M.SIGMAS[level]} set {name}")


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("depth", IL.DEPTHS)
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_behind_the_interleaver(code, depth, name):
    shifts, Z = M.CODES[code]
    n = shifts.shape[1] * Z
    for w, t0 in ((12, 11), (8, 0), (6, 11)):
        S = IL.symbols_per_codeword(n, w)
        for level in range(3):
            llr, bits = Q.case_il(code, w, t0, level, depth, name)
            assert llr.shape == (M.R_, w, t0 + M.C_ * S)                          # not one symbol to spare
            free = IL.unused(t0, M.C_, n, w, depth)
            if free.any():                                                       # loud against a 0 bit: counting one changes pre_err
                assert ((llr[:, free] == IL.LOUD) | (llr[:, free] == 0)).all() and not bits[:, free].any()
            want_out, want_post = Q.expected_il(code, w, t0, level, depth, name, 20)
            r = _decode(shifts, Z, llr, bits, t0=t0, codewords=M.C_, depth=depth, quant=Q.SETS[name])
            _check(r, want_out, want_post, n, f"{code} w={w} t0={t0} depth={depth} sigma={M.SIGMAS[level]} set {name}")


@pytest.mark.parametrize("code", sorted(M.CODES))
def test_dp_view_and_flat_form_agree(code):
    """A non-contiguous [R,2,2b,N] view (the DP tensors: w = 4 b = 12) gives what the contiguous [R,w,N] form gives, and no post without asking."""
    from vae_equalizer_amd.engine import LdpcCode, ldpc_decode
    shifts, Z = M.CODES[code]
    llr, bits = Q.case(code, 12, 11, 1, "A")
    R, _, N = llr.shape
    big_l = torch.full((R, 2, 6, N + 5), -3.0, device="cuda")
    big_b = torch.full((R, 2, 6, N + 5), 1, dtype=torch.int8, device="cuda")
    big_l[..., :N] = torch.from_numpy(llr).cuda().reshape(R, 2, 6, N)
    big_b[..., :N] = torch.from_numpy(bits).cuda().reshape(R, 2, 6, N)
    vl, vb = big_l[..., :N], big_b[..., :N]
    assert not vl.is_contiguous()
    want_out, want_post = Q.expected(code, 12, 11, 1, "A", 20)
    _check(_decode(shifts, Z, vl, vb, t0=11, codewords=M.C_, quant=Q.SETS["A"]), want_out, want_post, shifts.shape[1] * Z, f"{code} DP view")
    plain = ldpc_decode(vl, vb, LdpcCode(shifts, Z), t0=11, codewords=M.C_, quant=Q.SETS["A"])
    assert "post" not in plain and np.array_equal(_counters(plain), want_out)


def test_two_calls_and_the_float_decoder_s_pre_err():
    from vae_equalizer_amd.engine import LdpcCode, ldpc_decode
    shifts, Z = M.CODES["irregular-5-12-80"]
    for name in ("A", "E"):
        llr, bits = Q.case("irregular-5-12-80", 8, 11, 2, name, False)           # no planted NaN
        dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
        want_out, want_post = Q.expected("irregular-5-12-80", 8, 11, 2, name, 9, False)
        a = _decode(shifts, Z, dl, db, t0=11, codewords=M.C_, max_iter=9, quant=Q.SETS[name])
        _check(a, want_out, want_post, 960, f"set {name}, max_iter 9")
        b = _decode(shifts, Z, dl, db, t0=11, codewords=M.C_, max_iter=9, quant=Q.SETS[name])
        assert np.array_equal(_counters(a), _counters(b)) and torch.equal(a["post"], b["post"])
        flt = ldpc_decode(dl, db, LdpcCode(shifts, Z), t0=11, codewords=M.C_, max_iter=1)
        print(f"set {name}: pre_err {a['pre_err'].tolist()} float {flt['pre_err'].tolist()}")
        assert "quant" not in flt and torch.equal(a["pre_err"], flt["pre_err"]) and int(a["pre_err"].sum()) > 0


def test_defaults_and_bad_arguments():
    from vae_equalizer_amd._native import VaeqError
    from vae_equalizer_amd.engine import resolve_quant
    shifts, Z = M.CODES["array-3-6-7"]
    assert resolve_quant(dict(bits=4)) == dict(bits=4, scale=0.5, app_bits=6, num=6, beta=0)
    assert resolve_quant(dict(bits=5)) == dict(bits=5, scale=1.0, app_bits=7, num=6, beta=0) == Q.SETS["A"]
    llr, bits = Q.case("array-3-6-7", 12, 11, 1, "B")                            # planted at the scale 0.5 of 4 bits
    prm = dict(bits=4, scale=0.5, app_bits=6, num=6, beta=0)
    want_out, want_post = Q.decode_batch(shifts, Z, llr, bits, 11, M.C_, prm)
    r = _decode(shifts, Z, llr, bits, t0=11, codewords=M.C_, quant=dict(bits=4))
    _check(r, want_out, want_post, 42, "quant=dict(bits=4)")
    assert r["quant"] == prm
    r = _decode(shifts, Z, llr, bits, t0=11, quant=dict(bits=4), depth=None)     # depth None is depth 0; codewords default to the most that fit
    fit = (llr.shape[-1] - 11) * 12 // 42
    assert fit > M.C_ and _counters(r).shape == (M.R_, fit, 5) and np.array_equal(_counters(r)[:, :M.C_], want_out)
    for bad in (dict(), dict(bitz=5), dict(bits=5, scal=1.0), dict(bits=5.0), dict(bits="5")):
        with pytest.raises(ValueError):
            _decode(shifts, Z, llr, bits, t0=11, quant=bad)
    with pytest.raises(ValueError):
        _decode(shifts, Z, llr, bits, t0=11, quant=dict(bits=5), alpha=0.75)
    for bad in (dict(bits=9), dict(bits=1), dict(bits=5, app_bits=4), dict(bits=5, app_bits=16), dict(bits=5, scale=0.0), dict(bits=5, num=9),
                dict(bits=5, beta=128)):
        with pytest.raises(VaeqError):
            _decode(shifts, Z, llr, bits, t0=11, codewords=M.C_, quant=bad)


ENVELOPE = {
    "row-weight-32-in-8-layers": (8, 33, 13, 1),                                # one hole per block row: 32 edges per check
    "row-weight-32-at-61440-bytes": (3, 32, 512, 0),                            # 512 threads; 106 496 bytes in float32: refused there
    "smallest": (1, 2, 2, 0),
}


@pytest.mark.parametrize("name", sorted(ENVELOPE))
def test_corners_of_the_envelope(name):
    from vae_equalizer_amd import _native as nat
    mb, nb, Z, holes = ENVELOPE[name]
    shifts = M.array_shifts(mb, nb, Z)
    for l in range(mb if holes else 0):
        shifts[l, (3 * l + 1) % nb] = -1
    n = nb * Z
    lds = nat.lib().vaeq_ldpc_q_lds_bytes(mb, nb, Z)
    assert 0 < lds <= 64 * 1024 and int((shifts >= 0).sum(1).max()) == min(nb, 32)
    for level, sigma in enumerate((0.5, 0.8)):
        llr, bits = Q.make_case_q(77 + level, n, sigma, 2, 3, 12, 5, 1.0, erasures=2)
        want_out, want_post = Q.decode_batch(shifts, Z, llr, bits, 5, 3, Q.SETS["A"], 6)
        _check(_decode(shifts, Z, llr, bits, t0=5, codewords=3, max_iter=6, quant=Q.SETS["A"]), want_out, want_post, n, f"{name} sigma={sigma}")
    if name == "row-weight-32-at-61440-bytes":
        assert lds == 61440 and nat.lib().vaeq_ldpc_lds_bytes(mb, nb, Z) > 64 * 1024
        with pytest.raises(nat.VaeqError):
            _decode(shifts, Z, llr, bits, t0=5, codewords=3, max_iter=6)

"""vaeq_ldpc_decode (the batched QC-LDPC decoder over the demappers' LLRs) against the float32 model tests/_ref_ldpc.py, through
engine.ldpc_decode.

No tolerance: the header fixes the decoder down to the order of its individually rounded float32 operations, so the five counters and every
bit of the final LLRs have to be the model's; a differing value is a contraction or an ordering bug in the kernel.  tests/test_ref_ldpc_host.py
pins the model to an independent scalar restatement and asserts that the seeded cases reach iters == 0, several iterations, and max_iter
without success.

Cases (tests/_ref_ldpc.py): R = 3 runs of C = 5 codewords, t0 in {0, 11}, w in {12, 8, 6}, sigma in {0.3, 0.5, 0.8}, max_iter in {1, 20} on
array_code(3, 6, 7) (Z below a wave, n % 12 != 0: codewords start inside a symbol), array_code(4, 24, 31), and a seeded irregular 5 x 12 code
with holes at Z = 80 (non-prime, the checks of a layer on two waves); then the corners of the envelope: row weight 32 in 8 layers, Z = 512 with
61 952 bytes of state.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import _ref_ldpc as M
from _ldpc_cases import _check, _counters, _decode

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t0", [0, 11])
@pytest.mark.parametrize("w", [12, 8, 6])
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_against_the_model(code, w, t0):
    shifts, Z = M.CODES[code]
    for level in range(3):
        llr, bits = M.case(code, w, t0, level)
        for max_iter in (1, 20):
            want_out, want_post = M.expected(code, w, t0, level, max_iter)
            r = _decode(shifts, Z, llr, bits, t0=t0, codewords=M.C_, max_iter=max_iter)
            _check(r, want_out, want_post, shifts.shape[1] * Z, f"{code} w={w} t0={t0} sigma={M.SIGMAS[level]} max_iter={max_iter}")


@pytest.mark.parametrize("code", sorted(M.CODES))
def test_dp_view_and_flat_form_agree(code):
    """A non-contiguous [R,2,2b,N] view (the DP tensors: w = 4 b = 12) gives what the contiguous [R,w,N] form gives, and no post without asking."""
    from vae_equalizer_amd.engine import LdpcCode, ldpc_decode
    shifts, Z = M.CODES[code]
    llr, bits = M.case(code, 12, 11, 1)
    R, _, N = llr.shape
    big_l = torch.full((R, 2, 6, N + 5), float("nan"), device="cuda")
    big_b = torch.full((R, 2, 6, N + 5), 1, dtype=torch.int8, device="cuda")
    big_l[..., :N] = torch.from_numpy(llr).cuda().reshape(R, 2, 6, N)
    big_b[..., :N] = torch.from_numpy(bits).cuda().reshape(R, 2, 6, N)
    vl, vb = big_l[..., :N], big_b[..., :N]
    assert not vl.is_contiguous()
    want_out, want_post = M.expected(code, 12, 11, 1, 20)
    _check(_decode(shifts, Z, vl, vb, t0=11, codewords=M.C_), want_out, want_post, shifts.shape[1] * Z, f"{code} DP view")
    plain = ldpc_decode(vl, vb, LdpcCode(shifts, Z), t0=11, codewords=M.C_)
    assert "post" not in plain and np.array_equal(_counters(plain), want_out)


def test_default_codewords_are_the_most_that_fit():
    shifts, Z = M.CODES["array-3-6-7"]
    llr, bits = M.case("array-3-6-7", 12, 0, 1)                                  # 21 symbols of 12 bits: six codewords of 42 bits, to the last bit
    assert llr.shape[-1] * 12 == 6 * 42
    want_out, want_post = M.decode_batch(shifts, Z, llr, bits, 0, 6)
    _check(_decode(shifts, Z, llr, bits), want_out, want_post, 42, "default codewords")
    r = _decode(shifts, Z, llr, bits, t0=1)
    assert tuple(r["iters"].shape) == (3, 5)
    with pytest.raises(ValueError):
        _decode(shifts, Z, llr, bits, t0=18)                                      # 36 bits left: no codeword fits
    from vae_equalizer_amd._native import VaeqError
    with pytest.raises(VaeqError):
        _decode(shifts, Z, llr, bits, codewords=7)


def test_other_alpha_and_two_calls():
    shifts, Z = M.CODES["irregular-5-12-80"]
    llr, bits = M.case("irregular-5-12-80", 8, 11, 2)
    want_out, want_post = M.decode_batch(shifts, Z, llr, bits, 11, M.C_, 9, 0.8125)
    a = _decode(shifts, Z, llr, bits, t0=11, codewords=M.C_, max_iter=9, alpha=0.8125)
    _check(a, want_out, want_post, 960, "alpha 0.8125, max_iter 9")
    b = _decode(shifts, Z, llr, bits, t0=11, codewords=M.C_, max_iter=9, alpha=0.8125)
    assert np.array_equal(_counters(a), _counters(b)) and torch.equal(a["post"].view(torch.int32), b["post"].view(torch.int32))


ENVELOPE = {
    "row-weight-32-in-8-layers": (8, 33, 13, 1),                                # one hole per block row: 32 edges per check
    "Z-512-largest-state": (6, 5, 512, 0),                                      # 512 threads, 61 952 of the 65 536 bytes
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
    assert 0 < nat.lib().vaeq_ldpc_lds_bytes(mb, nb, Z) <= 64 * 1024
    for level, sigma in enumerate((0.5, 0.8)):
        llr, bits = M.make_case(77 + level, n, sigma, 2, 3, 12, 5, erasures=2)
        want_out, want_post = M.decode_batch(shifts, Z, llr, bits, 5, 3, 6)
        _check(_decode(shifts, Z, llr, bits, t0=5, codewords=3, max_iter=6), want_out, want_post, n, f"{name} sigma={sigma}")

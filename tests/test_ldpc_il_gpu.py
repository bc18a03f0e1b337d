"""vaeq_ldpc_decode_il (the batched QC-LDPC decoder behind a symbol interleaver over groups of `depth` codewords) against the model
tests/_ref_ldpc_il.py, through engine.ldpc_decode(depth=...).

No tolerance, as in tests/test_ldpc_gpu.py: the five counters and every bit of the final LLRs have to be the model's.  tests/test_ref_ldpc_il_host.py
holds the map itself (no overlap, containment, the degenerate depths).

Cases: the codes, t0, w, sigmas and max_iter of tests/test_ldpc_gpu.py (R = 3 runs of C = 5 codewords) at depth 1 (symbol-aligned contiguous),
2 (groups of 2, 2 and a ragged 1) and 5 (every codeword over the whole frame).  array-3-6-7 has n = 42: n % w is 6 at w = 12, 2 at w = 8 and 0 at
w = 6 (where the four-plane load runs into its clamp).  Every input has exactly N = t0 + C S symbols, so a read past the last symbol leaves
the buffer; the planes of partial last symbols that belong to no codeword hold -1e4 against a 0 bit and one exact zero, so that counting any
of them changes pre_err or erased; every run has four erasures inside its codewords.  The contiguous entry point runs on the same tensors
against its own model, tests/_ref_ldpc.py: it has to return what it returned before.  Then the corner Z = 512 at the largest state with
depth = C = 2.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import _ref_ldpc as M
import _ref_ldpc_il as IL
from _ldpc_cases import _check, _counters, _decode

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("depth", IL.DEPTHS)
@pytest.mark.parametrize("t0", [0, 11])
@pytest.mark.parametrize("w", [12, 8, 6])
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_against_the_model(code, w, t0, depth):
    shifts, Z = M.CODES[code]
    n = shifts.shape[1] * Z
    S = IL.symbols_per_codeword(n, w)
    for level in range(3):
        llr, bits = IL.case(code, w, t0, level, depth)
        assert llr.shape == (M.R_, w, t0 + M.C_ * S)                              # not one symbol to spare
        free = IL.unused(t0, M.C_, n, w, depth)
        assert int(free.sum()) == M.C_ * (S * w - n)
        if free.any():                                                           # loud, and with an erasure of their own
            assert ((llr[:, free] == IL.LOUD) | (llr[:, free] == 0)).all() and (llr[:, free] == 0).any() and not bits[:, free].any()
        dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
        for max_iter in (1, 20):
            want_out, want_post = IL.expected(code, w, t0, level, depth, max_iter)
            assert (want_out[..., 4].sum(1) == 4).all()                          # the erasures inside the codewords, and none of the others
            tag = f"{code} w={w} t0={t0} depth={depth} sigma={M.SIGMAS[level]} max_iter={max_iter}"
            _check(_decode(shifts, Z, dl, db, t0=t0, codewords=M.C_, max_iter=max_iter, depth=depth), want_out, want_post, n, tag)
            old_out, old_post = IL.expected_old(code, w, t0, level, depth, max_iter)
            _check(_decode(shifts, Z, dl, db, t0=t0, codewords=M.C_, max_iter=max_iter), old_out, old_post, n, tag + " contiguous")


def test_default_codewords_and_refusals():
    from vae_equalizer_amd._native import VaeqError
    from vae_equalizer_amd.engine import LdpcCode, ldpc_decode
    shifts, Z = M.CODES["array-3-6-7"]
    llr, bits = IL.case("array-3-6-7", 12, 11, 1, 2)                               # 11 + 5 x 4 symbols
    dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
    r = _decode(shifts, Z, dl, db, t0=11, depth=2)                                 # codewords default to (N - t0) // S = 5
    _check(r, *IL.expected("array-3-6-7", 12, 11, 1, 2, 20), 42, "default codewords")
    assert tuple(_decode(shifts, Z, dl, db, t0=12, depth=2)["iters"].shape) == (3, 4)
    for bad in (dict(depth=0), dict(depth=6), dict(depth=2, codewords=6)):
        with pytest.raises(VaeqError):
            _decode(shifts, Z, dl, db, t0=11, **{"codewords": 5, **bad})
    with pytest.raises(ValueError):
        _decode(shifts, Z, dl, db, t0=29, depth=1)                                 # 2 symbols left: no codeword fits
    plain = ldpc_decode(dl, db, LdpcCode(shifts, Z), t0=11, depth=2)
    assert "post" not in plain and np.array_equal(_counters(plain), IL.expected("array-3-6-7", 12, 11, 1, 2, 20)[0])


def test_z_512_at_the_state_limit():
    """Z = 512, 61 952 of the 65 536 bytes of state, 512 threads for S = 214 symbols: depth = C = 2, n % w = 4."""
    from vae_equalizer_amd import _native as nat
    mb, nb, Z = 6, 5, 512
    shifts = M.array_shifts(mb, nb, Z)
    n = nb * Z
    assert 0 < nat.lib().vaeq_ldpc_lds_bytes(mb, nb, Z) <= 64 * 1024
    for level, sigma in enumerate((0.5, 0.8)):
        llr, bits = IL.make_case_il(177 + level, n, sigma, 2, 2, 12, 5, 2, erasures=2)
        assert llr.shape[-1] == 5 + 2 * 214
        want_out, want_post = IL.decode_batch_il(shifts, Z, llr, bits, 5, 2, 2, 6)
        dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
        _check(_decode(shifts, Z, dl, db, t0=5, codewords=2, max_iter=6, depth=2), want_out, want_post, n, f"Z=512 depth=2 sigma={sigma}")
        old_out, old_post = M.decode_batch(shifts, Z, llr, bits, 5, 2, 6)
        _check(_decode(shifts, Z, dl, db, t0=5, codewords=2, max_iter=6), old_out, old_post, n, f"Z=512 contiguous sigma={sigma}")

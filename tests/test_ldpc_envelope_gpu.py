"""The three LDPC entry points (vaeq_ldpc_decode, vaeq_ldpc_decode_il, vaeq_ldpc_decode_q) over the parts of include/vaeq.h's envelope that the
tests of their feature commits leave out, through engine.ldpc_decode(..., want_post=True).

No tolerance anywhere: every comparison is np.array_equal on the five counters and on `post` (float32 through a uint32 view, int16 directly),
and the derived BER_post / BER_pre / FER as in tests/test_ldpc_gpu.py.  The cases live in tests/_ldpc_cases.py; the host tests
(tests/test_ref_ldpc_host.py, test_ref_ldpc_q_host.py, test_ref_ldpc_il_host.py) assert on the CPU that the models reach in them what this file
relies on.  Every test prints its figures before it asserts.

A. Against the models tests/_ref_ldpc.py, _ref_ldpc_il.py, _ref_ldpc_q.py (the fixed-point decoder under set A with its planted values):
   1. row weights 2, 8, 9, 16, 17, 25, 31, 32 in one table (mb = 8, nb = 40, Z = 65), and in the reverse layer order;
   2. nb = 64 at the largest Z the state allows (186 in float32, 315 in fixed point): the top of the 7-bit column field, row weight 32 in two
      layers (a row of 64 blocks is outside the envelope, so array_shifts(2, 64, Z) keeps 32 per row), max_iter = 100 reached undecoded;
   3. Z in {63, 64, 65, 511, 512} with a planted shift Z - 1 (i + s up to 2 Z - 2) and a planted shift 0;
   4. w in {1, 2, 3, 4, 5, 7, 13, 64}, contiguous and at depths 1, 2, 5 (n = 42 < w = 64: a codeword is part of one symbol);
   5. the grid: 300 codewords in one run (depth 7: a ragged group of six), 40 runs of one codeword, one workgroup;
   6. ragged last groups of more than one codeword: C = 7 at depths 3, 4, 7;
   7. alpha 0.7, 1.0, 0.5;  8. planted infinities of either sign (float decoder; a NaN there is outside the header's contract);
   9. the fixed-point corners: num = 1 with beta = 127, 8/8 and 2/2 bits, scale 1e-30 and 1e30 with -inf, a subnormal and both zeros planted.
C. The decoders held to each other with no model in the loop: float32 at alpha = 1 on small integers equals the fixed-point decoder where
   nothing clamps; the interleaved entry points equal the contiguous ones on the de-interleaved tensor."""
import numpy as np
import pytest
import torch

import _ldpc_cases as K
import _ref_ldpc as M
import _ref_ldpc_il as IL

pytestmark = pytest.mark.gpu


def _both(case, depth=None):
    """The float decoder, and the fixed-point one under set A on the same tensors with _ref_ldpc_q's values planted."""
    K.run(case, depth)
    K.run(case, depth, "A")


# ------------------------------------------------------------------ A. against the models
@pytest.mark.parametrize("sigma", [0.25, 0.45])
@pytest.mark.parametrize("name", ["mixed", "mixed-reversed"])
def test_mixed_row_weights(name, sigma):
    shifts, Z = K.code(name)
    assert sorted((shifts >= 0).sum(1).tolist()) == list(K.WEIGHTS) and (shifts >= 0).any(0).all()
    _both(K.MIXED[name, sigma])


@pytest.mark.parametrize("sigma", [0.3, 0.4])
def test_64_block_columns_at_the_state_limit(sigma):
    from vae_equalizer_amd import _native as nat
    assert nat.lib().vaeq_ldpc_lds_bytes(2, 64, K.Z_FLOAT_64) == 65472 and nat.lib().vaeq_ldpc_q_lds_bytes(2, 64, K.Z_Q_64) == 65520
    K.run(K.NB64[K.Z_FLOAT_64, sigma])
    K.run(K.NB64[K.Z_FLOAT_64, sigma], None, "A")
    K.run(K.NB64[K.Z_Q_64, sigma], None, "A")
    case = K.NB64[K.Z_Q_64, sigma]
    assert nat.lib().vaeq_ldpc_lds_bytes(2, 64, K.Z_Q_64) > 64 * 1024             # the float decoder must refuse the fixed-point one's largest Z
    with pytest.raises(nat.VaeqError):
        K._decode(*K.code(case.code), *K.inputs(case), t0=case.t0, codewords=case.C)


@pytest.mark.parametrize("sigma", [0.55, 0.65])
@pytest.mark.parametrize("Z", K.Z_WAVE)
def test_z_at_the_wave_boundary(Z, sigma):
    shifts, _ = K.code(f"planted-{Z}")
    assert (shifts == Z - 1).any() and (shifts == 0).any()
    _both(K.WAVE[Z, sigma])


@pytest.mark.parametrize("t0", [0, 11])
@pytest.mark.parametrize("w", K.WIDTHS)
@pytest.mark.parametrize("name", K.W_CODES)
def test_every_w(name, w, t0):
    n = K.n_of(K.width_case(name, w, t0, 0))
    S = IL.symbols_per_codeword(n, w)
    for level in range(3):
        case = K.width_case(name, w, t0, level)
        _both(case)
        for depth in IL.DEPTHS:
            llr, bits = K.inputs(case, depth)
            assert llr.shape == (case.R, w, t0 + case.C * S)                      # not one symbol to spare
            free = IL.unused(t0, case.C, n, w, depth)
            assert int(free.sum()) == case.C * (S * w - n)
            if free.any():                                                       # loud, and with an erasure of their own
                assert ((llr[:, free] == IL.LOUD) | (llr[:, free] == 0)).all() and (llr[:, free] == 0).any() and not bits[:, free].any()
            assert (K.expected(case, depth)[0][..., 4].sum(1) == 4).all()        # the erasures inside the codewords, and none of the others
            _both(case, depth)


@pytest.mark.parametrize("name", sorted(K.GRID))
def test_grid(name):
    case, depths = K.GRID[name]
    _both(case)
    for depth in depths:
        _both(case, depth)


@pytest.mark.parametrize("depth", K.RAGGED_DEPTHS)
@pytest.mark.parametrize("name,w", K.RAGGED)
def test_ragged_groups(name, w, depth):
    for level in range(3):
        _both(K.ragged_case(name, w, level), depth)


@pytest.mark.parametrize("alpha", K.ALPHAS)
def test_alpha(alpha):
    K.run(K.ALPHA_CASE, alpha=alpha)


def test_saturated_inputs():
    llr, bits, want_out, want_post, wrong = K.saturated()
    assert np.isinf(llr).sum() == K.SATURATED_CASE.R * K.SATURATED_CASE.C + 1 and not np.isnan(want_post).any()
    r = K.run(K.SATURATED_CASE, given=(llr, bits, want_out, want_post), tag="planted +-inf")
    assert not torch.isnan(r["post"]).any() and int(r["iters"][wrong]) == K.SATURATED_CASE.max_iter and int(r["ok"][wrong]) == 0


@pytest.mark.parametrize("quant", K.CORNER_SETS)
@pytest.mark.parametrize("name", K.W_CODES)
def test_fixed_point_corners(name, quant):
    for level in range(3):
        case = K.corner_case(name, level, quant)
        llr, _ = K.inputs(case, None, quant, True)
        assert np.isneginf(llr).sum() == np.isposinf(llr).sum() == np.isnan(llr).sum() == case.R
        K.run(case, None, quant, extra=True)


# ------------------------------------------------------------------ C. the decoders held to each other
@pytest.mark.parametrize("depth", [None, 2])
def test_float_is_fixed_point_where_nothing_clamps(depth):
    """alpha = 1 on integer LLRs is exact integer arithmetic in float32; bits = 8, app_bits = 15, scale = 1, num = 8, beta = 0 make f the identity
    and (tests/test_ref_ldpc_q_host.py) no clamp binds: the two kernels must agree in every counter and every final value."""
    case = K.INTEGER_CASE
    shifts, Z = K.code(case.code)
    llr, bits = K.integers()
    kw = dict(t0=case.t0, codewords=case.C, max_iter=case.max_iter, depth=depth)
    f = K._decode(shifts, Z, llr, bits, alpha=1.0, **kw)
    q = K._decode(shifts, Z, llr, bits, quant=K.QSETS["identity"], **kw)
    fo, qo, fp, qp = K._counters(f), K._counters(q), f["post"].cpu().numpy(), q["post"].cpu().numpy()
    print(f"depth={depth}: float iters {np.bincount(fo[..., 0].ravel()).tolist()} ok {int(fo[..., 1].sum())}/{fo[..., 1].size} pre_err "
          f"{int(fo[..., 3].sum())} post_err {int(fo[..., 2].sum())} erased {int(fo[..., 4].sum())} max |post| {np.abs(fp).max()}; "
          f"counters differ in {int((fo != qo).sum())}, post in {int((fp != qp).sum())} of {qp.size}")
    assert fp.dtype == np.float32 and qp.dtype == np.int16 and np.array_equal(fp, np.rint(fp)) and np.abs(fp).max() < 2 ** 14
    assert np.array_equal(fo, qo)
    assert np.array_equal(fp.astype(np.int16), qp)
    assert len(set(fo[..., 0].ravel().tolist())) >= 3 and 0 < fo[..., 1].sum() < fo[..., 1].size   # not vacuous: the host test shows the same


@pytest.mark.parametrize("depth", K.RAGGED_DEPTHS)
@pytest.mark.parametrize("w", [6, 2])
def test_interleaved_is_contiguous_on_the_deinterleaved_tensor(w, depth):
    """n % w == 0: vaeq_ldpc_decode_il on a tensor is vaeq_ldpc_decode on the tensor with its symbols permuted back, bit for bit."""
    for level in range(3):
        case = K.Case("array-3-6-7", w, 11, M.R_, K.RAGGED_C, M.SIGMAS[level], 60000 + 10 * w + level)
        shifts, Z = K.code(case.code)
        S = K.n_of(case) // w
        for quant in (None, "A"):
            llr, bits = K.inputs(case, depth, quant)
            assert llr.shape[-1] == case.t0 + case.C * S
            kw = dict(t0=case.t0, codewords=case.C, **(dict(quant=K.QSETS[quant]) if quant else {}))
            a = K._decode(shifts, Z, llr, bits, depth=depth, **kw)
            b = K._decode(shifts, Z, K.deinterleave(llr, case.t0, case.C, S, depth), K.deinterleave(bits, case.t0, case.C, S, depth), **kw)
            ao, bo = K._counters(a), K._counters(b)
            ap, bp = (x["post"].cpu().numpy() for x in (a, b))
            if quant is None:
                ap, bp = K._bits(ap), K._bits(bp)
            print(f"w={w} depth={depth} sigma={case.sigma} {'set A' if quant else 'float'}: iters {np.bincount(ao[..., 0].ravel()).tolist()} ok "
                  f"{int(ao[..., 1].sum())}/{ao[..., 1].size} pre_err {int(ao[..., 3].sum())} post_err {int(ao[..., 2].sum())} erased "
                  f"{int(ao[..., 4].sum())}; counters differ in {int((ao != bo).sum())}, post in {int((ap != bp).sum())} of {ap.size}")
            assert np.array_equal(ao, bo)
            assert np.array_equal(ap, bp)
            for k in ("BER_post", "BER_pre", "FER"):
                assert torch.equal(a[k], b[k])

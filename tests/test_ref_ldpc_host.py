"""tests/_ref_ldpc.py, the float32 model vaeq_ldpc_decode is held to bit for bit (tests/test_ldpc_gpu.py), checked on the CPU: the vectorised
model against its independent scalar restatement, the code construction of engine.LdpcCode / engine.array_code against the model's, and that the
seeded cases cover what the GPU test relies on -- codewords that pass the first test, codewords that need several iterations, codewords that
end at max_iter undecoded.  The same for the cases of tests/test_ldpc_envelope_gpu.py (tests/_ldpc_cases.py): every new table held to the
scalar restatement in the codewords that iterate longest (the tables of Z >= 186 in one codeword and three iterations), and per case what the
GPU test would pass vacuously without -- the set of row weights, a column >= 33, iters == 100 undecoded, the planted shifts, counters that tell
the codewords of the grid apart, planted infinities that yield no NaN."""
import numpy as np
import pytest

import _ref_ldpc as M


def _equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("name,shifts,Z", [("array-3-6-7", *M.CODES["array-3-6-7"]), ("holes", M.irregular_shifts(3, 3, 7, 6, 2), 6)])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_vectorised_model_is_the_scalar_one(name, shifts, Z, level):
    n = shifts.shape[1] * Z
    llr, bits = M.make_case(40 + level, n, M.SIGMAS[level], 2, 3, 12, 0, erasures=3)
    lc, bc = M.codewords(llr, 0, 3, n), M.codewords(bits, 0, 3, n)
    seen = set()
    for r in range(2):
        for c in range(3):
            for max_iter in (1, 7):
                a, b = M.decode(shifts, Z, lc[r, c], bc[r, c], max_iter), M.decode_scalar(shifts, Z, lc[r, c], bc[r, c], max_iter)
                assert _equal(a, b), (name, level, r, c, max_iter, a[0], b[0])
                seen.add(int(a[0][0]))
    print(name, "level", level, "iteration counts met:", sorted(seen))


def test_other_alpha_is_the_scalar_one_too():
    shifts, Z = M.CODES["array-3-6-7"]
    llr, bits = M.make_case(5, 42, 0.6, 1, 4, 6, 2)
    lc, bc = M.codewords(llr, 2, 4, 42), M.codewords(bits, 2, 4, 42)
    for c in range(4):
        assert _equal(M.decode(shifts, Z, lc[0, c], bc[0, c], 9, 0.8125), M.decode_scalar(shifts, Z, lc[0, c], bc[0, c], 9, 0.8125))


@pytest.mark.parametrize("mb,nb,Z", [(3, 6, 7), (4, 24, 31)])
def test_array_code_has_no_4_cycles(mb, nb, Z):
    from vae_equalizer_amd.engine import LdpcCode, array_code
    code = array_code(mb, nb, Z)
    assert (code.mb, code.nb, code.Z, code.n, code.m) == (mb, nb, Z, nb * Z, mb * Z) and code.shifts.dtype == np.int32
    assert np.array_equal(code.shifts, M.array_shifts(mb, nb, Z))
    H = code.H()
    assert H.dtype == np.uint8 and H.shape == (code.m, code.n) and np.array_equal(H, M.dense_H(code.shifts, Z))
    assert (H.sum(1) == nb).all() and (H.sum(0) == mb).all()
    G = H.astype(np.int64) @ H.T.astype(np.int64)
    assert (G[~np.eye(code.m, dtype=bool)] <= 1).all()                           # two checks share at most one variable
    holes = M.irregular_shifts(3, 3, 7, 6, 2)
    assert np.array_equal(LdpcCode(holes, 6).H(), M.dense_H(holes, 6)) and (LdpcCode(holes, 6).H().sum(1) == 5).all()


def test_codeword_order_is_symbol_major():
    x = np.arange(2 * 6 * 20).reshape(2, 6, 20)
    cw = M.codewords(x, 3, 2, 42)                              # 84 bits = 14 symbols of 6 planes behind t0 = 3
    for r, c, j in [(0, 0, 0), (0, 0, 41), (1, 1, 0), (1, 1, 41), (0, 1, 17)]:
        g = c * 42 + j
        assert cw[r, c, j] == x[r, g % 6, 3 + g // 6]


@pytest.mark.parametrize("code", sorted(M.CODES))
def test_ok_means_the_syndrome_of_the_tx_bits(code):
    shifts, Z = M.CODES[code]
    H = M.dense_H(shifts, Z).astype(np.int64)
    n = H.shape[1]
    for level in range(3):
        llr, bits = M.case(code, 12, 0, level)
        out, post = M.expected(code, 12, 0, level, 20)
        bc = M.codewords(bits, 0, M.C_, n)
        for r in range(M.R_):
            for c in range(M.C_):
                match = np.array_equal(H @ (post[r, c] < 0) % 2, H @ bc[r, c] % 2)
                assert match == bool(out[r, c, 1]), (code, level, r, c)
                assert out[r, c, 2] == ((post[r, c] < 0) != bc[r, c].astype(bool)).sum()


def _all_cases(code, level, max_iter=20):
    return np.concatenate([M.expected(code, w, t0, level, max_iter)[0].reshape(-1, 5) for w in (12, 8, 6) for t0 in (0, 11)])


@pytest.mark.parametrize("code", sorted(M.CODES))
def test_cases_cover_what_the_gpu_test_relies_on(code):
    clean, mid, bad = (_all_cases(code, level) for level in range(3))
    print(code, "sigma 0.3 iters", np.bincount(clean[:, 0]).tolist(), "| sigma 0.5 iters", np.bincount(mid[:, 0]).tolist(), "ok", int(mid[:, 1].sum()),
          "of", len(mid), "pre-FEC BER %.2e" % (mid[:, 3].sum() / (len(mid) * M.CODES[code][0].shape[1] * M.CODES[code][1])),
          "| sigma 0.8 ok", int(bad[:, 1].sum()), "of", len(bad))
    assert (clean[:, 0] == 0).any() and (clean[:, 0] > 0).any()                  # some pass the first test; an erased 1 does not
    assert (clean[:, 4] > 0).any() and clean[:, 4].sum() == 6 * M.R_ * 4          # the erasures are counted
    assert (mid[:, 0] >= (1 if code == "array-3-6-7" else 2)).any() and (mid[:, 3] > 0).any()   # (42 bits are corrected in one iteration)
    assert ((bad[:, 0] == 20) & (bad[:, 1] == 0)).any()
    one = _all_cases(code, 2, 1)
    assert (one[:, 0] <= 1).all() and ((one[:, 0] == 1) & (one[:, 1] == 0)).any()   # max_iter = 1 stops undecoded codewords after one iteration
    if code == "array-4-24-31":                                                  # the rate-5/6 array code: decodes all at 0.5, none at 0.8
        assert (mid[:, 1] == 1).all() and (mid[:, 2] == 0).all()
        assert (bad[:, 1] == 0).all()


# ------------------------------------------------------------------ the cases of tests/test_ldpc_envelope_gpu.py (tests/_ldpc_cases.py)
def _scalar_agrees(case, picks, max_iter=None, alpha=0.75, given=None):
    """The vectorised model against decode_scalar on codewords picks = [(run, codeword), ..] of a case's inputs."""
    import _ldpc_cases as K
    shifts, Z = K.code(case.code)
    llr, bits = given or K.inputs(case)
    lc, bc = K.codewords_of(case, llr), K.codewords_of(case, bits)
    max_iter = case.max_iter if max_iter is None else max_iter
    seen = []
    for r, c in picks:
        a, b = M.decode(shifts, Z, lc[r, c], bc[r, c], max_iter, alpha), M.decode_scalar(shifts, Z, lc[r, c], bc[r, c], max_iter, alpha)
        assert _equal(a, b), (case, r, c, a[0], b[0])
        seen.append(int(a[0][0]))
    print(case.code, "sigma", case.sigma, "alpha", alpha, "iterations of the codewords held to the scalar model:", seen)
    return seen


def _most_iterations(out, k=2):
    import _ldpc_cases as K
    return K.most_iterations(out, k)


@pytest.mark.parametrize("name", ["mixed", "mixed-reversed"])
def test_envelope_mixed_row_weights(name):
    import _ldpc_cases as K
    shifts, Z = K.code(name)
    wts = (shifts >= 0).sum(1).tolist()
    assert wts == list(K.WEIGHTS if name == "mixed" else K.WEIGHTS[::-1]) and set(wts) == {2, 8, 9, 16, 17, 25, 31, 32}
    assert (shifts >= 0).any(0).all() and shifts.shape == (8, 40) and Z == 65
    iters = []
    for sigma in (0.25, 0.45):
        case = K.MIXED[name, sigma]
        out, _ = K.expected(case)
        iters += out[..., 0].ravel().tolist()
        assert max(_scalar_agrees(case, _most_iterations(out))) >= 1
    print(name, "iteration counts", sorted(set(iters)))
    assert len(set(iters)) >= 3


def test_envelope_64_block_columns():
    import _ldpc_cases as K
    shifts, Z = K.code(f"nb64-{K.Z_FLOAT_64}")
    assert shifts.shape == (2, 64) and ((shifts >= 0).sum(1) == 32).all() and (shifts[:, 33:] >= 0).any() and (shifts[:, 63] >= 0).all()
    keep = shifts >= 0
    assert np.array_equal(shifts[keep], M.array_shifts(2, 64, Z)[keep])
    out = np.concatenate([K.expected(K.NB64[K.Z_FLOAT_64, sigma])[0].reshape(-1, 5) for sigma in (0.3, 0.4)])
    print("nb = 64: iters", out[:, 0].tolist(), "ok", out[:, 1].tolist())
    assert ((out[:, 0] == 100) & (out[:, 1] == 0)).any() and ((out[:, 1] == 1) & (out[:, 0] >= 1)).any()
    _scalar_agrees(K.NB64[K.Z_FLOAT_64, 0.4], [(0, 0)], 3)


@pytest.mark.parametrize("Z", [63, 64, 65, 511, 512])
def test_envelope_z_at_the_wave_boundary(Z):
    import _ldpc_cases as K
    shifts, z = K.code(f"planted-{Z}")
    assert z == Z and shifts.shape == (4, 10) and ((shifts < 0).sum(1) == 2).all() and (shifts == Z - 1).any() and (shifts == 0).any()
    iters = np.concatenate([K.expected(K.WAVE[Z, sigma])[0][..., 0].ravel() for sigma in (0.55, 0.65)])
    assert (iters >= 2).any()
    case = K.WAVE[Z, 0.65]
    if Z < 100:
        assert max(_scalar_agrees(case, _most_iterations(K.expected(case)[0]))) >= 2
    else:
        _scalar_agrees(case, [(1, 2)], 3)


@pytest.mark.parametrize("name", ["C=300", "R=40"])
def test_envelope_grid(name):
    import _ldpc_cases as K
    case, depths = K.GRID[name]
    for depth in (None,) + depths:
        out = K.expected(case, depth)[0].reshape(-1, 5)
        assert len(out) == case.R * case.C and len({tuple(o) for o in out.tolist()}) > 1, (name, depth)   # the counters tell codewords apart
    out = K.expected(case)[0]
    _scalar_agrees(case, _most_iterations(out, 3) + [(0, 0)])


def test_envelope_alpha_and_saturated_inputs():
    import _ldpc_cases as K
    for alpha in K.ALPHAS:
        out = K.expected(K.ALPHA_CASE, None, None, alpha)[0]
        assert max(_scalar_agrees(K.ALPHA_CASE, _most_iterations(out), alpha=alpha)) >= 2
    a = np.float32(0.7)                                                          # 0.7 rounds where 0.75 and 0.8125 do not
    assert float(a) * float(np.float32(1.5)) != float(a * np.float32(1.5))
    llr, bits, out, post, wrong = K.saturated()
    case = K.SATURATED_CASE
    lc, bc = K.codewords_of(case, llr), K.codewords_of(case, bits).astype(bool)
    n_inf = np.isinf(lc).sum(-1)
    assert (n_inf == 1 + (np.arange(case.R)[:, None] == wrong[0]) * (np.arange(case.C) == wrong[1])).all()
    assert ((lc < 0) != bc)[np.isinf(lc)].sum() == 1                              # every infinity has the sign of its TX bit, but one
    assert (K.code(case.code)[0] >= 0).sum(1).min() == 24                        # 22 finite |t| at least: an infinity never becomes m2
    print("saturated: iters", out[..., 0].tolist(), "NaN in post", int(np.isnan(post).sum()), "inf in post", int(np.isinf(post).sum()))
    assert not np.isnan(post).any() and np.isinf(post).sum() == n_inf.sum()
    assert out[wrong][0] == case.max_iter and out[wrong][1] == 0 and (out[..., 1] == 1).any()
    with np.errstate(invalid="ignore"):
        _scalar_agrees(case, [wrong, (0, 0)], given=(llr, bits))


def test_envelope_integer_llrs_are_exact_in_float32():
    """The float side of tests/test_ldpc_envelope_gpu.py's identity: at alpha = 1 every final value is an integer far below 2^24."""
    import _ldpc_cases as K
    llr, bits = K.integers()
    assert np.array_equal(llr, np.rint(llr)) and np.abs(llr).max() == 6 and (llr == 0).any()
    for depth in (None, 2):
        out, post = K.model(K.INTEGER_CASE, llr, bits, depth, None, 1.0)
        assert np.array_equal(post, np.rint(post)) and np.abs(post).max() < 2 ** 14
    out, _ = K.model(K.INTEGER_CASE, llr, bits, None, None, 1.0)
    _scalar_agrees(K.INTEGER_CASE, _most_iterations(out), alpha=1.0, given=(llr, bits))

"""tests/_ref_ldpc_q.py, the integer model vaeq_ldpc_decode_q is held to bit for bit (tests/test_ldpc_q_gpu.py), checked on the CPU: the
vectorised model against its independent scalar restatement on every code, noise level and parameter set; that the seeded cases reach
iters == 0, several iterations and max_iter without success; that every rule of the header binds somewhere in those cases (counted by the
model's own instrumentation); and the reason for the decoder -- scaling the LLRs changes what it decodes, and does not change what the float32
decoder decodes.  Then the cases of tests/test_ldpc_envelope_gpu.py (tests/_ldpc_cases.py): the new tables under set A and the parameter corners
held to the scalar restatement, the rule each corner is meant to bind counted by the same instrumentation (the channel clamp at scale 1e30, every
finite input erased at 1e-30, the a-posteriori clamp at app_bits == bits, f == 0 at beta = 127), and the condition of the float / fixed-point
identity: no clamp binds."""
import numpy as np
import pytest

import _ref_ldpc as M
import _ref_ldpc_q as Q

W, T0 = 12, 11


@pytest.mark.parametrize("name", sorted(Q.SETS))
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_vectorised_model_is_the_scalar_one(code, level, name):
    shifts, Z = M.CODES[code]
    n = shifts.shape[1] * Z
    llr, bits = Q.case(code, W, T0, level, name)
    lc, bc = M.codewords(llr, T0, M.C_, n), M.codewords(bits, T0, M.C_, n)
    want_out, want_post = Q.expected(code, W, T0, level, name, 20)
    seen = set()
    for r in range(M.R_):
        for c in range(M.C_):
            out, post = Q.decode_scalar(shifts, Z, lc[r, c], bc[r, c], Q.SETS[name], 20)
            assert np.array_equal(out, want_out[r, c]), (code, level, name, r, c, out, want_out[r, c])
            assert post.dtype == want_post.dtype == np.int16 and np.array_equal(post, want_post[r, c])
            seen.add(int(out[0]))
    print(code, "level", level, "set", name, "iteration counts met:", sorted(seen))


def test_one_iteration_is_the_scalar_one_too():
    shifts, Z = M.CODES["array-3-6-7"]
    llr, bits = Q.case("array-3-6-7", W, T0, 2, "B")
    lc, bc = M.codewords(llr, T0, M.C_, 42), M.codewords(bits, T0, M.C_, 42)
    for c in range(M.C_):
        a, b = Q.decode(shifts, Z, lc[0, c], bc[0, c], Q.SETS["B"], 1), Q.decode_scalar(shifts, Z, lc[0, c], bc[0, c], Q.SETS["B"], 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][0] <= 1


def test_the_quantiser():
    """Ties to even, the clamp, +-inf, NaN -> +0, and the rounding of the product before the clamp."""
    prm = dict(bits=3, scale=0.5, app_bits=5, num=6, beta=0)                          # Cmax = 3
    x = np.array([1, -1, 3, -3, 5, -5, 7, 6.9, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.99, 1.01, 100, -100], np.float32)
    assert Q.quantise(x, prm).tolist() == [0, 0, 2, -2, 2, -2, 3, 3, 3, -3, 0, 0, 0, 0, 1, 3, -3]
    for name, prm in Q.SETS.items():
        cmax, lmax = Q.limits(prm)
        assert cmax == 2 ** (prm["bits"] - 1) - 1 and lmax == 2 ** (prm["app_bits"] - 1) - 1 and lmax + cmax < 2 ** 15
        q = Q.quantise(np.array([v / prm["scale"] for v in Q.PLANTED], np.float32), prm)
        assert q.tolist() == [min(v, cmax) if v > 0 else max(v, -cmax) for v in (0, 0, 2, -2, 2, -2)] + [cmax, 0], name


@pytest.mark.parametrize("code", sorted(M.CODES))
def test_cases_cover_what_the_gpu_test_relies_on(code):
    """Under set A: codewords that pass the first test, codewords that need several iterations, codewords that end at max_iter undecoded."""
    def all_cases(level, max_iter=20):
        return np.concatenate([Q.expected(code, w, t0, level, "A", max_iter)[0].reshape(-1, 5) for w in (12, 8, 6) for t0 in (0, 11)])
    clean, mid, bad = (all_cases(level) for level in range(3))
    print(code, "sigma 0.3 iters", np.bincount(clean[:, 0]).tolist(), "| sigma 0.5 iters", np.bincount(mid[:, 0]).tolist(), "ok", int(mid[:, 1].sum()),
          "of", len(mid), "| sigma 0.8 ok", int(bad[:, 1].sum()), "of", len(bad))
    assert (clean[:, 0] == 0).any()
    assert (mid[:, 0] >= (1 if code == "array-3-6-7" else 2)).any() and (mid[:, 1] == 1).any() and (mid[:, 3] > 0).any()
    assert ((bad[:, 0] == 20) & (bad[:, 1] == 0)).any()
    one = all_cases(2, 1)
    assert (one[:, 0] <= 1).all() and ((one[:, 0] == 1) & (one[:, 1] == 0)).any()
    assert (clean[:, 4] > 0).any()                                               # erasures: the planted zeros, halves and the NaN at least


@pytest.fixture(scope="module")
def rule_counts():
    """{set: {code: {rule: count}}} over the cases at w = 12, t0 = 11, all three levels."""
    res = {}
    for name in sorted(Q.SETS):
        res[name] = {}
        for code in sorted(M.CODES):
            shifts, Z = M.CODES[code]
            st = {k: 0 for k in Q.STATS}
            for level in range(3):
                llr, bits = Q.case(code, W, T0, level, name)
                out, _ = Q.decode_batch(shifts, Z, llr, bits, T0, M.C_, Q.SETS[name], 20, 0, st)
                assert np.array_equal(out, Q.expected(code, W, T0, level, name, 20)[0])   # counting changes nothing
            res[name][code] = st
            print(name, code, st)
    return res


def test_every_rule_binds_somewhere(rule_counts):
    total = {k: sum(st[k] for per in rule_counts.values() for st in per.values()) for k in Q.STATS}
    print("over the suite:", total)
    for k in Q.STATS:
        assert total[k] > 0, k
    per_set = {name: {k: sum(st[k] for st in per.values()) for k in Q.STATS} for name, per in rule_counts.items()}
    for name, st in per_set.items():                                              # under every set
        for k in ("channel_clamp", "message_clamp", "tie_not_first", "t_zero", "half", "nan"):
            assert st[k] > 0, (name, k)
        assert st["nan"] == 3 * 3 * M.R_                                          # one per run, code and level
    assert {n for n, st in per_set.items() if st["app_clamp"] > 0} == {"A", "B", "E"}
    assert {c for c, st in rule_counts["A"].items() if st["app_clamp"] > 0} == {"irregular-5-12-80"}
    assert {n for n, st in per_set.items() if st["f_zero"] > 0} == {"B", "E"}


def test_the_scale_of_the_llrs_decides_what_decodes():
    """array-4-24-31 at sigma 0.5 under set A (5 bits, one nat per step): the LLRs as given decode more codewords than the same LLRs times
    0.25 -- what an equalizer that overestimates its noise variance fourfold hands over -- while the float32 decoder returns identical counters
    for both (0.25 is a power of two: every float32 operation scales exactly)."""
    code = "array-4-24-31"
    shifts, Z = M.CODES[code]
    llr, bits = M.case(code, W, T0, 1)
    quarter = (llr * np.float32(0.25)).astype(np.float32)
    a = Q.decode_batch(shifts, Z, llr, bits, T0, M.C_, Q.SETS["A"])[0]
    b = Q.decode_batch(shifts, Z, quarter, bits, T0, M.C_, Q.SETS["A"])[0]
    fa, fb = M.decode_batch(shifts, Z, llr, bits, T0, M.C_)[0], M.decode_batch(shifts, Z, quarter, bits, T0, M.C_)[0]
    print(f"fixed point: {int(a[..., 1].sum())} of {a[..., 1].size} decode as given, {int(b[..., 1].sum())} times 0.25 with {int(b[..., 2].sum())} "
          f"post-FEC bit errors; float32: {int(fa[..., 1].sum())} and {int(fb[..., 1].sum())}")
    assert b[..., 1].sum() < a[..., 1].sum()
    assert np.array_equal(fa, fb)
    assert np.array_equal(a[..., 3], fa[..., 3]) and np.array_equal(b[..., 3], fa[..., 3])   # pre_err is of the raw input


@pytest.mark.parametrize("name", sorted(Q.SETS))
@pytest.mark.parametrize("code", sorted(M.CODES))
def test_pre_err_is_the_float_decoder_s(code, name):
    shifts, Z = M.CODES[code]
    n = shifts.shape[1] * Z
    for level in range(3):
        llr, bits = Q.case(code, W, T0, level, name, False)                       # no planted NaN
        assert not np.isnan(llr).any() and np.isinf(llr).sum() == M.R_
        lc, bc = M.codewords(llr, T0, M.C_, n), M.codewords(bits, T0, M.C_, n)
        want = ((lc < 0) != bc.astype(bool)).sum(-1)                              # _ref_ldpc.decode's pre_err, without running it over an inf
        assert np.array_equal(Q.expected(code, W, T0, level, name, 20, False)[0][..., 3], want)
        with np.errstate(invalid="ignore"):
            one = M.decode(shifts, Z, lc[0, 0], bc[0, 0], 1)[0]
        assert one[3] == want[0, 0]


def test_interleaved_cases_plant_inside_the_codewords():
    import _ref_ldpc_il as IL
    for depth in IL.DEPTHS:
        llr, bits = Q.case_il("array-3-6-7", W, T0, 1, depth, "A")
        free = IL.unused(T0, M.C_, 42, W, depth)
        assert ((llr[:, free] == IL.LOUD) | (llr[:, free] == 0)).all() and not bits[:, free].any()
        cw = IL.codewords_il(llr, T0, M.C_, 42, depth)
        assert (np.isnan(cw).reshape(M.R_, -1).sum(1) == 1).all() and (np.isinf(cw).reshape(M.R_, -1).sum(1) == 1).all()
        assert np.isnan(llr).sum() == M.R_


# ------------------------------------------------------------------ the cases of tests/test_ldpc_envelope_gpu.py (tests/_ldpc_cases.py)
def _scalar_agrees(case, quant, picks, max_iter=None, extra=False, given=None):
    """The vectorised model against decode_scalar on codewords picks = [(run, codeword), ..] of a case's fixed-point inputs."""
    import _ldpc_cases as K
    shifts, Z = K.code(case.code)
    llr, bits = given or K.inputs(case, None, quant, extra)
    lc, bc = K.codewords_of(case, llr), K.codewords_of(case, bits)
    max_iter = case.max_iter if max_iter is None else max_iter
    seen = []
    for r, c in picks:
        a = Q.decode(shifts, Z, lc[r, c], bc[r, c], K.QSETS[quant], max_iter)
        b = Q.decode_scalar(shifts, Z, lc[r, c], bc[r, c], K.QSETS[quant], max_iter)
        assert np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype == np.int16 and np.array_equal(a[1], b[1]), (case, quant, r, c, a[0], b[0])
        seen.append(int(a[0][0]))
    print(case.code, "sigma", case.sigma, "set", quant, "iterations of the codewords held to the scalar model:", seen)
    return seen


def _most_iterations(out, k=2):
    import _ldpc_cases as K
    return K.most_iterations(out, k)


def test_envelope_tables_under_set_a():
    """The new tables with _ref_ldpc_q's planted values: the scalar restatement agrees, and the cases reach in fixed point what they reach in
    float32 (tests/test_ref_ldpc_host.py)."""
    import _ldpc_cases as K
    for name in ("mixed", "mixed-reversed"):
        iters = []
        for sigma in (0.25, 0.45):
            case = K.MIXED[name, sigma]
            out, _ = K.expected(case, None, "A")
            iters += out[..., 0].ravel().tolist()
            _scalar_agrees(case, "A", _most_iterations(out))
        assert len(set(iters)) >= 3, (name, iters)
    for Z in K.Z_WAVE:
        case = K.WAVE[Z, 0.65]
        out, _ = K.expected(case, None, "A")
        assert (out[..., 0] >= 2).any()
        _scalar_agrees(case, "A", _most_iterations(out) if Z < 100 else [(1, 2)], None if Z < 100 else 3)
    for name in ("C=300", "R=40"):
        case, depths = K.GRID[name]
        for depth in (None,) + depths:
            out = K.expected(case, depth, "A")[0].reshape(-1, 5)
            assert len({tuple(o) for o in out.tolist()}) > 1, (name, depth)
        _scalar_agrees(case, "A", _most_iterations(K.expected(case, None, "A")[0], 3))


def test_envelope_64_block_columns():
    """mb = 2, nb = 64 at the float decoder's largest Z and at this decoder's own: 3 n + 8 m = 208 Z bytes, 65 520 at Z = 315."""
    import _ldpc_cases as K
    assert K.Z_Q_64 == 65536 // 208 and 208 * (K.Z_Q_64 + 1) > 65536
    for Z in (K.Z_FLOAT_64, K.Z_Q_64):
        shifts, _ = K.code(f"nb64-{Z}")
        assert ((shifts >= 0).sum(1) == 32).all() and (shifts[:, 63] >= 0).all() and shifts.max() == 63
        out = np.concatenate([K.expected(K.NB64[Z, sigma], None, "A")[0].reshape(-1, 5) for sigma in (0.3, 0.4)])
        print("nb = 64, Z =", Z, "iters", out[:, 0].tolist(), "ok", out[:, 1].tolist())
        assert ((out[:, 0] == 100) & (out[:, 1] == 0)).any() and ((out[:, 1] == 1) & (out[:, 0] >= 1)).any()
        _scalar_agrees(K.NB64[Z, 0.4], "A", [(0, 1)], 3)


@pytest.mark.parametrize("quant", ["num1-beta127", "8-8", "2-2", "tiny", "huge"])
@pytest.mark.parametrize("code", ["array-3-6-7", "irregular-5-12-80"])
def test_envelope_parameter_corners_bind_their_rules(code, quant):
    import _ldpc_cases as K
    assert quant in K.CORNER_SETS and code in K.W_CODES
    prm = K.QSETS[quant]
    cmax, lmax = Q.limits(prm)
    st = {k: 0 for k in Q.STATS}
    for level in range(3):
        case = K.corner_case(code, level, quant)
        n = K.n_of(case)
        llr, bits = K.inputs(case, None, quant, True)
        assert np.isneginf(llr).sum() == np.isposinf(llr).sum() == np.isnan(llr).sum() == case.R       # -inf beside PLANTED's +inf and NaN
        assert ((llr != 0) & (np.abs(llr) < np.float32(1.2e-38))).sum() == case.R                      # the subnormal
        assert (np.signbit(llr) & (llr == 0)).sum() >= case.R                                           # -0.0
        one = {k: 0 for k in Q.STATS}
        counted = K.model(case, llr, bits, None, quant, max_iter=20, stats=one)                         # (20 iterations show every rule that 100 show)
        out, post = K.expected(case, None, quant, 0.75, True)
        if case.max_iter == 20:
            assert np.array_equal(out, counted[0]) and np.array_equal(post, counted[1])                 # counting changes nothing
        for k in Q.STATS:
            st[k] += one[k]
        L0 = Q.quantise(K.codewords_of(case, llr), prm)
        if quant == "num1-beta127":                                              # f is 0 everywhere: L never moves, whoever fails the first test runs out
            assert one["f_zero"] > 0 and np.array_equal(post, L0) and case.max_iter == 100
            assert np.array_equal(out[..., 0], np.where(out[..., 1] == 1, 0, 100)) and (out[..., 0] == 100).any()
        if quant == "tiny":                                                      # all but +-1.5, +-2.5 over the scale and +-inf, per run
            assert out[..., 4].sum() == case.R * (case.C * n - 6) and one["channel_clamp"] == 2 * case.R
            assert sorted(L0[L0 != 0].tolist()) == sorted([-cmax, -2, -2, 2, 2, cmax] * case.R)
        if quant == "huge":                                                      # the zeros, the subnormal, +-0.5 over the scale and the NaN stay 0,
            assert one["channel_clamp"] == (np.abs(L0) == cmax).sum() > 0         # +-1.5 and +-2.5 over the scale become +-2, all else clips
            assert set(np.unique(L0).tolist()) == {-cmax, -2, 0, 2, cmax} and (np.abs(L0) == 2).sum() == 4 * case.R
            cw = K.codewords_of(case, llr)
            stay = (cw == 0) | np.isnan(cw) | (np.abs(cw) < np.float32(1.2e-38)) | (np.abs(cw) == np.float32(0.5 / prm["scale"]))
            assert out[..., 4].sum() == stay.sum() >= case.R * (2 + 1 + 2 + 1)
        if quant == "2-2":
            assert set(np.unique(post).tolist()) <= {-1, 0, 1} and cmax == lmax == 1
        cap = 10 if quant == "num1-beta127" and n > 100 else case.max_iter        # (L never moves there: ten scalar iterations of 960 bits will do)
        assert max(_scalar_agrees(case, quant, _most_iterations(out), cap, extra=True)) == min(out[..., 0].max(), cap)
    print(code, quant, st)
    assert st["nan"] == 3 * M.R_
    if prm["app_bits"] == prm["bits"]:
        assert st["app_clamp"] > 0
    if quant == "huge":
        assert st["channel_clamp"] > 0 and st["message_clamp"] > 0


def test_envelope_float_is_fixed_point_where_nothing_clamps():
    """The condition of tests/test_ldpc_envelope_gpu.py's identity, on the CPU: under bits = 8, app_bits = 15, scale = 1, num = 8, beta = 0 no clamp
    binds on the integer LLRs (so f is the identity on every message), and the two models agree in every counter and final value."""
    import _ldpc_cases as K
    case, prm = K.INTEGER_CASE, K.QSETS["identity"]
    assert all(Q._f(np.arange(128), prm) == np.arange(128))
    llr, bits = K.integers()
    assert llr.shape == (2, 12, 3 + 240)
    for depth in (None, 2):
        st = {k: 0 for k in Q.STATS}
        out, post = K.model(case, llr, bits, depth, "identity", stats=st)
        fout, fpost = K.model(case, llr, bits, depth, None, 1.0)
        print("depth", depth, "iters", sorted(set(out[..., 0].ravel().tolist())), "ok", out[..., 1].ravel().tolist(), "max |post|", int(np.abs(post).max()), st)
        assert st["channel_clamp"] == st["message_clamp"] == st["app_clamp"] == st["f_zero"] == st["half"] == st["nan"] == 0
        assert np.array_equal(out, fout) and np.array_equal(fpost.astype(np.int16), post) and np.array_equal(fpost, np.rint(fpost))
        assert len(set(out[..., 0].ravel().tolist())) >= 3 and 0 < out[..., 1].sum() < out[..., 1].size and np.abs(post).max() < 128
    _scalar_agrees(case, "identity", _most_iterations(K.model(case, llr, bits, None, "identity")[0]), given=(llr, bits))

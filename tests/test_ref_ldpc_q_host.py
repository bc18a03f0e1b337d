"""tests/_ref_ldpc_q.py, the integer model vaeq_ldpc_decode_q is held to bit for bit (tests/test_ldpc_q_gpu.py), checked on the CPU: the
vectorised model against its independent scalar restatement on every code, noise level and parameter set; that the seeded cases reach
iters == 0, several iterations and max_iter without success; that every rule of the header binds somewhere in those cases (counted by the
model's own instrumentation); and the reason for the decoder -- scaling the LLRs changes what it decodes, and does not change what the float32
decoder decodes."""
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

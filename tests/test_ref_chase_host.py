"""The models of vaeq_chase_decode against each other and against what the case list claims, without a device: tests/_ref_chase.py's word() (the
specification, with a syndrome table) and word_search() (no table: the words within distance 1 by multiplication with H) agree on every codeword
of every case of n <= 20 bits; every branch counter is reached by the cases the GPU test runs, and the perfect codes never reach the two branches
they cannot; the case list covers what its docstring says; and Chase decoding does what it is for -- on a fixed seed of BPSK + AWGN the extended
(128, 120) code leaves fewer payload errors with 64 test patterns than with plain syndrome decoding, and fewer than it was given."""
import collections

import numpy as np

import _chase_cases as K
import _ref_chase as X


def test_models_agree():
    words = 0
    for case in K.CASES:
        cols, r = K.CODES[case.code]
        if len(cols) > 20:
            continue
        llr, bits = K.tensors(case)
        x, tx = X.gather(llr, case.t0, case.C, len(cols), case.depth), X.gather(bits, case.t0, case.C, len(cols), case.depth)
        want = K.expected(case)[0]
        for rr in range(case.R):
            for c in range(case.C):
                out_a, e_a = X.word(cols, case.p, case.K, x[rr, c], tx[rr, c])
                out_b, e_b = X.word_search(cols, r, case.p, case.K, x[rr, c], tx[rr, c])
                assert np.array_equal(out_a, out_b) and np.array_equal(e_a, e_b) and np.array_equal(out_a, want[rr, c]), (case.name, rr, c)
                words += 1
    print(f"{words} codewords of n <= 20 under both models")
    assert words == 16 * K.R_ * K.C_                            # four codes, four pattern counts


def test_every_branch_is_reached():
    total = collections.Counter()
    for case in K.CASES:
        out, _, _, count = K.expected(case)
        total.update(count)
        assert count["status0"] + count["status1"] + count["status2"] == case.R * case.C
        assert np.array_equal(np.bincount(out[..., 0].ravel(), minlength=3), [count[f"status{s}"] for s in range(3)])
        assert count["status1"], case.name                      # (a long code at sigma = 0.6 has no clean codeword among 21)
        if case.code in K.PERFECT:
            assert not count["status2"] and not count["no-candidate"], case.name
        if case.p == 0:
            assert not count["winner-T>0"] and not count["v-cancelled"] and not count["metric-tie"] and not count["reliability-tie"]
        assert (out[..., 4] >= 0).all() and out[..., 4].sum() >= 2 * case.R      # the +0 and the -0 of every run (a NaN is a third, rint makes more)
    print({k: total[k] for k in K.COUNTERS})
    assert all(total[k] > 0 for k in K.COUNTERS), [k for k in K.COUNTERS if not total[k]]
    assert set(total) == set(K.COUNTERS)


def test_case_list_covers_its_claims():
    cs = K.CASES
    assert len(cs) == 32 and len({c.name for c in cs}) == 32
    assert {(c.code, c.p) for c in cs} == {(code, p) for code in K.CODES for p in K.PATTERNS}
    assert {(c.w, c.depth) for c in cs} == {(w, d) for w in (1, 4, 12) for d in (0, 2, K.C_)}
    assert {(c.K == len(K.CODES[c.code][0]), c.spread) for c in cs} == {(a, b) for a in (False, True) for b in (0, 1)}
    assert {c.sigma for c in cs} == {0.45, 0.6} and {c.t0 for c in cs} == {0, 5}
    assert any(len(K.CODES[c.code][0]) % c.w and c.depth == 0 for c in cs)     # codewords that start inside a symbol
    for code, (cols, r) in K.CODES.items():
        assert len(set(cols.tolist())) == len(cols) and cols.min() >= 1 and cols.max() < 1 << r, code
    assert [len(K.CODES[c][0]) for c in K.CODES] == [7, 15, 16, 20, 100, 128, 256, 200]
    assert all(len(K.CODES[c][0]) == (1 << K.CODES[c][1]) - 1 for c in K.PERFECT)
    assert 2048 < K.STRIDE.R * -(-K.STRIDE.C // 8) < 4096 and K.STRIDE.C % 8       # more tiles than the launch has workgroups, a ragged one


def test_chase_beats_syndrome_decoding():
    case = K.AWGN
    chase, plain = K.expected(case, True)[0], K.expected(case, True, 0)[0]
    n = len(K.CODES[case.code][0])
    pre, pay6, pay0 = int(chase[..., 1].sum()), int(chase[..., 5].sum()), int(plain[..., 5].sum())
    print(f"{case.C} words of ({n}, {case.K}) at sigma {case.sigma}: {pre} errors in {case.C * n} bits ({pre / (case.C * n):.3e}); payload errors "
          f"{pay0} with p = 0 ({pay0 / (case.C * case.K):.3e}), {pay6} with p = 6 ({pay6 / (case.C * case.K):.3e})")
    assert np.array_equal(chase[..., 1], plain[..., 1]) and pre > 0
    assert pay6 < pay0 and pay6 < int(plain[..., 1].sum()) * case.K // n

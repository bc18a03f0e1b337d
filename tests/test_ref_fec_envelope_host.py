"""What tests/test_staircase_envelope_gpu.py, test_chase_envelope_gpu.py and test_tpc_envelope_gpu.py rely on, asserted without a device: the
models reach in the cases of tests/_staircase_envelope_cases.py, _chase_envelope_cases.py and _tpc_envelope_cases.py the branches and shapes
each group was built for; where an independent second model can follow (staircase chain_syn on the codes small enough for its table, Chase
word_search for n <= 20, TPC model (2) for component lengths <= 16) the two agree; planted cases give the planted outcome."""
import collections

import numpy as np
import pytest

import _chase_envelope_cases as CE
import _ref_bch as B
import _ref_chase as X
import _ref_staircase as S
import _ref_tpc as T
import _staircase_envelope_cases as SE
import _tpc_envelope_cases as TE

F = np.float32
SHAPE = -2


# ------------------------------------------------------------------ A. staircase
@pytest.mark.parametrize("group", sorted(SE.REACHED))
def test_staircase_groups_reach_every_branch(group):
    count = SE.counts(group)
    print(group, dict(count))
    assert all(count[k] > 0 for k in SE.REACHED[group]), [k for k in SE.REACHED[group] if not count[k]]


def test_staircase_long_chains_reuse_every_slot():
    """38 positions on a ring of 4 slots: the window moves 37 times, nine times round the ring.  The errors of two blocks that used one slot are
    filed apart: blocks that share a slot keep different non-zero counts."""
    for c, P, ring in zip(SE.GROUPS["long"][::2], (38, 19), (4, 3)):
        d = SE.case(c)
        assert d["pos_iters"].shape == (c.R, c.C, P) and S.n_positions(c.L, c.W) == P and c.W + 1 == ring and (P - 1) // ring >= 6
    assert (38 - 1) // 4 == 9
    for c in SE.GROUPS["long"]:
        d = SE.case(c)
        print(c.name, "pos_err", d["pos_err"][0, 0].tolist())
        assert (d["pos_err"].sum(-1) == d["out"][..., 2]).all() and len(set(d["pos_iters"].ravel().tolist())) >= 2
        if c.rate > 1:                                         # above the threshold every block keeps errors
            pe, ring = d["pos_err"].reshape(-1, c.L), c.W + 1
            assert (pe[:, :c.L // 2].sum(-1) > 0).all()
            assert all(any(row[a] and row[b] and row[a] != row[b] for a in range(ring) for b in range(a + ring, c.L, ring)) for row in pe)


def test_staircase_widest_window():
    seen = {}
    for c in SE.GROUPS["window"]:
        d = SE.case(c)
        seen[c.L] = d["pos_iters"].shape[-1]
        assert c.W == 32 and d["count"]["status1"] > 0 and (d["out"][..., 6] > 0).all()
    assert seen == {34: 3, 32: 1, 5: 1}


def test_staircase_iteration_cap():
    d = SE.case(SE.GROUPS["cap"][0])
    print("pos_iters", d["pos_iters"].tolist())
    assert d["iters"] == 100 and (d["pos_iters"] == 100).any() and (d["pos_iters"] < 100).any() and (d["out"][..., 5] == 100).any()


def test_staircase_smallest_block():
    """s = 2 lies inside the ranges of the header (vaeq_staircase_lds_bytes accepts it) but no component code exists there: parity(m, t) >= m >= 4
    = 2 s for every accepted m and t, so vaeq_staircase_decode refuses it for every m, and s = 3 with (m, t) = (4, 1) is the smallest block."""
    from vae_equalizer_amd import _native as nat
    P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call
    f = nat.lib().vaeq_staircase_decode
    for m in range(4, 11):
        assert nat.lib().vaeq_staircase_lds_bytes(m, 2, 1) > 0
        for t in (1, 2, 8):
            assert f(1, 1, 1 << 20, 12, 0, m, t, 2, 4, P, P, 1, 4, P, None, None, None, None) == SHAPE
    total = SE.counts("smallest")
    assert all(c.s == 3 and (c.m, c.t) == (4, 1) for c in SE.GROUPS["smallest"])
    assert total["status1"] > 0 and total["status2"] > 0 and total["miscorrected"] > 0 and total["bad_flips"] > 0 and total["pos-cap"] > 0


def test_staircase_table_builder_cases():
    chunks = {}
    for c in SE.GROUPS["tables"]:
        NT, q = (c.s + 63) // 64 * 64, (1 << c.m) - 1
        chunks[c.m] = (NT, -(-q // NT))
        assert 2 * c.s <= q and SE.case(c)["count"]["status1"] > 0 and SE.case(c)["count"]["status2"] > 0
    assert chunks == {10: (64, 16), 9: (256, 2), 4: (64, 1)}
    c = SE.GROUPS["tables"][2]
    assert 2 * c.s - 1 == 509 == (1 << c.m) - 3 and (c.s + 31) // 32 == 8 and c.s % 32 == 31


def test_staircase_widths_and_grid():
    for c in SE.GROUPS["widths"]:
        d = SE.case(c)
        assert d["llr"].shape == (c.R, c.w, c.t0 + -(-c.C * c.L * c.s * c.s // c.w) + c.spare) and (d["out"][..., 3] > 0).all()
    assert {(c.w, c.t0) for c in SE.GROUPS["widths"]} >= {(w, t0) for w in (1, 5, 13, 64) for t0 in (0, 11)}
    c = SE.GROUPS["widths"][-1]
    assert c.spare == 0 and c.t0 * c.w + c.C * c.L * c.s * c.s == SE.case(c)["llr"].shape[-1] * c.w
    many, runs = (SE.case(c) for c in SE.GROUPS["grid"])
    assert many["out"].shape == (1, 300, 8) and runs["out"].shape == (40, 1, 8)
    for d in (many, runs):                                     # chains that differ: an index into the wrong chain shows
        rows = d["out"].reshape(-1, 8)
        assert len({tuple(r) for r in rows.tolist()}) > len(rows) // 2


SYN = [c for g in ("long", "window", "smallest", "widths") for c in SE.GROUPS[g]] + [SE.GROUPS["tables"][3], SE.GROUPS["grid"][1]]


@pytest.mark.parametrize("c", SYN, ids=lambda c: c.name)
def test_staircase_bitmap_model_equals_syndrome_model(c):
    table = _table(c.m, c.t, c.s)
    d = SE.case(c)
    e, tx, _ = S.errors(d["llr"], d["bits"], c.t0, c.C, c.L, c.s)
    for r in range(c.R):
        for ch in range(c.C):
            fig, fin, pos_err, pos_iters = S.chain_syn(c.m, c.t, c.s, c.L, c.W, c.iters, e[r, ch], table)
            want = d["out"][r, ch]
            assert fig == (want[0], want[1], want[2], want[5], want[6], want[7]), (r, ch)
            assert np.array_equal(pos_err, d["pos_err"][r, ch]) and np.array_equal(pos_iters, d["pos_iters"][r, ch])
            assert np.array_equal(fin.reshape(-1) ^ tx[r, ch], d["hard"][r, ch].astype(bool))


_TABLES = {}


def _table(m, t, s):
    if (m, t, s) not in _TABLES:
        _TABLES[m, t, s] = B.Table(m, t, 2 * s)
    return _TABLES[m, t, s]


@pytest.mark.parametrize("mixed", (0, 1), ids=("row", "mixed"))
@pytest.mark.parametrize("m,t,s,ks", SE.PLANTED, ids=str)
def test_staircase_planted_components(m, t, s, ks, mixed):
    """A component of exactly k errors: k <= t is corrected whole (its k roots are the planted positions: six in the first packed word, the rest
    in the second), k = t + 1 is left alone.  Mixed patterns have positions in both halves of the word."""
    d, info, memo = SE.planted(m, t, s, mixed)
    print(d["name"], d["out"][0].tolist(), info)
    assert ks[-1] == t + 1 and max(ks) > 6 and [k for k, _, _ in info] == list(ks)
    for ch, (k, j, pos) in enumerate(info):
        status, flips, _ = memo[not mixed, pos]
        out = d["out"][0, ch]
        assert len(pos) == k and max(pos) < 2 * s <= 1023 and (not mixed or (min(pos) < s <= max(pos) and sum(p < s for p in pos) == SE.SHIELDED))
        if k <= t:
            assert status == 1 and sorted(flips) == list(pos)
            assert out[1] == 1 and out[2] == 0 and out[7] == 0 and out[6] == k + (SE.SHIELDED * t if mixed else 0) == out[3]
        else:
            assert status == 2 and flips == []
            assert mixed or (out[1] == 0 and out[2] == k and out[6] == 0 and out[7] == 0)


# ------------------------------------------------------------------ B. Chase
CHASE_REACHED = {
    "smallest": ("status0", "status1", "status2", "no-candidate", "v-cancelled", "winner-T>0", "metric-tie", "reliability-tie", "miscorrected"),
    "slots": ("status0", "status1", "status2", "no-candidate", "v-cancelled", "winner-T>0", "metric-tie", "reliability-tie", "miscorrected", "inf-metric"),
    "top": ("status0", "status1", "status2", "no-candidate", "winner-T>0", "miscorrected"),
    "tiles": ("status0", "status1", "status2", "no-candidate", "v-cancelled", "winner-T>0", "metric-tie", "reliability-tie", "miscorrected"),
    "widths": ("status0", "status1", "no-candidate", "v-cancelled", "winner-T>0", "metric-tie", "reliability-tie", "miscorrected", "inf-metric"),
    "payload": ("status0", "status1", "winner-T>0"), "grid": ("status0", "status1", "status2", "winner-T>0"),
}


@pytest.mark.parametrize("group", sorted(CHASE_REACHED))
def test_chase_groups_reach_their_branches(group):
    total = collections.Counter()
    for case in CE.GROUPS[group]:
        out, s_llr, _, count = CE.expected(case)
        total.update(count)
        assert out.shape == (case.R, case.C, 6) and s_llr.shape == (case.R, case.C * case.K)
        if case.code == "h3":                                  # perfect: every syndrome is a column
            assert not count["status2"] and not count["no-candidate"], case.name
    print(group, dict(total))
    assert all(total[k] > 0 for k in CHASE_REACHED[group]), [k for k in CHASE_REACHED[group] if not total[k]]


def test_chase_case_lists_cover_their_claims():
    G = CE.GROUPS
    for code, (cols, r) in CE.CODES.items():
        assert len(set(cols.tolist())) == len(cols) and cols.min() >= 1 and cols.max() < 1 << r and 3 <= len(cols) <= 256, code
    assert CE.CODES["h3"][0].tolist() == [1, 2, 3] and CE.CODES["h3"][1] == 2 and CE.CODES["e4"][0].tolist() == [1, 3, 5, 7] and CE.CODES["e4"][1] == 3
    assert {(c.code, c.p) for c in G["smallest"]} >= {("h3", 0), ("h3", 3), ("e4", 0), ("e4", 4)}
    assert {c.K for c in G["smallest"] if c.code == "h3"} == {1, 3}
    assert any(c.w == 64 and c.C * 3 == 63 and c.depth == 0 for c in G["smallest"])             # 21 codewords inside one symbol
    assert {CE.n_of(c) for c in G["slots"]} == {64, 65, 129, 192, 193, 255} and {c.p for c in G["slots"]} == {2, 4, 5}
    assert {-(-CE.n_of(c) // 64) for c in G["slots"]} == {1, 2, 3, 4}
    cols, r = CE.CODES["r256"]
    assert r == 10 and len(cols) == 256 and {1, 1023} <= set(cols.tolist())
    assert CE.TILE_WORDS == {n: min(32, 2048 // n) for n in (64, 65, 100, 129, 200)}
    for n, tw in CE.TILE_WORDS.items():
        mine = [c for c in G["tiles"] if CE.n_of(c) == n]
        assert {(bool(c.depth), c.spread) for c in mine} == {(False, 0), (False, 1), (True, 0), (True, 1)}
        assert {c.depth for c in mine} == {0, 7, 4 if tw % 3 == 0 else 3}
        assert all(2 * tw < c.C < 3 * tw and c.K < n and (not c.depth or (tw % c.depth and c.C % c.depth)) for c in mine)
    assert {(c.w, c.depth) for c in G["widths"]} == {(w, d) for w in (2, 3, 5, 7, 13, 64) for d in (0, 1, 7)} and all(c.C == 7 for c in G["widths"])
    assert {(c.K, c.spread) for c in G["payload"]} == {(K, s) for K in (1, 64) for s in (0, 1)} and all(CE.n_of(c) == 65 for c in G["payload"])
    assert {(c.R, c.C) for c in G["grid"]} == {(40, 1), (1, 1)} and any(CE.n_of(c) == 256 and c.C == 1 for c in G["grid"])


def _chase_words(case, degenerate=False):
    llr, bits = CE.tensors(case, degenerate)
    n = CE.n_of(case)
    return X.gather(llr, case.t0, case.C, n, case.depth), X.gather(bits, case.t0, case.C, n, case.depth)


def test_chase_models_agree():
    words = 0
    for case, degenerate in [(c, False) for g in CE.GROUPS for c in CE.GROUPS[g]] + [(c, True) for c in CE.DEGENERATE]:
        cols, r = CE.CODES[case.code]
        if len(cols) > 20:
            continue
        x, tx = _chase_words(case, degenerate)
        want = CE.expected(case, degenerate)[0]
        for rr in range(case.R):
            for c in range(case.C):
                out_a, e_a = X.word(cols, case.p, case.K, x[rr, c], tx[rr, c])
                out_b, e_b = X.word_search(cols, r, case.p, case.K, x[rr, c], tx[rr, c])
                assert np.array_equal(out_a, out_b) and np.array_equal(e_a, e_b) and np.array_equal(out_a, want[rr, c]), (case.name, rr, c)
                words += 1
    print(f"{words} codewords of n <= 20 under both models")
    assert words > 500


@pytest.mark.parametrize("case", CE.DEGENERATE, ids=lambda c: c.name)
def test_chase_degenerate_codewords(case):
    n, (cols, _) = CE.n_of(case), CE.CODES[case.code]
    x, tx = _chase_words(case, True)
    out = CE.expected(case, True)[0]
    for r in range(case.R):
        zeros, infs, equal = (collections.Counter() for _ in range(3))
        for c, count in ((CE.ZEROS, zeros), (CE.INFS, infs), (CE.EQUAL, equal)):
            got, _ = X.word(cols, case.p, case.K, x[r, c], tx[r, c], count)
            assert np.array_equal(got, out[r, c])
        xz = x[r, CE.ZEROS]
        assert ((xz == 0) | np.isnan(xz)).all() and out[r, CE.ZEROS, 4] == n and out[r, CE.ZEROS, 1] == tx[r, CE.ZEROS].sum()
        assert zeros["reliability-tie"] == 1
        if n >= 20:
            assert np.isnan(xz).any() and np.signbit(xz).any() and (~np.signbit(xz) & (xz == 0)).any()
        assert np.isinf(x[r, CE.INFS]).all() and out[r, CE.INFS, 1] == 2 and out[r, CE.INFS, 4] == 0 and infs["reliability-tie"] == 1
        assert infs["inf-metric"] > 0 and not infs["status0"]   # two errors of infinite reliability: every candidate costs infinity
        assert infs["status2"] or infs["metric-tie"] or infs["inf-metric"] == 1
        assert (np.abs(x[r, CE.EQUAL]) == F(2.5)).all() and out[r, CE.EQUAL, 1] == 1 + r % 3 and equal["reliability-tie"] == 1


# ------------------------------------------------------------------ C. TPC
ALL_TPC = [c for g in TE.GROUPS for c in TE.GROUPS[g]]


def test_tpc_every_stop_kind_and_the_whole_schedule():
    total = collections.Counter()
    for case in ALL_TPC + [TE.STRIDE]:
        out, _, _, ext, half, count = TE.expected(case)
        total.update(count)
        assert np.isfinite(ext).all() and (np.abs(ext) <= F(case.clip)).all(), case.name
        assert ((half >= 0).sum(-1) == out[..., 0]).all() and half.shape[-1] == 2 * case.iters
    print({k: total[k] for k in sorted(total)})
    assert all(total[k] > 0 for k in ("stop-h0", "stop-odd", "stop-even", "no-stop") + tuple(k for k in TE.K.COUNTERS))
    full, i8a, i8b = TE.GROUPS["schedule"]
    out, _, _, _, half, count = TE.expected(full)
    print(full.name, "half-iterations", out[..., 0].ravel().tolist())
    assert full.iters == 16 and (out[..., 0] == 32).any() and count["no-stop"] > 0 and (half[out[..., 0] == 32] >= 0).all()
    assert len(T.schedule(T.ALPHA, 16)) == 32
    assert ((out[..., 0] > 8) & (out[..., 0] < 32)).any()      # and a stop deep inside the continued part of the schedules
    for case in (i8a, i8b):
        out, count = TE.expected(case)[0], TE.expected(case)[5]
        assert case.iters == 8 and count["stop-even"] > 0 and ((out[..., 0] >= 3) & (out[..., 0] % 2 == 1) & (out[..., 1] == 1)).any()


def test_tpc_shapes_cover_their_claims():
    G = TE.GROUPS
    for code, (cols, r) in TE.CODES.items():
        assert len(set(cols.tolist())) == len(cols) and cols.min() >= 1 and cols.max() < 1 << r, code
    assert [TE.n_of(c) for c in G["rows"]] == [(8, 200), (8, 256), (4, 129), (8, 65), (150, 8), (192, 8)]
    for case in G["rows"] + G["waves"] + G["columns"]:         # not every block may stop at h = 0, and the model's cost stays low
        out = TE.expected(case)[0]
        assert out[..., 0].max() > 1 and case.p <= 4 and case.iters <= 3, case.name
    assert 8 * 256 <= 4096                                     # four lane slots on the 4-wave instantiation
    small = {TE.n_of(c): c for c in G["smallest"]}
    assert {(3, 3), (3, 256), (256, 3)} <= set(small) and any(c.p == 3 and (c.K1, c.K2) == (1, 1) for c in G["smallest"] if TE.n_of(c) == (3, 3))
    assert {TE.n_of(c) for c in G["waves"]} == {(65, 64), (256, 17)} and all(c.p <= 2 and c.iters <= 2 and c.C == 2 for c in G["waves"])
    assert 64 * 64 == 4096 < 65 * 64 and 256 * 17 > 4096
    for case in G["columns"]:
        (c1, r1), (c2, r2) = TE.CODES[case.col], TE.CODES[case.row]
        count = TE.expected(case)[5]
        assert r1 == r2 == 10 and len(c1) == len(c2) == 60 and {1, 1023} <= set(c1.tolist()) and {1, 1023} <= set(c2.tolist())
        assert count["status2"] > 0 and count["status1"] > 0, case.name
    assert any(c.p > 0 for c in G["columns"])
    assert [c.w for c in G["widths"]] == [2, 3, 5, 7, 13, 64]
    fit = next(c for c in G["widths"] if c.spare == 0)
    assert fit.t0 * fit.w + fit.C * 7 * 16 == TE.tensors(fit)[0].shape[-1] * fit.w
    grid = G["grid"][0]
    assert (grid.R, grid.C) == (40, 1) and len(set(grid.scale)) == 40 and TE.expected(grid)[0][..., 7].sum() > 0


def test_tpc_grid_stride_blocks_differ():
    case = TE.STRIDE
    n1, n2 = TE.n_of(case)
    out = TE.expected(case)[0]
    llr, bits, want = TE.stride()
    assert (n1, n2, case.w, case.t0, case.R, case.p, case.iters) == (65, 64, 1, 0, 1, 1, 1) and TE.STRIDE_BLOCKS == 1027 > 1024
    assert len({tuple(r) for r in out[0].tolist()}) == case.C == 5
    assert llr.shape == bits.shape == (1, 1, 1027 * n1 * n2) and want[0].shape == (1, 1027, 8) and want[3].shape == (1, 1027, n1 * n2)
    assert np.array_equal(want[0][0, 1025], out[0, 0])         # block g of the frame is block g mod 5 of the case
    assert np.array_equal(llr[0, 0, 1026 * n1 * n2:].view(np.uint32), TE.tensors(case)[0][0, 0, n1 * n2:2 * n1 * n2].view(np.uint32))


def test_tpc_beta_rule_of_the_model_is_the_header_s():
    """include/vaeq.h: beta = fl(beta_h scale_r) where that product is > 0 (a NaN, a zero and a negative product give +0), at most clip."""
    clip, count = F(6.0), collections.Counter()
    with np.errstate(over="ignore", invalid="ignore"):
        for beta_h, scale in ((0.2, 0.0), (0.2, -0.0), (0.2, -1.5), (0.2, np.nan), (0.2, -np.inf), (0.0, np.inf), (0.0, 1.0), (0.0, np.nan)):
            got = T._beta(F(beta_h), F(scale), clip, count)
            assert got == 0 and not np.signbit(got), (beta_h, scale)
        assert not count["clamp-beta"]
        for beta_h, scale in ((0.2, np.inf), (TE.FLT_MAX, 2.0), (TE.FLT_MAX, 1.0), (1.0, 9.0)):
            assert T._beta(F(beta_h), F(scale), clip, count) == clip
        assert count["clamp-beta"] == 4
        assert T._beta(F(0.2), F(1e-42), clip, count) == F(0.2) * F(1e-42) > 0      # a subnormal product is a product
        assert T._beta(F(TE.FLT_MAX), F(1e-38), clip, count) == F(TE.FLT_MAX) * F(1e-38) < clip


def test_tpc_corners():
    byname = {c.name: c for c in TE.GROUPS["corners"]}
    assert {c.alpha for c in byname.values()} >= {16.0, 0.0} and {c.beta for c in byname.values()} >= {0.0, TE.FLT_MAX}
    for case in byname.values():
        out, _, _, ext, _, count = TE.expected(case)
        assert out[..., 7].sum() > 0 and out[..., 0].max() > 1, case.name      # positions at +-beta, and a second half-iteration that reads them
    assert TE.expected(byname["betamax"])[5]["clamp-beta"] > 0 and TE.expected(byname["betamax-clip6"])[5]["clamp-beta"] > 0
    assert TE.expected(byname["alpha16-clip6"])[5]["clamp-W"] > 0
    for name in ("scales", "scales-clip6"):
        s = np.array(byname[name].scale, F)
        assert np.isnan(s).any() and np.isposinf(s).any() and (s == 0).any() and (s < 0).any()
    # beta = 0 and a scale of NaN or +inf: every position without a competitor gets a zero of the sign of its decision
    ext = TE.expected(byname["scales-beta0"])[3]
    assert (ext == 0).any() and np.signbit(ext[ext == 0]).any() and (~np.signbit(ext[ext == 0])).any()


def test_tpc_clip_corners_and_planted_blocks():
    for case in TE.GROUPS["clips"]:
        n1, n2 = TE.n_of(case)
        n = n1 * n2
        llr, bits = TE.tensors(case)
        out, _, _, _, _, count = TE.expected(case)
        x, tx = T.M.codewords(llr, case.t0, case.C, n), T.M.codewords(bits, case.t0, case.C, n)
        print(case.name, out[..., :4].tolist(), {k: count[k] for k in ("clamp-r", "clamp-W", "clamp-beta")})
        assert case.plant and case.C == 4
        assert (x[:, TE.ZEROS] == 0).all() and np.signbit(x[:, TE.ZEROS]).any() and (out[:, TE.ZEROS, 4] == n).all()
        assert (out[:, TE.ZEROS, :3] == [1, 1, 0]).all() and (out[:, TE.ZEROS, 3] == tx[:, TE.ZEROS].sum(-1)).all()   # zero towards the TX bit: clean
        assert np.isinf(x[:, TE.INFS]).all() and (out[:, TE.INFS, 3] >= 3).all() and (out[:, TE.INFS, 4] == 0).all()
        assert (out[:, TE.INFS, 0] > 1).any()
        assert (np.abs(x[:, TE.EQUAL]) == F(2.5)).all() and (out[:, TE.EQUAL, 3] >= 4).all() and (out[:, TE.EQUAL, 0] > 1).all()
        assert count["clamp-r"] >= case.R * n and count["delta-zero"] > 0
        if case.clip < 1:
            assert count["clamp-r"] >= 3 * case.R * n and count["clamp-W"] > 0 and count["clamp-beta"] > 0
    assert {c.clip for c in TE.GROUPS["clips"]} >= {2.0 ** 96, 2.0 ** -20}


TINY = [c for c in ALL_TPC if max(TE.n_of(c)) <= 16]


@pytest.mark.parametrize("case", TINY, ids=lambda c: c.name)
def test_tpc_models_agree(case):
    llr, bits = TE.tensors(case)
    out, s_llr, s_bits, ext, half, _ = TE.expected(case)
    (c1, r1), (c2, r2) = TE.CODES[case.col], TE.CODES[case.row]
    n1, n2 = len(c1), len(c2)
    n = n1 * n2
    alpha, beta = TE.schedules(case)
    scale = TE.scale_of(case)
    x, tx = T.M.codewords(llr, case.t0, case.C, n), T.M.codewords(bits, case.t0, case.C, n)
    for r in range(case.R):
        for c in range(case.C):
            with np.errstate(over="ignore", invalid="ignore"):
                o2, h2, d2, W2 = T.block2(c1, r1, c2, r2, x[r, c].reshape(n1, n2), tx[r, c].reshape(n1, n2), case.p, case.iters, alpha, beta,
                                          F(1.0) if scale is None else scale[r], case.clip, case.K1, case.K2)
            assert np.array_equal(o2, out[r, c]), (r, c, o2, out[r, c])
            assert np.array_equal(h2, half[r, c])
            assert np.array_equal(W2.ravel().view(np.uint32), ext[r, c].view(np.uint32))
            assert np.array_equal(np.where(tx[r, c].astype(bool) ^ d2.ravel(), F(-1.0), F(1.0)), s_llr[r, c * n:(c + 1) * n])
            assert np.array_equal(s_bits[r, c * n:(c + 1) * n], tx[r, c])


# ------------------------------------------------------------------ sensitivity: wrong variants of the models disagree on the case meant for them
@pytest.mark.parametrize("m,t,s,ks", SE.PLANTED, ids=str)
def test_staircase_planted_cases_catch_a_lost_second_root_word(m, t, s, ks, monkeypatch):
    """The model with every root behind the sixth dropped -- a root list whose second packed word is lost -- differs from the model on every
    planted chain of 7 .. t errors (the rest is corrected an iteration late) and on none of the others."""
    d, info, _ = SE.planted(m, t, s, 0)
    real = S.component
    monkeypatch.setattr(S, "component", lambda *a, **kw: (lambda status, flips: (status, sorted(flips)[:6]))(*real(*a, **kw)))
    e, _, _ = S.errors(d["llr"], d["bits"], d["t0"], d["C"], d["L"], s)
    for ch, (k, _, _) in enumerate(info):
        fig, _, pos_err, _ = S.chain(m, t, s, d["L"], d["W"], d["iters"], e[0, ch])
        same = fig == tuple(d["out"][0, ch, [0, 1, 2, 5, 6, 7]].tolist()) and np.array_equal(pos_err, d["pos_err"][0, ch])
        assert same == (not 6 < k <= t), (k, fig, d["out"][0, ch].tolist())


def test_chase_degenerate_cases_catch_a_reversed_tie_order():
    """The model with ties among equal |llr| falling to the larger position (the codeword, its bits and the columns reversed, the result turned
    back) differs from the model on codewords of zeros, of infinities and of one magnitude."""
    differ = collections.Counter()
    for case in CE.DEGENERATE:
        cols, K = CE.CODES[case.code][0], case.K
        x, tx = _chase_words(case, True)
        want = CE.expected(case, True)[0]
        for r in range(case.R):
            for c, name in ((CE.ZEROS, "zeros"), (CE.INFS, "infs"), (CE.EQUAL, "equal")):
                _, e = X.word(cols[::-1], case.p, K, x[r, c][::-1], tx[r, c][::-1])
                e = e[::-1]
                differ[name] += int(e.sum()) != want[r, c, 2] or int(e[:K].sum()) != want[r, c, 5]
    print(dict(differ))
    assert all(differ[k] > 0 for k in ("zeros", "infs", "equal"))

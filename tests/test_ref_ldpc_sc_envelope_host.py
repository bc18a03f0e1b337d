"""The cases of tests/test_ldpc_sc_envelope_gpu.py (tests/_ldpc_sc_envelope_cases.py) before anything on a GPU is compared with them, on the CPU:
the states fit and the largest Z are largest; the tables are the ones the groups need; the models (tests/_ref_ldpc_sc.py, tests/_ref_ldpc_sc_q.py)
reach in every group what it is aimed at; the ring models agree bit for bit with their scalar restatements on every case, shrunk where the scalar
walk would take too long; and wrong variants of the models -- a tail mask that is ignored, a column ring one slot short, edges renumbered
compactly, the weight of row 0 used for every row, an absent edge that contributes its sign -- fail the cases meant for them (the last two in
the integer model alone: the float model numbers the edges of a row block compactly by design and gives an absent edge no value at all; an
exception in a variant counts as a failure of the case).  Every test prints its figures before it asserts."""
import inspect

import numpy as np
import pytest

import _ref_ldpc as B
import _ref_ldpc_q as Q
import _ref_ldpc_sc as M
import _ref_ldpc_sc_q as S
import _ldpc_sc_envelope_cases as E

GROUPS = ("memory", "headtail", "tables", "nb32", "window32", "Z", "meet", "T", "bitmap", "iters", "q", "f")


def _results(g):
    """[(name, kind, case, expected)] of a group."""
    return [(n, kind, E.CASES[n], (E.expected_f if kind == "f" else E.expected_q)(n)) for n in E.group(g) for kind in E.CASES[n]["kinds"]]


def _edges(comp, l):
    """The edges of a full row l as the packer numbers them: (d, c, s), d descending, then c."""
    return [(d, c, int(comp[d, l, c])) for d in range(comp.shape[0] - 1, -1, -1) for c in range(comp.shape[2]) if comp[d, l, c] >= 0]


def _real(comp, l, t, Lc):
    """The numbers of the edges row block (t, l) really has: sc_mask restated."""
    return [e for e, (d, _, _) in enumerate(_edges(comp, l)) if 0 <= t - d < Lc]


def _table_ok(comp, Lc):
    """sc_pack's rule: at most 32 blocks in a full row, at least two in every row block of the chain."""
    ms, mb = comp.shape[0] - 1, comp.shape[1]
    return all(len(_edges(comp, l)) <= 32 and len(_real(comp, l, t, Lc)) >= 2 for l in range(mb) for t in range(Lc + ms))


# ------------------------------------------------------------------ the state and the tables
def test_every_state_fits_and_the_largest_Z_are_largest():
    assert set(E.CASES[n]["group"] for n in E.NAMES) == set(GROUPS)
    for n in E.NAMES:
        k = E.CASES[n]
        ms, mb, nb = E.dims(k)
        assert 1 <= ms <= 7 and 1 <= mb <= 4 and 2 <= nb <= 32 and 2 <= k["Z"] <= 512 and ms + 1 <= k["W"] <= 32 and 1 <= (k["T"] or 1) <= k["W"]
        assert 1 <= k["w"] <= 64 and 1 <= k["iters"] <= 100 and _table_ok(k["comp"], k["Lc"]), n
        for kind, f in (("f", E.lds_f), ("q", E.lds_q)):
            assert kind not in k["kinds"] or f(ms, mb, nb, k["Z"], k["W"]) <= 64 * 1024, (n, kind)
    for kind, f in (("f", E.lds_f), ("q", E.lds_q)):
        Z = E.NB32_Z[kind]
        print(f"nb = 32, {kind}: Z = {Z} takes {f(1, 2, 32, Z, 2)} bytes, Z = {Z + 1} takes {f(1, 2, 32, Z + 1, 2)}")
        assert f(1, 2, 32, Z, 2) <= 64 * 1024 < f(1, 2, 32, Z + 1, 2) and E.CASES[f"nb32-Z{Z}"]["W"] == 2 and kind in E.CASES[f"nb32-Z{Z}"]["kinds"]
    k = E.CASES["q-state-65472-app15"]
    assert E.lds_q(*E.dims(k), k["Z"], k["W"]) == 65472 < E.lds_q(*E.dims(k), k["Z"] + 1, k["W"])
    assert (k["W"] + 1) * 9 * 496 > 1 << 14                                       # more than 2^14 int16 entries in the ring of L


def test_the_tables_are_what_the_groups_need():
    weights, truncated, first_not_0, last_not_last, empty = set(), set(), 0, 0, 0
    for n in E.group("tables"):
        k = E.CASES[n]
        comp, (ms, mb, nb), Lc = k["comp"], E.dims(k), k["Lc"]
        wt = [len(_edges(comp, l)) for l in range(mb)]
        base = n[len("tables-"):].replace("-reversed", "")
        assert tuple(wt) == (E.TABLE_WEIGHTS[base][::-1] if n.endswith("reversed") else E.TABLE_WEIGHTS[base]) and len(set(wt)) == mb and mb >= 3
        weights |= set(wt)
        for l in range(mb):
            le = [sum(1 << e for e, (d, _, _) in enumerate(_edges(comp, l)) if d <= kk) for kk in range(ms + 1)]
            empty += sum(le[d] == le[d - 1] for d in range(1, ms + 1))                # no block with offset d: the two masks are the same
            for t in range(Lc + ms):
                real = _real(comp, l, t, Lc)
                truncated.add(len(real))
                first_not_0 += t < ms and real[0] > 0
                last_not_last += t >= Lc and real[-1] < wt[l] - 1
    print(f"full rows of {sorted(weights)}, row blocks of {sorted(truncated)}; {empty} (d, l) without a block; head rows whose first real edge is not "
          f"edge 0: {first_not_0}, tail rows whose last real edge is not edge wt - 1: {last_not_last}")
    assert weights >= {8, 9, 16, 17, 25, 31, 32} and min(weights) == 4 and 2 in truncated and empty >= 4 and first_not_0 and last_not_last
    # a full row of weight 2 cannot pass the table rule: row block 0 has component 0 alone, the last one component ms alone, two blocks each
    for ms in (1, 2):
        for split in ([1, 1], [2, 0], [0, 2]):
            comp = np.full((ms + 1, 1, 4), -1, np.int32)
            comp[0, 0, :split[0]], comp[ms, 0, :split[1]] = 1, 2
            assert len(_edges(comp, 0)) == 2 and not _table_ok(comp, 5)
    assert not _table_ok(np.array([[[3, -1, -1]], [[-1, 5, -1]]], np.int32), 4)   # the table tests/test_ldpc_sc_envelope_gpu.py sees refused
    assert all(E.CASES[n]["comp"][:, ::-1].tolist() == E.CASES[n + "-reversed"]["comp"].tolist() for n in E.group("tables") if n + "-reversed" in E.CASES)
    for Z in E.NB32_Z.values():
        comp = E.nb32_components(Z)
        assert [len(_edges(comp, l)) for l in range(2)] == [32, 32] and ((comp >= 0).sum((0, 1)) == 2).all() and comp.max() < Z
    k = E.CASES["memory-ms7-W8"]
    assert len(_edges(k["comp"], 0)) == 32 and _edges(k["comp"], 0)[0][0] == 7 and (k["comp"] >= 0).all() and E.dims(k) == (7, 1, 4)
    for Z in E.Z_EDGES:
        comp = E.CASES[f"Z-{Z}"]["comp"]
        assert all({0, Z - 1} <= set(comp[d].ravel().tolist()) for d in (0, 1)) and comp.max() == Z - 1


# ------------------------------------------------------------------ what the groups reach
def _reach(res):
    """Positions idle / partly used / exhausted, chains idle / decoded after work / failed, over (name, kind, case, expected) results."""
    pos, chains = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for _, _, k, r in res:
        it = r[3]
        pos += [(it == 0).sum(), ((it > 0) & (it < k["iters"])).sum(), (it == k["iters"]).sum()]
        out = r[0].reshape(-1, 6)
        chains += [(out[:, 0] == 0).sum(), ((out[:, 1] == 1) & (out[:, 0] > 0)).sum(), (out[:, 1] == 0).sum()]
    return pos, chains


@pytest.mark.parametrize("g", ("memory", "headtail", "tables", "Z", "meet", "T", "bitmap", "window32", "nb32"))
def test_a_group_has_idle_partly_used_and_exhausted_positions_and_decoded_and_failed_chains(g):
    for kind in "fq":
        pos, chains = _reach([x for x in _results(g) if x[1] == kind])
        print(f"{g} {kind}: positions idle / partly used / exhausted {pos.tolist()}, chains idle / decoded after work / failed {chains.tolist()}")
        assert pos.all() and chains[1] and chains[2]
    res = _results(g)
    assert sum(x[3][4].get("ties", 0) for x in res if x[1] == "f") + sum(x[3][4]["tie_not_first"] for x in res if x[1] == "q") > 0


def test_memory_both_rings_wrap_three_times():
    for n, kind, k, r in _results("memory"):
        ms, Lc, W = E.dims(k)[0], k["Lc"], k["W"]
        col, row = (Lc - 1) // (W + ms), (Lc + ms - 1) // W
        assert col >= 3 and row >= 3 and W in (ms + 1, ms + 1 + E.WIDE) and r[3].shape[-1] == Lc + ms - W + 1, n
        if kind == "q":
            print(f"{n}: the column ring of {W + ms} slots wraps {col} times, the row ring of {W} {row} times; counted {r[4]['ring_wraps']} over "
                  f"{r[0].shape[0] * r[0].shape[1]} chains; head rows {r[4]['head_rows']} tail rows {r[4]['tail_rows']}")
            assert r[4]["ring_wraps"] == col * r[0].shape[0] * r[0].shape[1] and r[4]["head_rows"] and r[4]["tail_rows"]
    assert {E.dims(E.CASES[n])[0] for n in E.group("memory")} == {4, 5, 6, 7}
    for n, kind, k, r in _results("window32"):
        ms, Lc = E.dims(k)[0], k["Lc"]
        assert k["W"] == 32 and (Lc - 1) // (32 + ms) >= 3 and (kind == "f" or r[4]["ring_wraps"] == (Lc - 1) // (32 + ms) * r[0].shape[0])
    assert {E.dims(E.CASES[n])[0] for n in E.group("window32")} == {1, 7}


def test_headtail_both_masks_cut_the_same_row():
    seen = 0
    for n, kind, k, r in _results("headtail"):
        (ms, mb, _), Lc, W = E.dims(k), k["Lc"], k["W"]
        both = [t for t in range(Lc + ms) if t < ms and t > Lc - 1]
        assert (len(both) > 0) == (Lc < ms) and W in (ms + 1, Lc + ms)
        assert all(_real(k["comp"], 0, t, Lc)[0] > 0 and _real(k["comp"], 0, t, Lc)[-1] < 4 * (ms + 1) - 1 for t in both)
        if kind == "q" and W == Lc + ms and Lc <= ms:         # one position, every row block truncated: the layer updates are iters x rows x mb
            updates = int(r[0][..., 0].sum()) * (Lc + ms) * mb
            twice = r[4]["head_rows"] + r[4]["tail_rows"] - updates
            print(f"{n}: {updates} layer updates, {r[4]['head_rows']} of head rows and {r[4]['tail_rows']} of tail rows: {twice} of rows that are both")
            assert twice == int(r[0][..., 0].sum()) * len(both) * mb
            seen += twice
    assert seen > 0
    assert {(E.dims(E.CASES[n])[0], E.CASES[n]["Lc"]) for n in E.group("headtail")} == {(7, 1), (7, 2), (7, 3), (7, 7), (7, 8), (4, 2), (4, 4), (4, 5)}


def test_meet_T_bitmap_and_iters_are_the_corners_they_claim():
    P = lambda n: M.positions(E.dims(E.CASES[n])[0], E.CASES[n]["Lc"], E.CASES[n]["W"])
    k = E.CASES
    assert P("meet-P1") == 1 and k["meet-P1"]["Lc"] + 2 == k["meet-P1"]["W"]
    assert P("meet-P2") == 2 and k["meet-P2"]["Lc"] + 2 == k["meet-P2"]["W"] + 1 and k["meet-P2"]["Lc"] < k["meet-P2"]["W"]
    assert P("meet-Lc-below-W") == 4 and k["meet-Lc-below-W"]["Lc"] < k["meet-Lc-below-W"]["W"]
    assert k["meet-Lc-W"]["Lc"] == k["meet-Lc-W"]["W"] and k["meet-Lc-W+1"]["Lc"] == k["meet-Lc-W+1"]["W"] + 1
    # T: every value on the same tensors, and two of them with different iterations per position, in either decoder
    assert [k[f"T-{T}"]["T"] for T in range(1, 7)] == list(range(1, 7)) and all(k[f"T-{T}"]["W"] == 6 for T in range(1, 7))
    assert all(E.inputs(f"T-{T}")[0] is E.inputs("T-1")[0] for T in range(1, 7))
    for f in (E.expected_f, E.expected_q):
        its = [f(f"T-{T}")[3].ravel().tolist() for T in range(1, 7)]
        print("pos_iters by T:", its)
        assert len({tuple(x) for x in its}) >= 2
    # min(p + T, rows) never binds before the last position, anywhere in the envelope
    assert all(P_ - 2 + W <= Lc + ms - 1 for ms in range(1, 8) for W in range(ms + 1, 33) for Lc in range(1, 90)
               for P_ in [M.positions(ms, Lc, W)] if P_ > 1)
    # the bit map: chains and column blocks that start inside a symbol, several column blocks in one symbol at w = 64, no symbol to spare
    for n in E.group("bitmap"):
        c = k[n]
        llr, bits = E.inputs(n)
        nbZ, nch = 33, E.n_chain(c)
        assert c["spare"] == 0 and c["t0"] > 0 and llr.shape == (len(c["sigmas"]), c["w"], c["t0"] + -(-c["C"] * nch // c["w"]))
        assert c["w"] == 1 or nbZ % c["w"] != 0
        free = E.unused(nch, c["C"], c["w"], c["t0"], llr.shape[-1])
        assert ((llr[:, free] == 0).sum(1) == 1).all() and (llr[:, free] <= 0).all() and not bits[:, free].any()
        inside = B.codewords(llr, c["t0"], c["C"], nch)                           # the zeros inside the chains, and not the one outside
        assert ((inside == 0).sum((1, 2)) == c["erasures"]).all()
        assert np.array_equal(E.expected_f(n)[0][..., 4], (inside == 0).sum(2))
        assert np.array_equal(E.expected_q(n)[0][..., 4], (Q.quantise(inside, c["prm"]) == 0).sum(2))
    assert {k[n]["w"] for n in E.group("bitmap")} == {1, 5, 7, 13, 64} and 33 < 64
    assert {(len(k[n]["sigmas"]), k[n]["C"]) for n in E.group("bitmap")} >= {(1, 40), (40, 1), (5, 3)}
    for f in (E.expected_f, E.expected_q):
        a, b = f("iters-100"), f("iters-1")
        print("iters-100:", a[3].tolist(), "iters-1:", b[0].tolist())
        assert (a[3] == 100).any() and k["iters-100"]["iters"] == 100 and (a[0][..., 1] == 0).all()
        assert k["iters-1"]["iters"] == 1 and (b[0][..., 2] == 0).all() and (b[0][..., 3] > 0).all() and (b[3] == 1).any()


class _Spy:
    """numpy as _ref_ldpc_sc_q sees it, keeping the argument of every np.abs: t of a layer update (decode() without stats takes no other)."""

    def __init__(self):
        self.t = []

    def __getattr__(self, name):
        return getattr(np, name)

    def abs(self, a):
        self.t.append(np.array(a))
        return np.abs(a)


def _chains(name):
    k = E.CASES[name]
    llr, bits = E.inputs(name)
    n = E.n_chain(k)
    lc, bc = B.codewords(llr, k["t0"], k["C"], n), B.codewords(bits, k["t0"], k["C"], n)
    return [(r, c, lc[r, c], bc[r, c]) for r in range(lc.shape[0]) for c in range(k["C"])]


def _spied(name, monkeypatch, chain=0):
    """t of every layer update of a case's chain, in order."""
    k = E.CASES[name]
    spy = _Spy()
    monkeypatch.setattr(S, "np", spy)
    _, _, llr, bits = _chains(name)[chain]
    S.decode(k["comp"], k["Z"], k["Lc"], llr, bits, k["W"], k["prm"], k["iters"], k["T"])
    monkeypatch.undo()
    return spy.t


def test_the_fixed_point_corners_bind(monkeypatch):
    res = {n: r for n, _, _, r in _results("q")}
    for n, r in res.items():
        print(n, E.CASES[n]["prm"], r[4], "largest |post|", int(np.abs(r[1].astype(np.int64)).max()))
    # app_bits = 15: Lmax = 16383 = the constant that stands in for an absent edge.  No L gets there: without a clamp L is the channel value plus
    # one message per check of the variable, at most Mmax (1 + (ms + 1) mb); the widest values of the envelope are 127 x 33 = 4191.
    for n in ("q-state-65472-app15", "q-head-rows-app15"):
        k, r = E.CASES[n], res[n]
        ms, mb, _ = E.dims(k)
        assert Q.limits(k["prm"]) == (127, 16383) and r[4]["app_clamp"] == 0 and r[4]["message_clamp"] > 0
        assert np.abs(r[1].astype(np.int64)).max() <= 127 * (1 + (ms + 1) * mb) <= 4191 < 16383
    assert np.abs(res["q-state-65472-app15"][1].astype(np.int64)).max() == 127 * 3 and res["q-state-65472-app15"][4]["channel_clamp"] > 17000
    assert res["q-head-rows-app15"][4]["head_rows"] > 0 and E.dims(E.CASES["q-head-rows-app15"])[0] == 4
    # app_bits = 9: the a-posteriori clamp binds at both signs, and |t| reaches Lmax + Mmax
    k, r = E.CASES["q-app9"], res["q-app9"]
    t = np.concatenate([x.ravel() for c in range(len(_chains("q-app9"))) for x in _spied("q-app9", monkeypatch, c)])
    print(f"q-app9: t from {int(t.min())} to {int(t.max())}, Lmax + Mmax = {255 + 127}; post from {int(r[1].min())} to {int(r[1].max())}")
    assert Q.limits(k["prm"]) == (127, 255) and r[4]["app_clamp"] > 0 and t.max() == 255 + 127 and t.min() == -(255 + 127)
    assert (r[1] == 255).any() and (r[1] == -255).any()
    # bits = app_bits = 2; num = 1, beta = 127: every message is zero and nothing ever changes
    assert Q.limits(E.CASES["q-bits2"]["prm"]) == (1, 1) and res["q-bits2"][4]["app_clamp"] > 0 and res["q-bits2"][4]["channel_clamp"] > 0
    k, r = E.CASES["q-messages-zero"], res["q-messages-zero"]
    assert all(Q._f(np.arange(16), k["prm"]) == 0) and r[4]["f_zero"] > 0 and (r[3] == k["iters"]).all()
    want = np.array([[Q.quantise(llr, k["prm"]) for _, c, llr, _ in _chains("q-messages-zero") if c == cc] for cc in range(k["C"])]).transpose(1, 0, 2)
    assert np.array_equal(r[1], want)
    # the planted values went in
    llr, _ = E.inputs("q-planted")
    tiny = np.float32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny and res["q-planted"][4]["nan"] == llr.shape[0]
    for r_ in range(llr.shape[0]):
        x = llr[r_]
        assert np.isnan(x).sum() == 1 and np.isposinf(x).sum() == 1 and np.isneginf(x).sum() == 1 and (x == tiny).sum() == 1
        assert ((x == 0) & np.signbit(x)).sum() == 1 and ((x == 0) & ~np.signbit(x)).sum() >= 2


@pytest.mark.parametrize("name", [n for n in E.group("q") if n.startswith("q-all-Mmax")])
def test_the_first_layer_update_is_a_head_row_with_every_real_edge_at_Mmax(name, monkeypatch):
    """The input is nothing but +-Mmax, so the first layer update of every chain -- row block 0, whose absent edges come first -- has a_e = Mmax
    on every real edge: the case in which the kernel's nidx stays on an absent edge.  The chains go on for all their iterations from there."""
    k = E.CASES[name]
    mmax, _ = Q.limits(k["prm"])
    r = E.expected_q(name)
    for _, _, llr, _ in _chains(name):
        assert (np.abs(Q.quantise(llr, k["prm"])) == mmax).all()
    absent = [_real(k["comp"], l, 0, k["Lc"])[0] for l in range(E.dims(k)[1])]
    first = _spied(name, monkeypatch)[0]
    later = sum(int((np.abs(x) >= mmax).all(axis=0).sum()) for x in _spied(name, monkeypatch)[1:])
    print(f"{name}: Mmax {mmax}, the first real edge of row block 0 is edge {absent}; t of the first update {np.unique(first).tolist()}; checks of "
          f"later updates with every real a_e = Mmax: {later}; iterations {r[3].ravel().tolist()}, post_err {r[0][..., 2].ravel().tolist()}")
    assert min(absent) > 0 and (np.abs(first) == mmax).all() and (r[0][..., 4] == 0).all() and (r[3] == k["iters"]).all() and r[4]["head_rows"] > 0
    assert later > 0


def test_the_float_cases_stay_finite_and_the_planted_one_does_not():
    worst = 0.0
    for n in E.FLOAT:
        llr, _ = E.inputs(n)
        post = E.expected_f(n)[1]
        assert not np.isnan(llr).any()
        if n == "f-planted":
            assert np.isposinf(llr).any() and np.isneginf(llr).any() and ((llr == 0) & np.signbit(llr)).any()
            assert np.isinf(post).any() and not np.isnan(post).any()
        else:
            assert np.isfinite(llr).all() and np.isfinite(post).all(), n
            worst = max(worst, float(np.abs(post).max()))
    print(f"largest |post| of a float case: {worst:.3g}")
    assert {E.CASES[n]["alpha"] for n in E.group("f")} == {0.5, 0.75, 1.0} and all(E.dims(E.CASES[n])[0] == 5 for n in E.group("f"))


@pytest.mark.parametrize("name", sorted(E.IDENTITY_CASES))
def test_the_identity_inputs_clamp_nothing(name):
    comp, Z, Lc, W, amp = E.IDENTITY_CASES[name]
    llr, bits = E.identity_inputs(name)
    assert np.array_equal(llr, np.rint(llr)) and not np.signbit(llr[llr == 0]).any() and np.abs(llr).max() == amp
    stats = S.new_stats()
    a = S.decode_batch(comp, Z, Lc, llr, bits, 7, 2, W, S.IDENTITY, 10, stats=stats)
    b = M.decode_batch(comp, Z, Lc, llr, bits, 7, 2, W, 10, 1.0)
    print(name, stats, "iters", a[0][..., 0].tolist(), "ok", a[0][..., 1].tolist(), "pre_err", a[0][..., 3].tolist(), "largest |post|", np.abs(a[1]).max())
    assert stats["channel_clamp"] == stats["message_clamp"] == stats["app_clamp"] == stats["half"] == stats["nan"] == 0
    assert (a[0][..., 0] > 0).all() and (a[0][..., 3] > 0).all() and stats["tie_not_first"] > 0 and stats["head_rows"] > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].astype(np.float32), b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert comp.shape[0] - 1 == 7 or comp.shape[1] == 4


# ------------------------------------------------------------------ the ring models against their scalar restatements
SCALAR_WORK = 160_000                                          # edge updates of the scalar walk, at most


def _shrunk(k):
    """The longest chain of at most W + ms + 1 positions whose scalar walk stays within SCALAR_WORK, or None."""
    (ms, mb, _), Z, W = E.dims(k), k["Z"], k["W"]
    weight = max(len(_edges(k["comp"], l)) for l in range(mb))
    for Lc in range(min(k["Lc"], W + ms + 1), 0, -1):
        if M.positions(ms, Lc, W) * min(k["iters"], 10) * min(W, Lc + ms) * mb * Z * weight <= SCALAR_WORK and _table_ok(k["comp"], Lc):
            return Lc
    return None


@pytest.mark.parametrize("g", GROUPS)
def test_the_two_restatements_agree(g):
    done = skipped = 0
    for n in E.group(g):
        k = E.CASES[n]
        Lc = _shrunk(k)
        if Lc is None:
            skipped += 1
            continue
        nbits = Lc * k["comp"].shape[2] * k["Z"]
        _, _, llr, bits = _chains(n)[-1]                        # the noisiest run
        llr, bits = llr[:nbits], bits[:nbits]
        iters = min(k["iters"], 10)
        with np.errstate(invalid="ignore"):
            if "f" in k["kinds"]:
                a = M.decode(k["comp"], k["Z"], Lc, llr, bits, k["W"], iters, k["alpha"], k["T"])
                b = M.decode_scalar(k["comp"], k["Z"], Lc, llr, bits, k["W"], iters, k["alpha"], k["T"])
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and a[1].dtype == b[1].dtype == np.float32, n
                assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) or np.isnan(a[1]).any(), n
            if "q" in k["kinds"]:
                a = S.decode(k["comp"], k["Z"], Lc, llr, bits, k["W"], k["prm"], iters, k["T"])
                b = S.decode_scalar(k["comp"], k["Z"], Lc, llr, bits, k["W"], k["prm"], iters, k["T"])
                assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].dtype == b[1].dtype == np.int16, n
        done += 1
    print(f"{g}: {done} cases walked edge by edge (chains of at most W + ms + 1 positions), {skipped} too large for the scalar walk")
    assert done > 0


# ------------------------------------------------------------------ wrong variants of the models fail the cases meant for them
def _variant(mod, *edits):
    """mod.decode with pieces of its text replaced: a patched copy that lives in this test alone."""
    src = inspect.getsource(mod.decode)
    for old, new in edits:
        assert old in src, old
        src = src.replace(old, new)
    ns = dict(vars(mod))
    exec(src, ns)
    return ns["decode"]


def _differing(decode, name, kind):
    """In how many chains of a case a variant differs from the model in out, post, pos_err or pos_iters (an exception counts)."""
    k = E.CASES[name]
    want = (E.expected_f if kind == "f" else E.expected_q)(name)
    tail = (k["iters"], k["alpha"], k["T"]) if kind == "f" else (k["prm"], k["iters"], k["T"])
    bad = 0
    for r, c, llr, bits in _chains(name):
        try:
            with np.errstate(invalid="ignore"):
                got = decode(k["comp"], k["Z"], k["Lc"], llr, bits, k["W"], *tail)
            bad += not all(np.array_equal(x, w[r, c]) for x, w in zip(got, want[:4]))
        except (ValueError, IndexError):
            bad += 1
    return bad, len(_chains(name))


TAIL = ("if 0 <= t - d < Lc", "if 0 <= t - d")
RING = ("nb * Z, W + ms, Lc + ms", "nb * Z, W + ms - 1, Lc + ms")
WT0 = ("    Lr, Br = np.zeros(ring", "    full = [f[:len(full[0])] for f in full]\n    Lr, Br = np.zeros(ring")
COMPACT = ('idx = s["E"][k]', "idx = k")
ABSENT = (("head=E[0] > 0", "absent=(len(full[l]) - len(E)) & 1, head=E[0] > 0"), ('^ s["sigma"]\n', '^ s["sigma"] ^ bool(s["absent"])\n'))
VARIANTS = [
    ("a tail mask that is ignored", (TAIL,), "fq", ("meet-Lc-W+1", "headtail-ms7-Lc2-W8", "tables-t4-ms2", "memory-ms4-W5")),
    ("a column ring of W + ms - 1 slots", (RING,), "fq", ("memory-ms4-W5", "memory-ms7-W12", "tables-t4-ms1", "window32-ms1")),
    ("the wt of row 0 for every row", (WT0,), "fq", ("tables-t4-ms1", "tables-t4-ms2", "tables-t3-ms3-reversed")),
    ("edges renumbered compactly in truncated rows", (COMPACT,), "q", ("q-head-rows-app15", "headtail-ms7-Lc7-W8", "tables-t3-ms3")),
    ("an absent edge that contributes its sign", ABSENT, "q", ("meet-Lc-W+1", "tables-t3-ms3", "bitmap-w7")),
]


@pytest.mark.parametrize("what,edits,kinds,names", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_a_wrong_variant_of_the_model_fails_its_cases(what, edits, kinds, names):
    for kind in kinds:
        wrong, right = _variant(M if kind == "f" else S, *edits), _variant(M if kind == "f" else S)
        for n in names:
            bad, total = _differing(wrong, n, kind)
            print(f"{what}, {kind}, {n}: differs in {bad} of {total} chains")
            assert bad > 0 and _differing(right, n, kind)[0] == 0                 # and the unpatched copy is the model

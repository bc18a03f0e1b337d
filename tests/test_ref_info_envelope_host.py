"""The preconditions of tests/test_info_envelope_gpu.py and tests/test_awgn_info_envelope_gpu.py, asserted on the CPU for every case of
tests/_info_envelope_cases.py: the kept counts are the ones the case tables state (no window is empty, or full, by accident), every compared
q-mode logarithm has an argument of at least 1e-30, every y-mode decision a top-two posterior gap at or above its pair's floor, every
hypothesis wins somewhere at every n_lev of every pair, the planted ties tie, the planted TX samples round as worked out by hand, and the float32
restatement of the CMA figures with the radii summed in the kernel's order stays where the pairwise one is.
"""
import numpy as np
import pytest

import _info_envelope_cases as K
import _ref_awgn_baseline_info as T
import _ref_awgn_info as A
import _ref_cma_info as C
import _ref_epilogue as E
import _ref_info as I


@pytest.mark.parametrize("name", list(K.DP))
def test_dp_cases_keep_what_the_table_says_and_meet_the_floors(name):
    xs, mq, my = K.dp(name)
    assert len(xs) <= 8 and len({(x["q"].shape, x["batch_len"]) for x in xs}) == 1
    for x, a, b, kept in zip(xs, mq, my, K.DP_KEPT[name]):
        assert a["kept"].tolist() == [kept, kept] and b["kept"].tolist() == [kept, kept], (name, a["kept"], kept)
        assert K.dp_floors_ok(a, b)
        if kept:
            assert a["min_post"] >= I.MIN_POST_FLOOR and b["qgap"] >= E.QGAP_FLOOR
    if name.startswith("clamp"):
        for x in xs:
            assert [K.clamp(w) for w in x["wild"]] == x["shift"].tolist() and any(abs(int(w)) > 10 for w in x["wild"])


def test_dp_special_runs():
    """B1-N64 keeps something at shift[0] = -10 alone; the run with shift (0, -7) of B20-N60 keeps one symbol and two hypotheses tie on it; the
    stride base runs differ in everything a run can differ in."""
    assert K.DP_KEPT["B1-N64"] == [32, 0, 0, 0, 0] and [x["shift"][0] for x in K.dp("B1-N64")[0]] == [-10, -9, 0, 5, 10]
    xs, mq, _ = K.dp("B20-N60")
    assert xs[5]["shift"].tolist() == [0, -7] and mq[5]["kept"].tolist() == [1, 1]
    for p in range(2):
        c = mq[5]["cnt"][:, p]
        assert c.min() == 0 and (c == 0).sum() == 2 and mq[5]["hyp"][p] == np.flatnonzero(c == 0)[0]
    assert 0 in K.DP_KEPT["B20-N60"] and max(K.DP_KEPT["B20-N60"]) > 20          # empty and kept runs in one launch
    xs = K.dp("stride")[0]
    for k in ("shift", "r", "hyp", "var"):
        assert len({str(np.asarray(x[k]).tolist()) for x in xs}) == (2 if k == "r" else 3), k
    assert xs[16384 % 3] is xs[1]                                               # 16385 = 3 * 5461 + 2: the last run is base run 1, not base run 0


@pytest.mark.parametrize("name", list(K.CMA))
def test_cma_cases(name):
    xs, ms = K.cma(name)
    assert len(xs) <= 8
    for x, m, kept in zip(xs, ms, K.CMA_KEPT[name]):
        assert m["kept"].tolist() == [kept, kept] and m["qgap"] >= E.QGAP_FLOOR and C.planted_recovered(x, m)


def test_cma_extremes_cover_all_sixteen_shift_pairs_and_all_four_exchanges():
    xs = K.cma("extremes0-n8")[0] + K.cma("extremes1-n2")[0]
    assert len({(tuple(x["shift_c"]), tuple(x["shift_q"])) for x in xs}) == 16
    assert {(x["r_c"], x["r_q"]) for x in xs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    every = [x for name in K.CMA for x in K.cma(name)[0]]
    assert {bool(x["s"] != 1 and sc) for x, sc in zip(every, [s["scale_edges"] for name in K.CMA for s in K.CMA[name]])} == {True, False}


@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_cases(name):
    xs, mq, my = K.awgn(name)
    short = {f"N{N}-s{sh}": kept for N, sh, kept in K.AWGN_SHORT}
    want = [short[name]] * 3 if name in short else K.AWGN_KEPT[name]
    assert len(xs) <= 8 and [m["kept"] for m in mq] == want and [m["kept"] for m in my] == want
    for x, a, b in zip(xs, mq, my):
        assert A.meets_floors(x, a, b)
        if a["kept"]:
            assert a["min_post"] >= A.MIN_POST_FLOOR and b["qgap"] > A.QGAP_FLOOR and b["margin"] >= A.MARGIN_FLOOR


@pytest.mark.parametrize("name", list(K.TRACK))
def test_track_cases(name):
    xs, ms = K.track(name)
    if name.startswith("wild"):
        want = K.TRACK_WILD_KEPT[name[:-4]]
    else:
        want = [{(Nd, e, sh): kept for Nd, e, sh, kept in K.TRACK_GEOM}[(xs[0]["tx"].shape[-1], xs[0]["edge"], xs[0]["shift"])]] * 2
    assert [m["kept"] for m in ms] == want
    for x, m in zip(xs, ms):
        assert T.meets_floors(x, m) and len(x["z"]) - x["tx"].shape[-1] in (0, 1)


def test_every_hypothesis_wins_somewhere_at_every_n_lev():
    """Among the runs that keep more than ten symbols (fewer decide nothing), per pair and n_lev."""
    won = {}
    for pair, names, get, nh in (("dp", K.DP, lambda n: K.dp(n)[1:], 8), ("cma", K.CMA, lambda n: K.cma(n)[1:], 8),
                                 ("awgn", K.AWGN, lambda n: K.awgn(n)[1:], 4), ("track", K.TRACK, lambda n: K.track(n)[1:], 4)):
        for name in names:
            xs = {"dp": K.dp, "cma": K.cma, "awgn": K.awgn, "track": K.track}[pair](name)[0]
            for models in get(name):
                for x, m in zip(xs, models):
                    if np.min(m["kept"]) > 10:
                        won.setdefault((pair, x["n"]), set()).update(int(h) for h in np.atleast_1d(m["hyp"]))
        for n in (2, 4, 8):
            assert won[(pair, n)] == set(range(nh)), (pair, n, won[(pair, n)])


# ------------------------------------------------------------------ planted edges
def test_tx_levels_round_half_to_even_and_clamp():
    for n in (2, 4, 8):
        tx, want = K.off_grid_tx(n)
        assert I.tx_levels(tx, n).tolist() == want.tolist() and A.tx_levels(tx, n).tolist() == want.tolist(), n
        f32 = np.float32(0.5 * (n - 1))                                          # info_tx_level's own arithmetic, in float32
        assert np.clip(np.rint(f32 * tx.astype(np.float32) + f32), 0, n - 1).astype(int).tolist() == want.tolist(), n
    assert I.tx_levels(np.float16(0.0), 2) == 0 and A.tx_levels(np.float16(0.0), 2) == 0      # 0.5 rounds to even
    assert K.HALF_ULP_4[1] == np.nextafter(K.HALF_ULP_4[0], np.float16(1)) and K.HALF_ULP_8[1] == np.nextafter(K.HALF_ULP_8[0], np.float16(1))


@pytest.mark.parametrize("pair", ["dp", "awgn"])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_planted_posterior_ties_are_equal_floats_and_the_first_maximum_errs(pair, n):
    x, m = (K.planted_dp if pair == "dp" else K.planted_awgn)(f"posterior-tie-n{n}")
    q = x["q"].reshape(-1, 2, n, 60)                                             # [pol][axis][level][symbol]
    lev = I.tx_levels(x["tx"], n).reshape(-1, 2, 60)
    errs = 0
    for k, pos in enumerate(K.PLANTED_POS):
        p, c = divmod(k % (2 * len(q)), 2)
        col = q[p, c, :, pos]
        top = np.flatnonzero(col == col.max())
        assert col.dtype == np.float32 and len(top) == 2 and top[1] == top[0] + 1 and lev[p, c, pos] in top
        errs += lev[p, c, pos] == top[1]                                         # the first maximum is the wrong level
    assert errs >= 2 and m["qgap"] == 0.0 and np.min(m["kept"]) == 38


def test_planted_hypothesis_ties():
    for name, (h1, h2, n) in K.DP_TIES.items():
        x, m = K.planted_dp(name)
        for p in range(2):
            c = m["cnt"][:, p]
            assert 0 < h1 < h2 and c[h1] == c[h2] == c.min() and (c == c.min()).sum() == 2 and m["hyp"][p] == h1
    assert sum(h2 >= 4 for _, h2, _ in K.DP_TIES.values()) >= 1
    for name, (h1, h2, n) in K.AWGN_TIES.items():
        x, m = K.planted_awgn(name)
        c = m["cnt"]
        assert 0 < h1 < h2 and c[h1] == c[h2] == c.min() and (c == c.min()).sum() == 2 and m["hyp"] == h1
    m = K.planted_dp("pmf-one-level-n2")[1]                                      # one symbol throughout: hypotheses 0 and 7 tie
    assert (m["cnt"][0] == m["cnt"][7]).all() and m["hyp"].tolist() == [0, 0]


@pytest.mark.parametrize("pair", ["dp", "awgn"])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_planted_subnormals_cost_126_bit(pair, n):
    """A subnormal posterior, or a set of them, is below FLT_MIN: the model charges log2 FLT_MIN = -126 bit, as for an exact zero."""
    x, m = (K.planted_dp if pair == "dp" else K.planted_awgn)(f"subnormal-n{n}")
    assert 0 < m["min_post"] < I.FLT_MIN
    z = dict(x, q=np.where(x["q"] < I.FLT_MIN, np.float32(0), x["q"]))
    mz = I.info_q(z["q"], z["tx"], z["P"], z["shift"], z["r"], None) if pair == "dp" else A.info_q(z["q"], z["tx"], z["P"], z["shift"])
    assert np.array_equal(np.asarray(mz["AIR"]), np.asarray(m["AIR"])) and np.array_equal(np.asarray(mz["GMI"]), np.asarray(m["GMI"]))
    assert np.all(np.asarray(m["AIR"]) < -126.0 * 2 / 38)


@pytest.mark.parametrize("name", [k for k in K.PLANTED_DP if not k.startswith("posterior-tie")] + list(K.DP_TIES))
def test_planted_runs_keep_a_dominant_posterior(name):
    """What lets the GPU tests compare the LLR signs with bit_err: in the models, the signs of the LLRs are the bits of the decisions."""
    import _ref_llr as L
    x, m = K.planted_dp(name)
    planes, mask = L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], m["hyp"], None)
    bits = L.label_bits(x["tx"], x["n"])
    assert [L.sign_errors(planes[p], bits[p], mask[p]) for p in range(2)] == m["bit_err"].tolist()
    if name in K.PLANTED_AWGN or name in K.AWGN_TIES:
        x, m = K.planted_awgn(name)
        planes, mask = L.awgn_llr_q(x["q"], x["n"], x["shift"], m["hyp"])
        assert L.sign_errors(planes, L.label_bits(x["tx"], x["n"]), mask) == m["bit_err"]


@pytest.mark.parametrize("pair", ["dp", "awgn"])
def test_planted_pmfs(pair):
    for n in (2, 4, 8):
        get = K.planted_dp if pair == "dp" else K.planted_awgn
        z, one = get(f"pmf-zeros-n{n}")[0]["P"], get(f"pmf-one-level-n{n}")[0]["P"]
        assert (z == 0).any() and abs(z.sum() - 1) < 1e-6 and sorted(one.tolist())[-2:] == [0.0, 1.0] and I.entropy(one) == 0.0
        assert I.entropy(z) == (1.0 if n > 2 else 0.0)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_far_samples_decide_the_outer_level(n):
    x, m = K.far_dp(n)
    assert m["qgap"] >= E.QGAP_FLOOR and m["sym_err"].tolist() == [0, 0] and np.isfinite(m["AIR"]).all() and np.isfinite(m["GMI"]).all()
    assert (np.abs(x["y"][:, :, list(K.PLANTED_POS)]) == 50).all() and (x["var"] == np.float32(1e-6)).all()
    lev = I.tx_levels(x["tx"], n)[:, :, list(K.PLANTED_POS)]
    assert np.isin(lev, (0, n - 1)).all()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_far_awgn_samples_leave_the_scales_alone(n):
    x, m = K.far_awgn(n)
    yh = A.normalised(x["y"], x["amp_mean"])
    assert np.allclose(np.abs(yh[0, list(K.PLANTED_POS)]), 50.0, rtol=1e-5) and (np.abs(yh[1, list(K.PLANTED_POS)]) > 45).all()
    assert m["sym_err"] == 0 and m["kept"] == 38 and m["qgap"] > A.QGAP_FLOOR and m["margin"] >= A.MARGIN_FLOOR and np.isfinite(m["GMI"])
    assert x["var"] == np.float32(1e-6)


def test_cma_float32_restatement_in_the_kernels_order_is_pinned():
    """float32_deviation(ordered=True) sums the radii as cma_radius_factor does; over the envelope cases it stays within the float64 model by
    what the pairwise restatement does, and both are printed."""
    worst = {False: 0.0, True: 0.0}
    for name in K.CMA:
        for x in K.cma(name)[0]:
            for o in worst:
                worst[o] = max(worst[o], C.float32_deviation(x, ordered=o))
    print(f"CMA float32 restatement over the envelope cases: pairwise {worst[False]:.3e} bit, in the kernel's order {worst[True]:.3e} bit")
    assert worst[True] <= 2e-5 and worst[True] <= 2 * worst[False]               # 1.4e-5 at 14 kept 16-QAM symbols (N46 run 3)
    x = K.cma("N43")[0][0]
    W = C.window_c(43, x["shift_c"])
    rad = np.abs(np.random.default_rng(1).normal(size=(2, W.stop - W.start))).astype(np.float32)
    assert abs(float(C._radius_sum(rad, W.start)) - rad.astype(np.float64).sum()) <= 1e-5

"""The float64 model of vaeq_cma_epilogue_info (tests/_ref_cma_info.py) and the launch grid of tests/test_cma_info_gpu.py, checked on the host:
the preconditions of an exact count comparison with a float32 kernel, the model against what it is composed of and against a closed form, that the
grid can see the unscaled frame edges, and what the float32 format costs the kernel's operation order (CMA_DEV, the unit of the GPU test's bound)."""
import numpy as np
import pytest

import _ref_cma_info as C
import _ref_epilogue as E
import _ref_info as I


def _all_runs():
    for name in C.LAUNCHES:
        xs, ms = C.build_launch(name)
        for x, m in zip(xs, ms):
            yield name, x, m


def test_grid_is_the_one_the_issue_sets():
    specs = [s for name in C.LAUNCHES for s in C.launches()[name]]
    assert len(C.LAUNCHES) == 12 and len(specs) == 36
    assert {s["N"] for s in specs} == {43, 47, 400, 1030} and {s["n"] for s in specs} == {2, 4, 8}
    assert {s["shift_c"] for s in specs} == {(-10, 0), (0, 10), (10, -10)} and {s["shift_q"] for s in specs} == {(0, 0), (2, -1), (-3, 3)}
    assert {s["r_c"] for s in specs} == {0, 1} and {s["r_q"] for s in specs} == {0, 1} and {s["hyp"] for s in specs} == set(range(8))
    assert {s["s"] for s in specs} == {0.8, 1.25, 0.6} and {s["nu"] for s in specs} == {0.0, I.NU_SHAPED}
    # the runs the agreement test with the epilogue uses exist for both long rows
    sel = [s for s in specs if s["shift_q"] == (0, 0) and s["r_q"] == 0 and s["N"] >= 400]
    assert {s["N"] for s in sel} == {400, 1030} and all(s["r_c"] == 0 for s in sel) and len({s["shift_c"] for s in sel}) == 3
    assert {(s["r_c"], s["r_q"]) for s in specs} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_floors_and_planted_counts():
    worst = np.inf
    for name, x, m in _all_runs():
        worst = min(worst, m["qgap"])
        assert m["qgap"] >= E.QGAP_FLOOR, (name, m["qgap"])
        N = x["y"].shape[-1]
        kept = N - 2 * E.EDGE - int(np.abs(x["shift_q"]).max())
        assert (m["kept"] == kept).all() and kept > 0, (name, m["kept"])
        for p in range(2):
            assert m["sym_err"][p] == x["n_err"][p] and m["hyp"][p] == x["hyp"], (name, p, m["sym_err"], x["n_err"], m["hyp"], x["hyp"])
        assert m["bit_err"].min() >= m["sym_err"].min() and np.isfinite(m["GMI"]).all() and np.isfinite(m["AIR"]).all()
        assert abs(m["fac"] / x["s"] - 1) < (0.06 if N >= 400 else 0.25), (name, m["fac"], x["s"])
    print(f"smallest top-two posterior gap over the grid: {worst:.3f} (floor {E.QGAP_FLOOR})")


@pytest.mark.parametrize("n,shift_q,r_q", [(8, (2, -1), 1), (4, (-3, 3), 0), (2, (0, 0), 1)])
def test_composition_with_unit_factor_is_info_y(n, shift_q, r_q):
    """shift_c = 0, r_c = 0 and a y whose mean radius over W_c is TX's: the model is _ref_info.info_y on the same input."""
    x = I.make_run(seed=31 + n, N=300, n=n, shift=shift_q, r=r_q, hyp=5, batch_len=None, nu=I.NU_SHAPED, var=(0.004, 0.005), n_err=(2, 3))
    y0, W = np.asarray(x["y"], np.float64), C.window_c(300, (0, 0))
    t = np.asarray(x["tx"], np.float64)[..., W]
    y = y0 * (np.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2).sum() / np.sqrt(y0[:, 0, W] ** 2 + y0[:, 1, W] ** 2).sum())
    m = C.info(y, x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], (0, 0), 0, x["shift"], x["r"])
    ref = I.info_y(y, x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], None)
    assert abs(m["fac"] - 1) < 1e-14
    for k in C.CNT:
        assert np.array_equal(m[k], ref[k]), k
    for k in C.FIG:
        assert np.abs(m[k] - ref[k]).max() < 1e-9, k


def test_noise_free_uniform_4qam_carries_2_bit():
    rng = np.random.default_rng(5)
    amp = E.amp_levels(2)
    tx = amp[rng.integers(0, 2, (2, 2, 200))].astype(np.float16)
    tx64 = np.asarray(tx, np.float64)
    for shift_c, r_c, s in (((0, 0), 0, 1.0), ((3, -2), 1, 0.7)):
        y = I.channel(tx64 / s, r_c, np.asarray(shift_c))
        m = C.info(y, tx, np.full(2, 0.5), amp, 0.0, (0.004, 0.004), shift_c, r_c, (0, 0), 0)
        print(f"4-QAM noise-free, shift_c {shift_c} r_c {r_c} s {s}: fac {m['fac']:.6f} AIR {m['AIR']} GMI {m['GMI']} BER {m['BER']}")
        assert np.abs(m["AIR"] - 2).max() < 1e-6 and np.abs(m["GMI"] - 2).max() < 1e-6 and (m["BER"] == 0).all() and (m["sym_err"] == 0).all()
        assert np.abs(m["NGMI"] - 1).max() < 1e-6 and (m["hyp"] == 0).all()


def test_zero_radius_is_no_measurement():
    x = C.build_launch("N47-n4")[0][0]
    m = C.info(np.zeros_like(x["y"]), x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift_c"], x["r_c"], x["shift_q"], x["r_q"])
    assert all(np.isnan(m[k]).all() for k in C.FIG) and all(not m[k].any() for k in C.CNT)


def test_grid_sees_the_unscaled_edge():
    """shift_q != 0 and s = 0.6: kept symbols whose stage-c index lies outside W_c stay unscaled.  A model that scaled them too counts other symbol
    errors on the grid's own run, and on the run whose edges were built scaled the true model does."""
    name, k = next((nm, i) for nm in C.LAUNCHES for i, sp in enumerate(C.launches()[nm])
                   if sp["s"] == 0.6 and sp["shift_q"] == (-3, 3) and sp["n"] == 8)
    x, m = C.build_launch(name)[0][k], C.build_launch(name)[1][k]
    N = x["y"].shape[-1]
    W = C.window_c(N, x["shift_c"])
    idx = np.stack([E.kept_indices(N, x["shift_q"], None) + int(x["shift_q"][p]) for p in range(2)])
    outside = int(((idx < W.start) | (idx >= W.stop)).sum())
    ya = E.align(np.asarray(x["y"], np.float64), x["shift_c"], x["r_c"])
    wrong = I.info_y(ya * m["fac"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift_q"], x["r_q"], None)
    print(f"{name} run {k}: {outside} kept samples outside W_c; sym_err {m['sym_err']} with the edge unscaled, {wrong['sym_err']} when it is scaled too")
    assert outside > 0 and not np.array_equal(wrong["sym_err"], m["sym_err"])
    spec = dict(C.launches()[name][k])
    y2 = C.make_run(scale_edges=True, **spec)
    m2 = C.model(y2)
    assert not np.array_equal(m2["sym_err"], np.asarray(spec["n_err"]))


def test_float32_deviation_is_bounded_by_cma_dev():
    worst, where = 0.0, None
    for name, x, m in _all_runs():
        d = C.float32_deviation(x)
        if d > worst:
            worst, where = d, name
    print(f"largest float32 deviation of the kernel's operation order from the model: {worst:.3e} bit ({where}); CMA_DEV = {C.CMA_DEV:.1e}")
    assert worst <= C.CMA_DEV
    assert C.CMA_DEV <= 2 * worst                               # recorded, not padded

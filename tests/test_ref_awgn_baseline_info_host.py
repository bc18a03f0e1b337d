"""The float64 model of the AWGN baselines' information-rate figures (tests/_ref_awgn_baseline_info.py) against the second, independently written
model of the same decisions (tests/_ref_awgn.py: ser on the reference's own slices, dfe), the window arithmetic against the reference's Python
slices, and the preconditions the GPU cases of tests/test_awgn_baseline_info_gpu.py rely on: every normalised sample of the slice at least 0.05
level spacings from a threshold, a top-two posterior gap above 0.05, posteriors at the transmitted level >= 1e-30.  It also computes Z_DEV, the
cost of the float32 format the GPU bound is built on."""
import numpy as np
import pytest

import _ref_awgn as R
import _ref_awgn_baseline_info as B
import _ref_awgn_info as A


@pytest.mark.parametrize("e,dz", [(11, 0), (31, 0), (31, 1)])
def test_window_is_the_reference_slices(e, dz):
    """z[:, e+sh : -e] against data[:, e : -e-sh] (func_CMA_MQAM_shaping.py:231, DFE_MQAM_shaping.py:282, :293): where the data slice holds a
    positive number of symbols the window is those slices; everywhere else it is empty."""
    for Nd in (2 * e + 1, 2 * e + 2, 2 * e + 13, 400):
        zi, di = np.arange(Nd + dz), np.arange(Nd)
        for sh in range(-e - 2, 14):
            zs, ds = zi[e + sh:-e], di[e:-e - sh]
            ri, ti = B.window(Nd + dz, Nd, e, sh)
            if e + sh <= 0 or Nd - 2 * e - sh <= 0:
                assert len(ri) == 0 and len(ti) == 0, (Nd, sh)
                assert len(ds) == 0 or len(zs) == 0 or e + sh <= 0
            else:
                assert np.array_equal(ri, zs) and np.array_equal(ti, ds) and len(ri) == len(ti) + dz, (Nd, sh)


def test_no_int32_shift_or_edge_leaves_a_row():
    for Nd, dz, e in ((1, 0, 0), (23, 1, 11), (1000, 0, 31), (1000, 1, 2 ** 31 - 1)):
        for sh in (-2 ** 31, -12, -e, -e + 1, 0, Nd - 2 * e - 1, Nd - 2 * e, 2 ** 31 - 1):
            ri, ti = B.window(Nd + dz, Nd, e, sh)
            assert len(ri) == 0 and len(ti) == 0 or (1 <= ri.min() and ri.max() < Nd + dz and 0 <= ti.min() and ti.max() < Nd and len(ri) == len(ti) + dz)


@pytest.mark.parametrize("name", B.LAUNCHES + ["wide"])
def test_gpu_cases_meet_the_floors_and_the_second_model(name):
    xs, ms = B.build_launch(name)
    if name != "wide":
        assert [x["shift"] for x in xs] == [-10, 0, 10]
    for x, m in zip(xs, ms):
        Nd = x["tx"].shape[-1]
        assert m["kept"] == max(Nd - 2 * x["edge"] - x["shift"], 0) and B.meets_floors(x, m)
        sl = B.slices_of(x)
        if m["kept"] == 0:
            assert sl is None and np.isnan(m["AIR"]) and np.isnan(m["GMI"]) and m["sym_err"] == 0 and m["bit_err"] == 0
            continue
        assert m["margin"] >= 0.05 and m["qgap"] > 0.05 and m["min_post"] >= 1e-30
        counts, winner, dist, _ = R.ser(sl[0], sl[1], x["amp"])                 # the same slices, the other model
        assert sl[0].shape[1] == len(x["z"]) - Nd + m["kept"] and sl[1].shape[1] == m["kept"]
        assert m["hyp"] == winner and m["sym_err"] == counts[winner] and np.array_equal(m["cnt"], counts)
        if m["kept"] >= 11:
            assert m["hyp"] == x["hyp"] and m["sym_err"] == x["n_err"]


def test_launches_cover_what_they_are_meant_to():
    L = B.launches()
    S = [s for v in L.values() for s in v]
    assert len(L) == 144 and {s["Nd"] - 2 * s["e"] for s in S} == {1, 2, 11, 38, 247, 1008} and {s["e"] for s in S} == {11, 31}
    assert {s["dz"] for s in S} == {0, 1} and {s["interleaved"] for s in S} == {False, True} and {s["n"] for s in S} == {2, 4, 8}
    assert {s["hyp"] for s in S} == {0, 1, 2, 3} and {s["nu"] for s in S} == {0.0, B.NU_SHAPED} and {s["var"] for s in S} == {0.004, 0.0063, 0.01}
    assert all(g != 1 for s in S for g in s["gain"]) and {s["n_err"] for s in S} == {0, 1, 2, 3}
    kept = {name: [m["kept"] for m in B.build_launch(name)[1]] for name in ("D1-e11-dz0-il0-n8", "D11-e31-dz1-il1-n4", "D247-e11-dz0-il1-n2")}
    assert kept == {"D1-e11-dz0-il0-n8": [11, 1, 0], "D11-e31-dz1-il1-n4": [21, 11, 1], "D247-e11-dz0-il1-n2": [257, 247, 237]}
    assert [(x["shift"], x["edge"]) for x in B.build_launch("wide")[0]] == [(-12, 31), (11, 31), (-12, 31)]
    hyps = {(m["hyp"], x["n"]) for name in B.LAUNCHES for x, m in zip(*B.build_launch(name)) if m["kept"] >= 11}
    assert hyps == {(h, n) for h in range(4) for n in (2, 4, 8)}                # every hypothesis wins at every constellation size


def test_zero_track_and_the_minus_edge_shift_have_no_measurement():
    x = dict(B.build_launch("D38-e11-dz0-il0-n4")[0][1])
    assert B.model(x)["kept"] == 38
    assert B.model(dict(x, shift=-11))["kept"] == 0 and B.model(dict(x, z=np.zeros_like(x["z"])))["kept"] == 0
    assert np.isnan(B.model(dict(x, z=np.zeros_like(x["z"])))["GMI"])


def test_the_extra_sample_of_the_slice_enters_the_scale():
    """_ref_awgn.longer_slice_frame: one symbol sits 1 % inside a threshold with the one-sample-longer slice in the scale and 3 % outside without."""
    fr = R.longer_slice_frame()
    z, P = fr["track"], np.full(4, 0.25)
    with_extra = B.track_info(z, fr["data"], P, fr["levels"], 0.01, 3, 31)
    without = B.track_info(z[:-1], fr["data"], P, fr["levels"], 0.01, 3, 31)
    assert (with_extra["kept"], with_extra["sym_err"], without["sym_err"]) == (1100 - 62 - 3, 3, 4)


@pytest.mark.parametrize("case", B.DFE_CASES)
def test_nearest_level_of_the_dfe_soft_sequence_is_the_dfe_decision(case):
    n_lev, K2, N, _ = case
    for fr in B.dfe_frames(case):
        dec, margin = R.dfe(fr["ff"], fr["fb"], fr["init"], fr["levels"])
        assert np.array_equal(dec, fr["expected"]) and margin > 0
        z = B.dfe_soft(fr["ff"], fr["fb"], dec, fr["levels"])
        near = R.slice_axis(z.real, fr["levels"])[0] * n_lev + R.slice_axis(z.imag, fr["levels"])[0]
        assert np.array_equal(near[K2:], dec[K2:])
        c = fr["levels"].astype(np.float64)[dec[:K2] // n_lev] + 1j * fr["levels"].astype(np.float64)[dec[:K2] % n_lev]
        assert np.array_equal(z[:K2], c)


def test_float32_cost_is_what_the_gpu_bound_is_built_on():
    """tests/test_awgn_baseline_info_gpu.py holds the kernel to three times Z_DEV: the largest deviation of the kernel's operation order in numpy
    float32 from the float64 model over the planted launches."""
    worst, where = 0.0, None
    for name in B.LAUNCHES:
        for x, m in zip(*B.build_launch(name)):
            d = B.track_float32_deviation(x, m)
            if d is not None and d > worst:
                worst, where = d, (name, x["shift"])
    print(f"track info in float32, largest deviation from the model: {worst:.3e} bit at {where}")
    assert worst <= B.Z_DEV and where[0] == B.Z_DEV_LAUNCH and worst > B.Z_DEV / 2

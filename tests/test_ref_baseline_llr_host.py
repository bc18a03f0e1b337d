"""The float64 LLR models of the baselines (tests/_ref_baseline_llr.py) against the float64 information-rate models they must be consistent with,
on the CPU, over every launch of _ref_cma_info.LAUNCHES (12 launches of 3 runs) and of _ref_awgn_baseline_info.LAUNCHES + ["wide"] (435 runs): the
GMI is an exact function of the LLRs and the transmitted bits, the sign of an LLR is the demapper's bit decision, and the mask is the kept window.
Also what the float32 format costs (the kernels' operation order in numpy float32), which sets the bounds of the GPU tests.
"""
import functools

import numpy as np
import pytest

import _ref_awgn_baseline_info as T
import _ref_awgn_info as A
import _ref_baseline_llr as B
import _ref_cma_info as C
import _ref_info as I
import _ref_llr as L

GMI_TOL = 1e-6          # bit, as tests/test_ref_llr_host.py
TRACK_LAUNCHES = T.LAUNCHES + ["wide"]


@functools.lru_cache(maxsize=None)
def _cma(name):
    """Per run of the launch: (planes[2][2b][N], mask[2][N], bits[2][2b][N], x, info model) under the info model's own hypothesis."""
    xs, ms = C.build_launch(name)
    return [B.cma_llr(x, m["hyp"]) + (L.label_bits(x["tx"], x["n"]), x, m) for x, m in zip(xs, ms)]


@functools.lru_cache(maxsize=None)
def _track(name):
    xs, ms = T.build_launch(name)
    return [B.track_llr(x, m["hyp"]) + (L.label_bits(x["tx"], x["n"]), x, m) for x, m in zip(xs, ms)]


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_cma_gmi_sign_errors_and_mask(name):
    for pl, mask, bits, x, m in _cma(name):
        H = I.entropy(x["P"])
        for p in range(2):
            assert int(mask[p].sum()) == int(m["kept"][p]) and m["kept"][p] > 0
            assert not pl[p][:, ~mask[p]].any()
            assert L.sign_errors(pl[p], bits[p], mask[p]) == int(m["bit_err"][p])
            gmi = L.gmi_from_llr(pl[p], bits[p], mask[p], H)
            assert abs(gmi - m["GMI"][p]) <= GMI_TOL, (name, p, gmi, m["GMI"][p])


@pytest.mark.parametrize("name", TRACK_LAUNCHES)
def test_track_gmi_sign_errors_and_mask(name):
    for pl, mask, bits, x, m in _track(name):
        assert int(mask.sum()) == int(m["kept"])
        assert not pl[:, ~mask].any()
        assert L.sign_errors(pl, bits, mask) == int(m["bit_err"])
        if m["kept"]:
            assert mask[x["edge"]] and not mask[:x["edge"]].any() and mask[x["edge"]:x["edge"] + int(m["kept"])].all()
            gmi = L.gmi_from_llr(pl, bits, mask, A.entropy(x["P"]))
            assert abs(gmi - m["GMI"]) <= GMI_TOL, (name, gmi, m["GMI"])


def test_launch_counts():
    """12 x 3 CMA runs; 435 track runs, of which D = 1 at shift +10 (and D = 2) keep nothing."""
    assert sum(len(_cma(n)) for n in C.LAUNCHES) == 36
    kept = [int(m["kept"]) for n in TRACK_LAUNCHES for *_, m in _track(n)]
    assert len(kept) == 435 and kept.count(0) == 48
    assert sorted({int(m["kept"]) for *_, m in _track("D1-e11-dz0-il0-n2")}) == [0, 1, 11]


@pytest.mark.parametrize("name", ["N43-n8", "N1030-n4"])
def test_cma_hypothesis_is_a_plane_transform(name):
    for x in C.build_launch(name)[0]:
        base = B.cma_llr(x, (0, 0))[0]
        for h in range(1, 8):
            got = B.cma_llr(x, (h, 7 - h))[0]
            assert np.array_equal(got[0], L.retransform(base[0], h, x["n"])) and np.array_equal(got[1], L.retransform(base[1], 7 - h, x["n"]))


def test_cma_without_a_radius_is_all_zeros():
    x = dict(C.build_launch("N43-n2")[0][0])
    x["y"] = np.zeros_like(x["y"])
    for f in (B.cma_llr, B.cma_llr32):
        pl, mask = f(x, (0, 0))
        assert not pl.any() and not mask.any()


def test_float32_deviation_is_the_recorded_one():
    """Y_LLR_DEV_CMA and Y_LLR_DEV_TRACK bound what float32 in the kernels' operation order costs an LLR, relative to max(1, |lam|), over every
    launch; the launch that sets each is the recorded one."""
    worst = {"cma": (0.0, ""), "track": (0.0, "")}
    big = {"cma": 0.0, "track": 0.0}
    for name in C.LAUNCHES:
        for k, (pl, mask, _, x, m) in enumerate(_cma(name)):
            d = L.rel_dev(B.cma_llr32(x, m["hyp"])[0], pl, mask)
            worst["cma"] = max(worst["cma"], (d, f"{name} run {k}"))
            big["cma"] = max(big["cma"], float(np.abs(pl).max()))
    for name in TRACK_LAUNCHES:
        for k, (pl, mask, _, x, m) in enumerate(_track(name)):
            e, mask32 = B.track_llr32(x, m["hyp"])
            assert np.array_equal(mask32, mask)
            d = L.rel_dev(e, pl, mask)
            worst["track"] = max(worst["track"], (d, f"{name} run {k}"))
            big["track"] = max(big["track"], float(np.abs(pl).max()))
    print(f"float32 emulation relative to max(1, |lam|): CMA {worst['cma'][0]:.3e} ({worst['cma'][1]}), track {worst['track'][0]:.3e} "
          f"({worst['track'][1]}); largest |lam| {big['cma']:.1f} / {big['track']:.1f} nats")
    assert worst["cma"][0] <= B.Y_LLR_DEV_CMA and worst["track"][0] <= B.Y_LLR_DEV_TRACK
    assert worst["cma"][0] >= 0.9 * B.Y_LLR_DEV_CMA and worst["track"][0] >= 0.9 * B.Y_LLR_DEV_TRACK   # this measurement rounded up, no looser
    assert worst["cma"][1] == B.Y_LLR_DEV_CMA_LAUNCH and worst["track"][1] == B.Y_LLR_DEV_TRACK_LAUNCH

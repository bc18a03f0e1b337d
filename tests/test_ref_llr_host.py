"""The float64 LLR model tests/_ref_llr.py against the float64 information-rate models it must be consistent with, on the CPU, over every launch
of _ref_info.LAUNCHES (DP) and _ref_awgn_info.LAUNCHES (AWGN): the GMI is an exact function of the LLRs and the transmitted bits, the sign of an
LLR is the demapper's bit decision, a hypothesis only exchanges planes and negates top-bit planes, and the mask is the kept window.  Also what
the float32 format costs y-mode (the kernels' operation order in numpy float32), which sets the bound of the GPU tests.
"""
import functools

import numpy as np
import pytest

import _ref_awgn_info as A
import _ref_info as I
import _ref_llr as L

GMI_TOL = 1e-6          # bit: the info model takes log2 of a set sum of float32 posteriors that add up to 1 within a few 1e-8 (7e-8 measured)


@functools.lru_cache(maxsize=None)
def _dp(name, mode):
    """Per run of the launch: (planes[2][2b][N], mask[2][N], bits[2][2b][N], x, info model) under the info model's own hypothesis."""
    xs, mq, my = I.build_launch(name)
    out = []
    for x, m in zip(xs, mq if mode == "q" else my):
        if mode == "q":
            pl, mask = L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], m["hyp"], x["batch_len"])
        else:
            pl, mask = L.dp_llr_y(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], m["hyp"], x["batch_len"])
        out.append((pl, mask, L.label_bits(x["tx"], x["n"]), x, m))
    return out


@functools.lru_cache(maxsize=None)
def _awgn(name, mode):
    xs, mq, my = A.build_launch(name)
    out = []
    for x, m in zip(xs, mq if mode == "q" else my):
        if mode == "q":
            pl, mask = L.awgn_llr_q(x["q"], x["n"], x["shift"], m["hyp"])
        else:
            pl, mask = L.awgn_llr_y(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], m["hyp"])
        out.append((pl, mask, L.label_bits(x["tx"], x["n"]), x, m))
    return out


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", I.LAUNCHES)
def test_dp_gmi_sign_errors_and_mask(name, mode):
    for pl, mask, bits, x, m in _dp(name, mode):
        H = I.entropy(x["P"])
        for p in range(2):
            assert int(mask[p].sum()) == int(m["kept"][p])
            assert not pl[p][:, ~mask[p]].any()
            assert L.sign_errors(pl[p], bits[p], mask[p]) == int(m["bit_err"][p])
            if m["kept"][p]:
                gmi = L.gmi_from_llr(pl[p], bits[p], mask[p], H)
                assert abs(gmi - m["GMI"][p]) <= GMI_TOL, (name, mode, p, gmi, m["GMI"][p])


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", A.LAUNCHES)
def test_awgn_gmi_sign_errors_and_mask(name, mode):
    for pl, mask, bits, x, m in _awgn(name, mode):
        assert int(mask.sum()) == int(m["kept"])
        assert not pl[:, ~mask].any()
        assert L.sign_errors(pl, bits, mask) == int(m["bit_err"])
        if m["kept"]:
            gmi = L.gmi_from_llr(pl, bits, mask, A.entropy(x["P"]))
            assert abs(gmi - m["GMI"]) <= GMI_TOL, (name, mode, gmi, m["GMI"])


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_dp_hypothesis_is_a_plane_transform(name):
    for x in I.build_launch(name)[0]:
        base = L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], (0, 0), x["batch_len"])[0]
        basey = L.dp_llr_y(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], (0, 0), x["batch_len"])[0]
        for h in range(1, 8):
            got = L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], (h, 7 - h), x["batch_len"])[0]
            assert np.array_equal(got[0], L.retransform(base[0], h, x["n"])) and np.array_equal(got[1], L.retransform(base[1], 7 - h, x["n"]))
            goty = L.dp_llr_y(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], (h, h), x["batch_len"])[0]
            assert np.array_equal(goty, L.retransform(basey, h, x["n"]))


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_awgn_hypothesis_is_a_plane_transform(name):
    for x in A.build_launch(name)[0]:
        base = L.awgn_llr_q(x["q"], x["n"], x["shift"], 0)[0]
        basey = L.awgn_llr_y(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], 0)[0]
        for h in range(1, 4):
            assert np.array_equal(L.awgn_llr_q(x["q"], x["n"], x["shift"], h)[0], L.retransform(base, h, x["n"]))
            assert np.array_equal(L.awgn_llr_y(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], h)[0], L.retransform(basey, h, x["n"]))


def test_y_mode_float32_deviation_is_the_recorded_one():
    """Y_LLR_DEV (DP) and Y_LLR_DEV_AWGN bound what float32 in the kernels' operation order costs an LLR, relative to max(1, |lam|), over every
    launch."""
    dp = aw = 0.0
    big = 0.0
    for name in I.LAUNCHES:
        for pl, mask, _, x, m in _dp(name, "y"):
            e = L.dp_llr_y32(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], m["hyp"], x["batch_len"])[0]
            dp = max(dp, L.rel_dev(e, pl, mask))
            big = max(big, float(np.abs(pl).max()))
    for name in A.LAUNCHES:
        for pl, mask, _, x, m in _awgn(name, "y"):
            e = L.awgn_llr_y32(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], m["hyp"])[0]
            aw = max(aw, L.rel_dev(e, pl, mask))
            big = max(big, float(np.abs(pl).max()))
    print(f"y-mode float32 emulation: DP {dp:.3e}, AWGN {aw:.3e} relative to max(1, |lam|); largest |lam| {big:.1f} nats")
    assert dp <= L.Y_LLR_DEV and aw <= L.Y_LLR_DEV_AWGN
    assert dp >= 0.9 * L.Y_LLR_DEV and aw >= 0.9 * L.Y_LLR_DEV_AWGN            # the recorded figures are this measurement rounded up, no looser

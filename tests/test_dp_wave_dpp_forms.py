"""The two forms of a row- or bank-masked DPP step of the wave sums and prefix scans (vae_equalizer_amd/csrc/vaeq_wave.h), as a numpy model of the 64 lanes:

  zero   t = the DPP source where the masks and the row bounds allow it, else +0;  v = v + t on every lane            (wave_sum_dpp, wave_incl_scan_dpp)
  keep   v = v + source on the lanes the masks enable; every other lane keeps v                                      (wave_sum5_dpp_keep, wave_incl_scan2_dpp_keep)

float32 additions in numpy round as the hardware's do (IEEE, round to nearest even), so the model decides bits:
  * the SUM (lane 63) has the same bits in both forms for every input, -0 included: a row that a masked step switches off is never read again;
  * the SCAN has the same bits in both forms unless a partial sum of a switched-off lane is -0 (-0 + 0 = +0, kept it stays -0) -- shown on an all -0 input --
    and no partial sum is -0 when no input is (only -0 + -0 gives -0): the argument the baked B = 100 DP kernel makes for its variance scan, whose inputs are >= +0.
"""
import numpy as np
import pytest

LANES = np.arange(64)
NEG0 = np.uint32(0x80000000)


def _src(ctrl):
    """(source lane, valid) per lane for a DPP control of the gfx9 encoding"""
    l = LANES
    if ctrl in ("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]"):
        perm = np.array([1, 0, 3, 2] if ctrl.endswith("[1,0,3,2]") else [2, 3, 0, 1])
        return (l & ~3) | perm[l & 3], np.ones(64, bool)
    if ctrl == "row_half_mirror":
        return (l & ~7) | (7 - (l & 7)), np.ones(64, bool)
    if ctrl == "row_mirror":
        return (l & ~15) | (15 - (l & 15)), np.ones(64, bool)
    if ctrl.startswith("row_shr:"):
        n = int(ctrl.split(":")[1])
        return np.maximum(l - n, 0), (l & 15) >= n
    if ctrl == "row_bcast:15":                               # the last lane of a row into the next row
        return np.maximum((l & ~15) - 1, 0), l >= 16
    if ctrl == "row_bcast:31":                               # lane 31 into rows 2 and 3
        return np.full(64, 31), l >= 32
    raise ValueError(ctrl)


def dpp_add(v, ctrl, row_mask=0xF, bank_mask=0xF, keep=False, src=None):
    """One step  v (or src) shifted by ctrl, added to v;  keep: the kept-destination form, else the add of a masked zero (bound_ctrl: 0 outside the row)."""
    s, valid = _src(ctrl)
    on = ((row_mask >> (LANES >> 4)) & 1).astype(bool) & ((bank_mask >> ((LANES & 15) >> 2)) & 1).astype(bool)
    moved = (v if src is None else src)[s]
    if keep:
        t = np.where(valid, moved, np.float32(0))
        return np.where(on, (v + t).astype(np.float32), v)
    return (v + np.where(on & valid, moved, np.float32(0))).astype(np.float32)


def wave_sum(v, keep):
    v = np.asarray(v, np.float32)
    for ctrl in ("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror", "row_mirror"):
        v = dpp_add(v, ctrl)
    v = dpp_add(v, "row_bcast:15", row_mask=0xA, keep=keep)
    v = dpp_add(v, "row_bcast:31", row_mask=0xC, keep=keep)
    return v[63]


def wave_incl_scan(v, keep, half=False):
    v = np.asarray(v, np.float32)
    s = dpp_add(v, "row_shr:1")
    s = dpp_add(s, "row_shr:2", src=v)
    s = dpp_add(s, "row_shr:3", src=v)
    s = dpp_add(s, "row_shr:4", bank_mask=0xE, keep=keep)
    s = dpp_add(s, "row_shr:8", bank_mask=0xC, keep=keep)
    s = dpp_add(s, "row_bcast:15", row_mask=0xA, keep=keep)
    return s if half else dpp_add(s, "row_bcast:31", row_mask=0xC, keep=keep)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def inputs(nonneg):
    """Random lanes, lanes with zeros, exact cancellations, constants, tiny and huge magnitudes; nonneg: no negative value and no -0"""
    rng = np.random.default_rng(14)
    out = [np.zeros(64, np.float32), np.full(64, 0.3, np.float32), np.full(64, 1e-45, np.float32)]
    for i in range(200):
        v = rng.standard_normal(64).astype(np.float32) * np.float32(10.0 ** rng.integers(-20, 20))
        if i % 3 == 0:
            v[rng.random(64) < 0.5] = 0.0
        if i % 5 == 0:
            v[rng.random(64) < 0.8] = 0.0
        if i % 7 == 0:
            v[1::2] = -v[0::2]                               # neighbours cancel: partial sums that are exactly +0
        out.append(np.abs(v) if nonneg else v)
    if not nonneg:
        z = np.zeros(64, np.float32)
        z[rng.random(64) < 0.5] = -0.0
        out += [z, -np.zeros(64, np.float32)]
    return out


def test_model_sums_and_scans_are_sums_and_scans():
    rng = np.random.default_rng(3)
    v = rng.random(64).astype(np.float32)
    for keep in (False, True):
        assert abs(float(wave_sum(v, keep)) - float(np.sum(v, dtype=np.float64))) < 1e-4
        assert np.max(np.abs(wave_incl_scan(v, keep).astype(np.float64) - np.cumsum(v, dtype=np.float64))) < 1e-4
        h = wave_incl_scan(v, keep, half=True).astype(np.float64)
        assert np.max(np.abs(h - np.concatenate([np.cumsum(v[:32], dtype=np.float64), np.cumsum(v[32:], dtype=np.float64)]))) < 1e-4
    # the fixed order of the sum: (r3 + r2) + (r1 + r0) over the row sums of the butterfly
    r = [wave_sum(np.where(LANES >> 4 == k, v, np.float32(0)), False) for k in range(4)]
    assert bits(wave_sum(v, True)) == bits(np.float32(np.float32(r[3] + r[2]) + np.float32(r[1] + r[0])))


def test_sum_has_the_same_bits_in_both_forms_for_every_input():
    for v in inputs(nonneg=False):
        assert bits(wave_sum(v, keep=True)) == bits(wave_sum(v, keep=False))
    assert bits(wave_sum(-np.zeros(64, np.float32), keep=True)) == NEG0      # ... a -0 result included


@pytest.mark.parametrize("half", [False, True])
def test_scan_has_the_same_bits_in_both_forms_without_negative_zero(half):
    for v in inputs(nonneg=True):                            # what the kernel's variance scan sees: values >= +0
        a, b = wave_incl_scan(v, True, half), wave_incl_scan(v, False, half)
        assert np.array_equal(bits(a), bits(b)) and not np.any(bits(a) == NEG0)
    for v in inputs(nonneg=False):                           # any sign: still equal as long as no INPUT is -0 (then no partial sum is)
        if np.any(bits(v) == NEG0):
            continue
        a, b = wave_incl_scan(v, True, half), wave_incl_scan(v, False, half)
        assert np.array_equal(bits(a), bits(b)) and not np.any(bits(a) == NEG0)


def test_scan_forms_differ_exactly_where_a_kept_partial_sum_is_negative_zero():
    v = -np.zeros(64, np.float32)
    a, b = wave_incl_scan(v, keep=True), wave_incl_scan(v, keep=False)
    assert not np.array_equal(bits(a), bits(b))
    # lane 3 of a row has all of row_shr:1..3 in range (-0 four times over) and is switched off by bank_mask 0xe: kept it stays -0, with the zero added it is +0
    assert bits(a)[3] == NEG0 and bits(b)[3] == 0
    assert np.all((bits(a) == bits(b)) | ((bits(a) == NEG0) & (bits(b) == 0)))   # the only difference there is
    assert np.array_equal(a, b)                              # ... and one that a comparison of floats does not see

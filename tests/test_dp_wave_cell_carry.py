"""The carried cells of the DP wave kernel's FIR, dL/dU and D loops (CellCarry, csrc/vaeq_dp_wave_kernel.h) in the LDS bank model: the reads that
remain are a subset of the plain loops' reads, so they may need no more passes per half-wave, in the worst read and in total, and the number of
per-lane reads falls by what the loop bounds predict (tools/lds_bank_model.py dp_fir_carry | dp_du_carry | dp_d3_carry).  No GPU needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# reads removed per wave-step at B = 100, M = 25 (G = 6 stages of four taps and one left-over tap; NB = 6 stages of two a):
#   FIR and dL/dU: per array (p resp. chi) 2 cells in each of the stages 1..5 and 1 cell of the left-over tap = 11, two arrays each: 22
#   D: per nu 2 cells in each of the stages 1..5 = 10, two nu: 20
@pytest.mark.parametrize("entry, removed", [("dp_fir_carry", 22), ("dp_du_carry", 22), ("dp_d3_carry", 20)])
def test_carried_loops_need_no_more_passes_than_the_loops_they_replace(entry, removed):
    r = _model().DP_CARRY[entry](100, 25)
    assert r["carry_worst"] <= r["plain_worst"], r
    assert r["carry_passes"] <= r["plain_passes"], r
    assert r["plain_reads"] - r["carry_reads"] == removed, r

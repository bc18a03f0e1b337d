"""The tap-pair lane map of the DP wave kernel's tap gradients (TapPairMap, csrc/vaeq_dp_wave_kernel.h) in the LDS bank model: no per-lane read of
the new mapping may need more passes per half-wave than the plain mapping's reads do (tools/lds_bank_model.py dp_tappair).  No GPU needed."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tap_pair_reads_are_conflict_free_in_the_bank_model(capsys):
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.dp_tappair_model(100, 25)
    out = capsys.readouterr().out
    assert "pairs dL/dh  [1, 1, 1, 1, 1, 1]" in out and "pairs dL/dw  [1, 1, 1, 1, 1, 1]" in out, out

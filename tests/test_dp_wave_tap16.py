"""The seeds of tests/test_dp_wave_tap16_gpu.py's one-hot h cases, checked on the CPU by the oracle alone: at each of them the fp32 C oracle's loss,
var_est, dL/dh and dL/dw are within half that file's tolerances of its own float64 evaluation, for every (chi, nu, j) and all three runs, and its
largest |dL/dw| is not degenerate (onehot_h_seed_ok there)."""
import pytest

from test_dp_wave_tap16_gpu import SEED_H, onehot_h_seed_ok


@pytest.mark.parametrize("n", sorted(SEED_H))
def test_the_one_hot_h_seeds_are_well_conditioned_by_the_oracle_alone(n):
    assert onehot_h_seed_ok(n, SEED_H[n])

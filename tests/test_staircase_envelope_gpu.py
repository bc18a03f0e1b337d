"""vaeq_staircase_decode over the parts of include/vaeq.h's envelope that tests/test_staircase_gpu.py leaves out, through engine.staircase_decode
against the integer model (tests/_ref_staircase.py) with no tolerance: np.array_equal on out, hard, pos_err and pos_iters.  The cases live in
tests/_staircase_envelope_cases.py (its docstring lists them); tests/test_ref_fec_envelope_host.py asserts on the CPU that the model reaches in
them what this file relies on.  Every test prints its figures before it asserts.

  long chains (the ring of slots reused up to nine times), the widest window (W = 32, also longer than the chain), the iteration cap of 100,
  the smallest block (s = 3), the table builder on 64 and 256 threads over GF(2^10), GF(2^9) and GF(2^4), planted components of exactly
  5 .. t + 1 errors at t = 8 and t = 7 (the packed root list and its second word), w in {1, 5, 13, 64} and a frame that fits exactly, and the
  grid: 300 chains in one run, 40 runs of one chain."""
import numpy as np
import pytest
import torch

import _ref_staircase as S
import _staircase_envelope_cases as E

pytestmark = pytest.mark.gpu

FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max", "nflip", "bad_flips")


def _decode(c):
    from vae_equalizer_amd.engine import BchCode, StaircaseCode, staircase_decode
    code = StaircaseCode(BchCode(c["m"], c["t"], n=2 * c["s"]), c["L"])
    return staircase_decode(torch.from_numpy(c["llr"].copy()).cuda(), torch.from_numpy(c["bits"].copy()).cuda(), code, c["W"], t0=c["t0"],
                            chains=c["C"], iters=c["iters"], want_hard=True, want_profile=True)


def _same(got, c):
    out = np.stack([got[k].cpu().numpy() for k in FIGS], -1)
    diff = {k: int((a != b).sum()) for k, a, b in (("out", out, c["out"]), ("hard", got["hard"].cpu().numpy(), c["hard"]),
                                                   ("pos_err", got["pos_err"].cpu().numpy(), c["pos_err"]),
                                                   ("pos_iters", got["pos_iters"].cpu().numpy(), c["pos_iters"]))}
    want = c["out"]
    short = (lambda v: v.ravel().tolist()) if want.shape[0] * want.shape[1] <= 12 else (lambda v: f"sum {int(v.sum())}")
    print(f"{c['name']}: pre_err {short(want[..., 3])} post_err {short(want[..., 2])} iters {short(want[..., 0])} iters_max {short(want[..., 5])} "
          f"nflip {short(want[..., 6])} bad_flips {short(want[..., 7])}; the kernel differs in {diff}")
    assert out.shape == want.shape and got["hard"].dtype == torch.int8 and tuple(got["hard"].shape) == c["hard"].shape
    assert not any(diff.values()), (c["name"], diff)
    assert got["positions"] == S.n_positions(c["L"], c["W"]) == c["pos_iters"].shape[-1]


def _state_fits(c):
    from vae_equalizer_amd import _native as nat
    lds = nat.lib().vaeq_staircase_lds_bytes(c.m, c.s, c.W)
    assert 0 < lds <= 64 * 1024, (c.name, lds)
    return lds


@pytest.mark.parametrize("c", [c for g in ("long", "window", "cap", "smallest", "widths", "grid") for c in E.GROUPS[g]], ids=lambda c: c.name)
def test_kernel_equals_model(c):
    _same(_decode(E.case(c)), E.case(c))


@pytest.mark.parametrize("c", E.GROUPS["tables"], ids=lambda c: c.name)
def test_table_builder_against_thread_count(c):
    """The launch has ceil(s / 64) waves: 64 threads build the 1023 entries of GF(2^10) sixteen each, 256 threads the 511 of GF(2^9) two each."""
    lds = _state_fits(c)
    print(f"{c.name}: {(c.s + 63) // 64 * 64} threads, q = {(1 << c.m) - 1}, {lds} bytes of state")
    _same(_decode(E.case(c)), E.case(c))


@pytest.mark.parametrize("mixed", (0, 1), ids=("row", "mixed"))
@pytest.mark.parametrize("m,t,s", [p[:3] for p in E.PLANTED], ids=str)
def test_planted_root_counts(m, t, s, mixed):
    c, info, _ = E.planted(m, t, s, mixed)
    _state_fits(E.Case(*(c[k] for k in E.Case._fields)))
    print(f"{c['name']}: planted components (k, j, positions) {info}")
    _same(_decode(c), c)

"""The three epilogue entry points (vaeq_dp_epilogue, vaeq_dp_epilogue_compact, vaeq_cma_epilogue) over their envelope against the float64
model of tests/_ref_epilogue.py -- EXACTLY: shifts and swap flags equal, SER == float32(count) / float32(kept) bit for bit, NaN exactly
where the model keeps nothing.  No tolerance anywhere: every case is built with margins (correlation peaks, decision thresholds, q gaps)
that test_ref_epilogue_host.py asserts on the CPU, so a float32 kernel that decides differently is wrong, not unlucky.

The cases (launches() in _ref_epilogue.py, one launch of R <= 8 runs each, 37 for the batching case): every shift[0] in -10 .. 10 with both
swap flags and all 8 rotation / IQ-flip hypotheses at n_lev 2, 4, 8; frame lengths at the entry points' minimum with every N % 4 residue, at
the edges of the 704-symbol correlation tile, and on both sides of the compact kernel's LDS-residency switch; minibatch lengths 20 .. 1000
incl. odd ones, > 256, == N; empty kept windows (NaN); batch_len < 20 (negative slice end); per-run parameters in one launch."""
import numpy as np
import pytest
import torch

import _ref_epilogue as M

pytestmark = pytest.mark.gpu

KEYS = ("shift_q", "r_q", "shift_c", "r_c", "SER")


def _dev(xs, k, dtype=None):
    a = torch.from_numpy(np.ascontiguousarray(np.stack([x[k] for x in xs]))).cuda()
    return a if dtype is None else a.to(dtype)


def _host(res):
    return {k: res[k].cpu().numpy() for k in KEYS}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype for k in KEYS)


def _assert_model(res, ms, what):
    for i, m in enumerate(ms):
        got = {k: res[k][i] for k in KEYS}
        print(what, i, "kept", (m["kept_c"], m["kept_q"]), "SER", got["SER"], "model", m["SER"], "shifts", got["shift_c"], got["shift_q"], flush=True)
        assert np.array_equal(got["shift_q"], m["shift_q"]) and int(got["r_q"]) == m["r_q"], (what, i, got, m["shift_q"], m["r_q"])
        assert np.array_equal(got["shift_c"], m["shift_c"]) and int(got["r_c"]) == m["r_c"], (what, i, got, m["shift_c"], m["r_c"])
        assert got["SER"].dtype == np.float32 and np.array_equal(np.isnan(got["SER"]), np.isnan(m["SER"])), (what, i, got["SER"], m["SER"])
        ok = ~np.isnan(m["SER"])
        assert got["SER"][ok].tobytes() == m["SER"][ok].tobytes(), (what, i, got["SER"], m["SER"], m["cnt_c"].min(0), m["cnt_q"].min(0))


def _compact_inputs(xs):
    """eq / dec as the training kernel would hand them over, derived from q in float64."""
    eqs, decs = zip(*[M.q_to_compact(x["q"], x["amp"]) for x in xs])
    return (torch.from_numpy(np.stack(eqs).astype(np.float32)).cuda(), torch.from_numpy(np.stack(decs).astype(np.int8)).cuda())


def _run_all_forms(xs, monkeypatch):
    """-> dict form -> host results: the full-q entry point and the compact one in its three forms."""
    from vae_equalizer_amd.engine import dp_epilogue, dp_epilogue_compact
    bl = xs[0]["batch_len"]
    q, y, tx, amp, nu, var = _dev(xs, "q"), _dev(xs, "y"), _dev(xs, "tx"), xs[0]["amp"], _dev(xs, "nu_sc"), _dev(xs, "var")
    eq, dec = _compact_inputs(xs)
    out = {"full": _host(dp_epilogue(q, y, tx, amp, nu, var, bl)), "compact": _host(dp_epilogue_compact(eq, dec, y, tx, amp, nu, var, bl))}
    monkeypatch.setenv("VAEQ_EPI_NOTXC", "1")
    out["compact-notxc"] = _host(dp_epilogue_compact(eq, dec, y, tx, amp, nu, var, bl))
    monkeypatch.delenv("VAEQ_EPI_NOTXC")
    monkeypatch.setenv("VAEQ_EPI_REREAD", "1")
    out["compact-reread"] = _host(dp_epilogue_compact(eq, dec, y, tx, amp, nu, var, bl))
    monkeypatch.delenv("VAEQ_EPI_REREAD")
    return out


@pytest.mark.parametrize("name", [k for k in M.DP_LAUNCHES if k != "per-run-R37"])
def test_dp_entry_points_equal_the_model(name, monkeypatch):
    xs, ms = M.build_launch(name)
    out = _run_all_forms(xs, monkeypatch)
    for form, res in out.items():
        _assert_model(res, ms, f"{name}/{form}")
    for form in ("compact-notxc", "compact-reread"):
        assert _same(out["compact"], out[form]), (name, form, out["compact"], out[form])


def test_per_run_parameters_in_one_launch(monkeypatch):
    """37 runs with their own shift, swap, rotation, gain, nu_sc, var and pmf: one launch == the same runs launched one by one == the model."""
    from vae_equalizer_amd.engine import dp_epilogue, dp_epilogue_compact
    xs, ms = M.build_launch("per-run-R37")
    assert len(xs) == 37
    out = _run_all_forms(xs, monkeypatch)
    for form, res in out.items():
        _assert_model(res, ms, f"per-run-R37/{form}")
    for i, x in enumerate(xs):
        one = [x]
        q, y, tx, nu, var = _dev(one, "q"), _dev(one, "y"), _dev(one, "tx"), _dev(one, "nu_sc"), _dev(one, "var")
        eq, dec = _compact_inputs(one)
        for form, res in (("full", dp_epilogue(q, y, tx, x["amp"], nu, var, x["batch_len"])),
                          ("compact", dp_epilogue_compact(eq, dec, y, tx, x["amp"], nu, var, x["batch_len"]))):
            res = _host(res)
            for k in KEYS:
                assert np.array_equal(res[k][0], out[form][k][i], equal_nan=True), (form, i, k, res[k][0], out[form][k][i])


@pytest.mark.parametrize("name", M.CMA_LAUNCHES)
def test_cma_entry_point_equals_the_model(name):
    from vae_equalizer_amd.engine import cma_epilogue
    xs, ms = M.build_launch(name)
    y, tx, nu, var = _dev(xs, "y"), _dev(xs, "tx"), _dev(xs, "nu_sc"), _dev(xs, "var")
    res = _host(cma_epilogue(y, tx, xs[0]["amp"], nu, var))
    _assert_model(res, ms, name)
    assert _same(res, _host(cma_epilogue(y, tx, xs[0]["amp"], nu, var)))          # a repeat call is bitwise equal


@pytest.mark.parametrize("name", ["shift-n8", "B257-N771", "empty-N400-B20", "N705"])
def test_repeat_call_is_bitwise_equal(name):
    from vae_equalizer_amd.engine import dp_epilogue, dp_epilogue_compact
    xs, _ = M.build_launch(name)
    bl = xs[0]["batch_len"]
    q, y, tx, amp, nu, var = _dev(xs, "q"), _dev(xs, "y"), _dev(xs, "tx"), xs[0]["amp"], _dev(xs, "nu_sc"), _dev(xs, "var")
    eq, dec = _compact_inputs(xs)
    assert _same(_host(dp_epilogue(q, y, tx, amp, nu, var, bl)), _host(dp_epilogue(q, y, tx, amp, nu, var, bl)))
    assert _same(_host(dp_epilogue_compact(eq, dec, y, tx, amp, nu, var, bl)), _host(dp_epilogue_compact(eq, dec, y, tx, amp, nu, var, bl)))

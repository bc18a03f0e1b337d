"""vaeq_dp_epilogue_info (GMI, achievable rate, pre-FEC BER of a DP frame) against the float64 model tests/_ref_info.py.

Launches of R = 3 runs: N in {43, 47, 400, 1030} (the compact epilogue's tile edges and one tile boundary), batch_len in {0, 20, 100}, n_lev in
{2, 4, 8}, shifts -10 / 0 / +10 unequal between the polarisations, both r, uniform and heavily shaped (nu = 0.1222578) pmf, var per run and
polarisation, every hypothesis.  tests/test_ref_info_host.py asserts the preconditions: posteriors at the transmitted level >= 1e-30 and a
top-two posterior gap above 0.05 in every compared case.

Bounds.  q-mode: the model's terms come from the same float32 q; a float32 log2 of magnitude <= 100 is good to a few 1e-5 at worst and a
fixed-order mean over <= 1030 terms adds less: 1e-4 bit.  y-mode: against the model evaluated in float64 from y; three times the largest
deviation measured on these cases (DESIGN.md section 5 records both maxima).  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_epilogue as E
import _ref_info as I

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4            # bit, set by the issue from the precision of a float32 log2
Y_TOL = 3 * I.Y_DEV     # bit: three times the largest y-mode deviation recorded for the cases below
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")


def _dev(xs, key, dtype=None):
    a = np.stack([np.asarray(x[key]) for x in xs])
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _call(xs, mode, **over):
    from vae_equalizer_amd.engine import dp_epilogue_info
    kw = dict(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), r=_dev(xs, "r"), batch_len=xs[0]["batch_len"])
    if mode == "q":
        kw["q"] = _dev(xs, "q")
    else:
        kw.update(y=_dev(xs, "y"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"))
    kw.update(over)
    return dp_epilogue_info(**kw)


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    """One kernel launch per (launch, mode), shared by the tests; -> dict of numpy arrays [R,2]."""
    xs = I.build_launch(name)[0]
    return {k: v.cpu().numpy() for k, v in _call(xs, mode).items()}


def _dev_max(got, models, keys):
    """Largest |kernel - model| over the runs that keep something, per figure."""
    out = {}
    for k in keys:
        d = [np.abs(got[k][i].astype(np.float64) - m[k]).max() for i, m in enumerate(models) if m["kept"][0] > 0]
        out[k] = max(d) if d else 0.0
    return out


def _check_counts_and_nan(got, models):
    for i, m in enumerate(models):
        for k in CNT:
            assert np.array_equal(got[k][i], m[k]), (i, k, got[k][i], m[k])
        if m["kept"][0] == 0:
            for k in FIG:
                assert np.isnan(got[k][i]).all(), (i, k)


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_q_mode_counts_equal_the_model(name):
    _check_counts_and_nan(_run(name, "q"), I.build_launch(name)[1])


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_q_mode_figures(name):
    got, models = _run(name, "q"), I.build_launch(name)[1]
    dev = _dev_max(got, models, FIG)
    print(f"q-mode {name}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["AIR"] <= Q_TOL and dev["GMI"] <= Q_TOL
    assert dev["NGMI"] <= Q_TOL and dev["BER"] <= 1e-7                          # NGMI = GMI rescaled by 1 / (2 b) <= 1 / 2; BER one float32 division


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_q_mode_symbol_errors_are_the_epilogue_ser(name):
    """On the alignment dp_epilogue itself finds on the same inputs, sym_err / kept is its soft-demapper SER, exactly."""
    from vae_equalizer_amd.engine import dp_epilogue
    xs = I.build_launch(name)[0]
    ep = dp_epilogue(_dev(xs, "q"), _dev(xs, "y"), _dev(xs, "tx"), xs[0]["amp"], _dev(xs, "nu_sc"), _dev(xs, "var"), batch_len=xs[0]["batch_len"])
    got = _call(xs, "q", shift=ep["shift_q"], r=ep["r_q"])
    ser = got["sym_err"].float() / got["kept"].float()                         # 0 / 0 = NaN, the epilogue's empty window
    print(f"{name}: SER_q {ep['SER'][:, 2:4].cpu().numpy().tolist()} sym_err / kept {ser.cpu().numpy().tolist()}")
    assert torch.equal(torch.nan_to_num(ser, nan=-1.0), torch.nan_to_num(ep["SER"][:, 2:4], nan=-1.0))
    assert torch.equal(torch.isnan(ser), got["kept"] == 0)


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_y_mode_counts_equal_the_model(name):
    _check_counts_and_nan(_run(name, "y"), I.build_launch(name)[2])


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_y_mode_figures(name):
    got, models = _run(name, "y"), I.build_launch(name)[2]
    dev = _dev_max(got, models, FIG)
    print(f"y-mode {name}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["AIR"] <= Y_TOL and dev["GMI"] <= Y_TOL
    assert dev["NGMI"] <= Y_TOL and dev["BER"] <= 1e-7


def _underflow_case():
    x = dict(I.make_run(seed=7, N=300, n=8, shift=(0, 0), r=0, hyp=0, batch_len=None, nu=0.0, var=(0.004, 0.004), n_err=(0, 0)))
    t = int(E.tx_levels(x["tx"], 8)[0, 0, 100])
    q = x["q"].copy()
    q[0, t, 100] = 0.0
    x["q0"], x["q"] = x["q"], q
    return x


def test_underflow_costs_126_bit_in_q_mode_and_nothing_in_y_mode():
    x = _underflow_case()
    base = _call([dict(x, q=x["q0"])], "q")
    got, goty = _call([x], "q"), _call([x], "y")
    K = int(got["kept"][0, 0])
    m = I.info_q(x["q"], x["tx"], x["P"], x["shift"], 0)
    step = (got["AIR"][0, 0].double() - base["AIR"][0, 0].double()).item() * K
    want = -126.0 - np.log2(float(x["q0"][0, int(E.tx_levels(x["tx"], 8)[0, 0, 100]), 100]))
    print(f"underflow: AIR {got['AIR'][0].tolist()} model {m['AIR'].tolist()}; the symbol's term moved by {step:.4f} bit, expected {want:.4f}")
    assert m["min_post"] == 0.0 and torch.isfinite(got["AIR"]).all() and torch.isfinite(got["GMI"]).all()
    assert abs(step - want) <= 2 * Q_TOL * K                                  # two AIR values, each within Q_TOL of its model
    assert np.abs(got["AIR"][0].cpu().numpy() - m["AIR"]).max() <= Q_TOL and np.abs(got["GMI"][0].cpu().numpy() - m["GMI"]).max() <= Q_TOL
    my = I.info_y(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], 0)
    assert torch.isfinite(goty["AIR"]).all() and np.abs(goty["AIR"][0].cpu().numpy() - my["AIR"]).max() <= Y_TOL


def test_empty_window_gives_nan_figures_and_zero_counts():
    x = I.make_run(seed=11, N=60, n=8, shift=(10, 10), r=0, hyp=0, batch_len=20, nu=0.0, var=(0.004, 0.004), n_err=(0, 0))
    for mode in ("q", "y"):
        got = _call([x], mode)
        for k in FIG:
            assert torch.isnan(got[k]).all(), (mode, k)
        for k in CNT:
            assert not got[k].any(), (mode, k)


@pytest.mark.parametrize("name", ["N1030-B0-n8", "N400-B100-n4"])
def test_two_calls_give_identical_bits(name):
    xs = I.build_launch(name)[0]
    for mode in ("q", "y"):
        a, b = _call(xs, mode), _call(xs, mode)
        for k in FIG + CNT:
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), (mode, k)


def test_both_or_neither_source_is_refused():
    from vae_equalizer_amd.engine import dp_epilogue_info
    xs = I.build_launch("N43-B0-n2")[0]
    with pytest.raises(ValueError):
        _call(xs, "q", y=_dev(xs, "y"))
    with pytest.raises(ValueError):
        dp_epilogue_info(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), r=_dev(xs, "r"))


def test_run_dp_batch_reports_the_figures_of_its_frames():
    """want_info=True: the last frame's figures (q-mode there: keep_last materialises its q) are dp_epilogue_info's on that frame's outputs, the
    y-mode figures of the same frame agree with them to the demapper's float32 rounding, and nothing else changes."""
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    from vae_equalizer_amd.engine import dp_epilogue_info
    nus = [0.0, 0.0270955, 0.1222578]
    runs = [DPRun(22 + i, nus[i], 0.01, 0.3, 2.5e-3, 90e9, seed=300 + i) for i in range(3)]
    kw = dict(mod="64-QAM", sps=2, M_est=25, batch_len=100, N_frame_max=1000, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24,
              tau_pmd=0.1e-12 * np.sqrt(1000), phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, keep_last=True)
    a = run_dp_batch(runs, want_info=True, **kw)
    b = run_dp_batch(runs, want_info=False, **kw)
    assert "info" not in b and set(a) - set(b) == {"info"}
    for k in ("SER", "Var_est", "var"):
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), k
    for k in ("q", "y", "data", "shift_q", "r_q"):
        assert torch.equal(a["last"][k], b["last"][k]), k
    assert torch.equal(a["engine"].W, b["engine"].W)
    last = a["last"]
    tabs = [sfun.qam_tables("64-QAM", nu) for nu in nus]
    P = np.stack([t["P"] for t in tabs])
    common = dict(data=last["data"], amp_levels=tabs[0]["amps"], P=P, shift=last["shift_q"], r=last["r_q"], batch_len=100)
    fq = dp_epilogue_info(q=last["q"], **common)
    fy = dp_epilogue_info(y=last["y"], nu_sc=np.array([t["nu_sc"] for t in tabs]), var=a["var"], **common)
    info = a["info"]
    print("run_dp_batch last frame: GMI", info["GMI"][:, :, -1].tolist(), "NGMI", info["NGMI"][:, :, -1].tolist(), "BER", info["BER"][:, :, -1].tolist())
    for k in FIG + CNT:
        assert info[k].shape == (3, 2, 2)
        assert torch.equal(info[k][:, :, -1], fq[k].cpu()), k
    assert (info["kept"] > 800).all() and torch.isfinite(info["GMI"]).all()
    ser_q = a["SER"][:, 2:4, :]
    assert torch.equal(info["sym_err"].float() / info["kept"].float(), ser_q)  # every frame, y-mode and q-mode alike
    for k in CNT:                                                              # the demapper's decisions do not depend on the form it is evaluated in
        assert torch.equal(fy[k], fq[k]), k
    assert torch.isfinite(fy["GMI"]).all() and torch.isfinite(fy["AIR"]).all()

"""vaeq_awgn_info (GMI, achievable rate, pre-FEC BER of an AWGN validation frame) against the float64 model tests/_ref_awgn_info.py, and its way up
through engine.awgn_info, AWGNEngine.info / NNEngine.info, run_awgn_batch / run_vaenn_batch(want_info=True) and the two sweep scripts.

Launches of R = 3 runs with shifts -10 / 0 / +10: N in {23, 24, 33, 60, 257, 1030, 2100} (11 / 1 / 0 and 21 / 11 / 1 kept symbols, one symbol in the
second round of the 256-thread workgroup, both sides of the 1000-symbol shift-search length), n_lev in {2, 4, 8}, every hypothesis, uniform and
heavily shaped (nu = 0.1222578) pmf, var in {0.004, 0.0063, 0.01}.  tests/test_ref_awgn_info_host.py asserts the preconditions of every case.

Bounds.  q-mode: the model's terms come from the same float32 q; a float32 log2 of magnitude <= 126 is good to a few 1e-5 at worst and a
fixed-order mean over <= 2100 terms adds less: 1e-4 bit (the project's Q_TOL, tests/test_epilogue_info_gpu.py).  y-mode: three times
_ref_awgn_info.Y_DEV, the largest deviation of the kernel's operation order in numpy float32 from the model over these cases, computed on the
CPU; the factor allows for the device's exp2 / log2 and another order of the sums behind m_c.  Every test prints its figures before it asserts.
"""
import functools
import math

import numpy as np
import pytest
import scipy.io as io
import torch

import _ref_awgn_info as A

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4            # bit, set by the issue from the precision of a float32 log2
Y_TOL = 3 * A.Y_DEV     # bit
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")


def _dev(xs, key, dtype=None):
    a = np.stack([np.asarray(x[key]) for x in xs])
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _call(xs, mode, **over):
    from vae_equalizer_amd.engine import awgn_info
    kw = dict(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"))
    if mode == "q":
        kw["q"] = _dev(xs, "q")
    else:
        kw.update(y=_dev(xs, "y"), amp_mean=_dev(xs, "amp_mean"), var=_dev(xs, "var"))
    kw.update(over)
    return awgn_info(**kw)


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    """One kernel launch per (launch, mode), shared by the tests; -> dict of numpy arrays [R]."""
    return {k: v.cpu().numpy() for k, v in _call(A.build_launch(name)[0], mode).items()}


def _dev_max(got, models, keys):
    """Largest |kernel - model| over the runs that keep something, per figure."""
    out = {}
    for k in keys:
        d = [abs(float(got[k][i]) - m[k]) for i, m in enumerate(models) if m["kept"] > 0]
        out[k] = max(d) if d else 0.0
    return out


def _check_counts_and_nan(got, models):
    for i, m in enumerate(models):
        for k in CNT:
            assert int(got[k][i]) == m[k], (i, k, got[k][i], m[k])
        if m["kept"] == 0:
            for k in FIG:
                assert np.isnan(got[k][i]), (i, k)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", A.LAUNCHES)
def test_counts_equal_the_model(name, mode):
    got, models = _run(name, mode), A.build_launch(name)[1 if mode == "q" else 2]
    print(f"{mode}-mode {name}: " + ", ".join(f"{k} {got[k].tolist()}" for k in CNT) + f"; model {[[m[k] for m in models] for k in CNT]}")
    _check_counts_and_nan(got, models)


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_q_mode_figures(name):
    got, models = _run(name, "q"), A.build_launch(name)[1]
    dev = _dev_max(got, models, FIG)
    print(f"q-mode {name}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["AIR"] <= Q_TOL and dev["GMI"] <= Q_TOL
    assert dev["NGMI"] <= Q_TOL and dev["BER"] <= 1e-7


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_y_mode_figures(name):
    got, models = _run(name, "y"), A.build_launch(name)[2]
    dev = _dev_max(got, models, FIG)
    print(f"y-mode {name}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()) + f" (bound {Y_TOL:.2e})")
    assert dev["AIR"] <= Y_TOL and dev["GMI"] <= Y_TOL
    assert dev["NGMI"] <= Y_TOL and dev["BER"] <= 1e-7


def test_empty_windows_give_nan_figures_and_zero_counts():
    """shift = -11 (data[:, 11:0] is empty), a y whose Q component is zero throughout (no normalisation: y-mode only), and a run that keeps its
    symbols between them, in one launch."""
    xs = [dict(x) for x in A.build_launch("N60-n8")[0]]
    xs[0]["shift"] = -11
    y = xs[2]["y"].copy()
    y[1] = 0
    xs[2]["y"] = y
    for mode in ("q", "y"):
        got = {k: v.cpu().numpy() for k, v in _call(xs, mode).items()}
        models = [A.models(x)[0 if mode == "q" else 1] for x in xs]
        print(f"{mode}-mode: " + ", ".join(f"{k} {got[k].tolist()}" for k in FIG + CNT))
        assert [m["kept"] for m in models] == ([0, 38, 28] if mode == "q" else [0, 38, 0])
        _check_counts_and_nan(got, models)
        for i, m in enumerate(models):
            if m["kept"]:
                assert abs(got["GMI"][i] - m["GMI"]) <= (Q_TOL if mode == "q" else Y_TOL)


def test_underflow_costs_126_bit_in_q_mode_and_everything_stays_finite():
    x = dict(A.make_run(seed=7, N=300, n=8, shift=0, hyp=0, nu=0.0, var=0.004, n_err=0))
    t = int(A.tx_levels(x["tx"], 8)[0, 100])
    q = x["q"].copy()
    was = float(q[t, 100])
    q[t, 100] = 0.0
    base, got = _call([x], "q"), _call([dict(x, q=q)], "q")
    m = A.info_q(q, x["tx"], x["P"], 0)
    K = int(got["kept"][0])
    step = (got["AIR"][0].double() - base["AIR"][0].double()).item() * K
    want = -126.0 - math.log2(was)
    print(f"underflow: AIR {got['AIR'].tolist()} GMI {got['GMI'].tolist()} model {m['AIR']:.6f} {m['GMI']:.6f}; the symbol's term moved by {step:.4f} bit, "
          f"expected {want:.4f}")
    assert m["min_post"] == 0.0 and K == 278 and torch.isfinite(got["AIR"]).all() and torch.isfinite(got["GMI"]).all()
    assert abs(step - want) <= 2 * Q_TOL * K                                  # two AIR values, each within Q_TOL of its model
    assert abs(got["AIR"][0].item() - m["AIR"]) <= Q_TOL and abs(got["GMI"][0].item() - m["GMI"]) <= Q_TOL
    assert int(got["sym_err"][0]) == m["sym_err"] == 1


@functools.lru_cache(maxsize=None)
def _eq_runs(N, n):
    """The launch N-n of the model; N = 64, which is none of its sizes, is built the same way (three conditioned runs, shifts -10 / 0 / +10)."""
    if f"N{N}-n{n}" in A.launches():
        return A.build_launch(f"N{N}-n{n}")[0]
    return [A.conditioned_run(dict(seed=31000 + 300 * n + 100 * k, N=N, n=n, shift=sh, hyp=(n + k) % 4, nu=(0.0, A.NU_SHAPED)[k % 2], var=A.VARS[k],
                                   n_err=1 + k))[0] for k, sh in enumerate(A.SHIFTS)]


@functools.lru_cache(maxsize=None)
def _validated(N, n):
    """The launch's planted y as conditioned frames x[R,2,2N] (x[:, :, ::2] = y, zeros between) through a fresh AWGNEngine with M_est = 25: the
    Dirac taps make the validation kernel's output the planted y exactly.  -> (xs, engine, x, data, (ser, shift, y))."""
    from vae_equalizer_amd.engine import AWGNEngine
    xs = _eq_runs(N, n)
    yp = _dev(xs, "y")
    R, _, N = yp.shape
    x = torch.zeros(R, 2, 2 * N, device="cuda")
    x[:, :, ::2] = yp
    eng = AWGNEngine(R, 25, xs[0]["amp"], np.stack([v["P"] for v in xs]), [float(v["amp_mean"]) for v in xs], [float(v["var"]) for v in xs], "cuda:0", 2)
    data = _dev(xs, "tx")
    return xs, eng, x, data, eng.validate(x, data, 21)


# N = 60 goes through vaeq_awgn_validate_short (AWGNEngine.validate picks it for rows under the 64 symbols vaeq_awgn_validate asks for: the same
# kernel); N = 64, the shortest row of vaeq_awgn_validate itself, stands beside it.
EQ_SIZES = (60, 64, 1030, 2100)


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("N", EQ_SIZES)
def test_y_mode_symbol_errors_are_the_validation_ser(N, n):
    """At whatever shift the validation finds (its 0.02 N threshold misfires on short rows by design of the reference), sym_err / kept of y-mode on
    the y it returns is its SER bit for bit: the margin floor of the whole row keeps every symbol off the rounding of a threshold."""
    name = f"N{N}-n{n}"
    xs, eng, x, data, (ser, shift, y) = _validated(N, n)
    got = eng.info(y, data, shift)
    mine = got["sym_err"].float() / got["kept"].float()                       # 0 / 0 = NaN, the validation's empty window
    print(f"{name}: shift {shift.tolist()} (planted {[v['shift'] for v in xs]}) SER {ser.tolist()} sym_err / kept {mine.tolist()} kept {got['kept'].tolist()}")
    assert torch.equal(y, _dev(xs, "y"))                                      # the conditioning: the kernel's output is the planted y
    assert torch.equal(torch.nan_to_num(mine, nan=-1.0), torch.nan_to_num(ser, nan=-1.0))
    assert torch.equal(torch.isnan(ser), got["kept"] == 0)


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("N", EQ_SIZES)
def test_q_mode_on_the_forward_q_counts_as_y_mode(N, n):
    """q-mode on AWGNEngine.forward's q of the same frame, at the validation's shift, counts what y-mode counts."""
    from vae_equalizer_amd.engine import awgn_info
    name = f"N{N}-n{n}"
    xs, eng, x, data, (ser, shift, y) = _validated(N, n)
    q, yf = eng.forward(x)
    gq = awgn_info(q=q, data=data, amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=shift)
    gy = eng.info(y, data, shift)
    print(f"{name}: q-mode {[gq[k].tolist() for k in CNT]} y-mode {[gy[k].tolist() for k in CNT]} GMI {gq['GMI'].tolist()} {gy['GMI'].tolist()}")
    for k in CNT:
        assert torch.equal(gq[k], gy[k]), k


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("N", [33, 60, 63])
def test_short_row_validation_equals_the_reference_steps(N, n):
    """AWGNEngine.validate on rows under 64 symbols (vaeq_awgn_validate_short) against the torch restatement of the reference's own steps on
    vaeq_awgn_forward's q of the same frame: the same shift, the same SER (one symbol of slack for the packed and the scalar FIR, as
    tests/test_awgn_kernel_gpu.py allows the long rows), the same y.  Noisy frames through non-Dirac taps, so that the FIR has work to do."""
    from vae_equalizer_amd.engine import AWGNEngine
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import SER_q, find_shift
    xs = [A.make_run(seed=41000 + 10 * N + k, N=N, n=n, shift=sh, hyp=k, nu=0.0, var=0.01, n_err=2, gain=(1.0, 1.0)) for k, sh in enumerate((-3, 0, 5))]
    g = torch.Generator().manual_seed(N + n)
    yp = _dev(xs, "y")
    x = torch.zeros(3, 2, 2 * N, device="cuda")
    x[:, :, ::2] = yp
    x += 0.02 * torch.randn(3, 2, 2 * N, generator=g).cuda()
    eng = AWGNEngine(3, 25, xs[0]["amp"], np.stack([v["P"] for v in xs]), [float(v["amp_mean"]) for v in xs], 0.01, "cuda:0", 2)
    eng.W[:, :, 11] = 0.05
    eng.W[:, 0, 13] = -0.04
    data = _dev(xs, "tx")
    ser, sh, y = eng.validate(x, data, 21)
    q, y2 = eng.forward(x)
    amp = torch.tensor(xs[0]["amp"], device="cuda")
    print(f"N{N}-n{n}: shift {sh.tolist()} SER {ser.tolist()} max |y - y_forward| {(y - y2).abs().max().item():.2e}")
    assert (y - y2).abs().max().item() <= 1e-6 * y2.abs().max().item()
    for i in range(3):
        s_ref = int(find_shift(q[i], data[i], 21, amp, n))
        e_ref = float(SER_q(q[i][:, 11 + s_ref:-11], data[i][:, 11:-11 - s_ref], 2, n))
        print(f"  run {i}: reference steps shift {s_ref} SER {e_ref}")
        assert int(sh[i]) == s_ref
        assert abs(float(ser[i]) - e_ref) <= 1.0 / (N - 22 - s_ref) + 1e-6


def test_short_row_validation_keeps_the_limits():
    from vae_equalizer_amd._native import VaeqError
    from vae_equalizer_amd.engine import AWGNEngine
    eng = AWGNEngine(1, 25, A.amp_levels(4), np.full(4, 0.25, np.float32), 0.6, 0.01, "cuda:0", 2)
    with pytest.raises(VaeqError):                                            # 23 + 21 // 2 = 33 is the shortest row that keeps a symbol at every shift
        eng.validate(torch.zeros(1, 2, 64, device="cuda"), torch.zeros(1, 2, 32, dtype=torch.float16, device="cuda"), 21)


@pytest.mark.parametrize("name", ["N2100-n8", "N257-n4"])
def test_two_calls_give_identical_bits(name):
    xs = A.build_launch(name)[0]
    for mode in ("q", "y"):
        a, b = _call(xs, mode), _call(xs, mode)
        print(f"{mode}-mode {name}: GMI {a['GMI'].tolist()} {b['GMI'].tolist()}")
        for k in FIG + CNT:
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), (mode, k)


def test_both_or_neither_source_is_refused():
    from vae_equalizer_amd.engine import awgn_info
    xs = A.build_launch("N23-n2")[0]
    with pytest.raises(ValueError):
        _call(xs, "q", y=_dev(xs, "y"), amp_mean=_dev(xs, "amp_mean"), var=_dev(xs, "var"))
    with pytest.raises(ValueError):
        awgn_info(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"))


def _record_shifts(monkeypatch, cls):
    """The shifts a batch runner hands to cls.info, one [R] tensor per evaluation."""
    seen, orig = [], cls.info

    def info(self, a, data, shift, *args, **kw):
        seen.append(torch.as_tensor(shift).cpu().long())
        return orig(self, a, data, shift, *args, **kw)
    monkeypatch.setattr(cls, "info", info)
    return seen


def _check_runner_info(ser, ser0, info, shifts, R, n_eval, kept0):
    assert torch.equal(torch.nan_to_num(ser, nan=-1.0), torch.nan_to_num(ser0, nan=-1.0))     # the opt-in changes nothing it does not add
    assert set(info) == set(FIG + CNT)
    for k in FIG + CNT:
        assert tuple(info[k].shape) == (R, n_eval) and info[k].device.type == "cpu", k
        assert info[k].dtype == (torch.float32 if k in FIG else torch.int64), k
    assert torch.equal(info["kept"], kept0 - torch.stack(shifts, 1))
    assert ((info["sym_err"].double() - ser.double() * info["kept"].double()).abs() <= 1).all()   # a symbol at a threshold's rounding may differ
    assert torch.isfinite(info["AIR"]).all() and torch.isfinite(info["GMI"]).all()


@pytest.mark.parametrize("generator", ["numpy", "hip"])
def test_run_awgn_batch_reports_the_figures_of_its_validations(generator, monkeypatch):
    from vae_equalizer_amd.engine import AWGNEngine
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    from vae_equalizer_amd.shared_funcs import qam_tables
    nus = [0.0, 0.0270955, 0.1222578]
    runs = [dict(SNR=24, nu=nu, lr_optim=5e-3, seed=400 + i) for i, nu in enumerate(nus)]
    args = (runs, "64-QAM", 2, 25, 100, 1200, 300, 4, 2, "h1")
    ser0 = run_awgn_batch(*args, generator=generator, seed=11)
    shifts = _record_shifts(monkeypatch, AWGNEngine)
    ser, info = run_awgn_batch(*args, generator=generator, seed=11, want_info=True)
    print(f"run_awgn_batch[{generator}]: SER {ser.tolist()} shift {[s.tolist() for s in shifts]} " + " ".join(f"{k} {info[k].tolist()}" for k in FIG + CNT))
    assert isinstance(ser0, torch.Tensor) and len(shifts) == 2
    _check_runner_info(ser, ser0, info, shifts, 3, 2, 1178)
    H = np.array([A.entropy(qam_tables("64-QAM", nu)["P"]) for nu in nus])[:, None]
    want = 1 - (2 * H - info["GMI"].double().numpy()) / 6
    err = np.abs(info["NGMI"].double().numpy() - want)
    # the host forms H, 2 H - GMI, the quotient and the difference in float32: four roundings of values no larger than |NGMI| + 1 (an
    # unconverged 4-epoch run has GMI << 0), half a unit in the last place each
    tol = 4 * 2.0 ** -24 * (np.abs(want) + 1)
    print(f"NGMI recomputed from the pmf: max |difference| {err.max():.3e} (largest bound {tol.max():.3e})")
    assert (err <= tol).all()


@pytest.mark.parametrize("net_type,gen", [("Net", "hip"), ("Net_BN", "numpy")])
def test_run_vaenn_batch_reports_the_figures_of_its_validations(net_type, gen, monkeypatch):
    from vae_equalizer_amd.engine import NNEngine
    from vae_equalizer_amd.func_VAENN_MQAM import run_vaenn_batch
    runs = [dict(SNR=20, lr_optim=4e-3, seed=3), dict(SNR=24, lr_optim=4e-3, seed=1003)]
    args = (runs, "64-QAM", 2, 25, 25, 3, 300, 2000, 900, 4, 2, "h1")
    ser0 = run_vaenn_batch(*args, generator=gen, seed=5, net_type=net_type)
    shifts = _record_shifts(monkeypatch, NNEngine)
    ser, info = run_vaenn_batch(*args, generator=gen, seed=5, net_type=net_type, want_info=True)
    print(f"run_vaenn_batch[{net_type}]: SER {ser.tolist()} shift {[s.tolist() for s in shifts]} " + " ".join(f"{k} {info[k].tolist()}" for k in FIG + CNT))
    assert isinstance(ser0, torch.Tensor) and len(shifts) == 2
    _check_runner_info(ser, ser0, info, shifts, 2, 2, 1978)


def test_processing_want_info_is_keyword_only_and_per_run():
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as le, func_VAENN_MQAM as nn
    a = le.processing("16-QAM", 2, 20, 0.0, 25, 5e-3, 100, 600, 300, 2, 2, "h1", seed=9, verbose=False, want_info=True)
    b = nn.processing("16-QAM", 2, 20, 25, 25, 3, 4e-3, 100, 600, 300, 2, 2, "h1", "Net", seed=9, verbose=False, want_info=True)
    for ser, info in (a, b):
        print("processing:", ser.tolist(), {k: v.tolist() for k, v in info.items()})
        assert tuple(ser.shape) == (1,) and all(tuple(info[k].shape) == (1,) for k in FIG + CNT)
    with pytest.raises(TypeError):
        le.processing("16-QAM", 2, 20, 0.0, 25, 5e-3, 100, 600, 300, 2, 2, "h1", None, None, False, None, True)


VAELE_KEYS = {"SER", "SNR", "M", "lr", "N_train", "nu"}
VAENN_KEYS = {"SER", "SNR", "k2", "k1", "M", "lr", "N_train"}


@pytest.mark.parametrize("on", [False, True])
def test_eval_run_awgn_script_info_metrics(tmp_path, monkeypatch, on):
    from vae_equalizer_amd import Eval_run_shaping_vaele as ev
    monkeypatch.setattr(ev, "iter", 2); monkeypatch.setattr(ev, "num_epochs", 4); monkeypatch.setattr(ev, "N_valid", 2000)
    monkeypatch.setattr(ev, "savePATH", str(tmp_path) + "/"); monkeypatch.setattr(ev, "base_seed", 3); monkeypatch.setattr(ev, "info_metrics", on)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    print(f"info_metrics={on}: keys {sorted(m.dtype.names)}" + (f" GMI {d['GMI'].ravel().tolist()} BER {d['BER'].ravel().tolist()}" if on else ""))
    assert set(m.dtype.names) == (VAELE_KEYS | {"GMI", "NGMI", "AIR", "BER"} if on else VAELE_KEYS) and set(d) == set(m.dtype.names)
    assert d["SER"].shape == (1, 1, 1, 1, 1, 1, 2, 2)
    if on:
        for k in ("GMI", "NGMI", "AIR", "BER"):
            assert d[k].shape == d["SER"].shape and d[k].dtype == np.float32 and np.isfinite(d[k]).all(), k


@pytest.mark.parametrize("on", [False, True])
def test_eval_run_vaenn_script_info_metrics(tmp_path, monkeypatch, on):
    from vae_equalizer_amd import Eval_run_vaenn as ev
    monkeypatch.setattr(ev, "iter", 2); monkeypatch.setattr(ev, "num_epochs", 4); monkeypatch.setattr(ev, "N_valid", 2000)
    monkeypatch.setattr(ev, "train_len", 900); monkeypatch.setattr(ev, "SNR_vec", [20, 24])
    monkeypatch.setattr(ev, "savePATH", str(tmp_path) + "/"); monkeypatch.setattr(ev, "base_seed", 3); monkeypatch.setattr(ev, "info_metrics", on)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    print(f"info_metrics={on}: keys {sorted(m.dtype.names)}" + (f" GMI {d['GMI'].ravel().tolist()} BER {d['BER'].ravel().tolist()}" if on else ""))
    assert set(m.dtype.names) == (VAENN_KEYS | {"GMI", "NGMI", "AIR", "BER"} if on else VAENN_KEYS) and set(d) == set(m.dtype.names)
    assert d["SER"].shape == (2, 1, 1, 1, 1, 1, 2, 2)
    if on:
        for k in ("GMI", "NGMI", "AIR", "BER"):
            assert d[k].shape == d["SER"].shape and d[k].dtype == np.float32 and np.isfinite(d[k]).all(), k

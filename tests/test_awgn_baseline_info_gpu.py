"""vaeq_awgn_track_info (GMI, achievable rate, pre-FEC BER of an AWGN baseline's soft sequence) and vaeq_awgn_dfe_soft (the DFE's slicer input)
against the float64 model tests/_ref_awgn_baseline_info.py, and their way up through engine.awgn_track_info / awgn_dfe_soft,
run_awgn_cma_batch / run_dfe_batch(want_info=True), processing and Eval_run_shaping_cma.

Planted launches of R = 3 runs with shifts -10 / 0 / +10: Nd - 2 e in {1, 2, 11, 38, 247, 1008} (11 / 1 / 0 kept symbols up to one symbol in the
second round of the 256-thread workgroup and both sides of the shift-search length), e in {11, 31}, Nz - Nd in {0, 1}, both layouts, n_lev in
{2, 4, 8}, every hypothesis, uniform and heavily shaped pmf, var in {0.004, 0.0063, 0.01}, per-component gains != 1.
tests/test_ref_awgn_baseline_info_host.py asserts the preconditions of every case.

Bounds.  Counts are exact.  AIR / GMI / NGMI: three times _ref_awgn_baseline_info.Z_DEV, the largest deviation of the kernel's operation order
in numpy float32 from the model over these launches, computed on the CPU; the factor (tests/test_awgn_info_gpu.py's for its y-mode) allows for
the device's exp2 / log2 and another order of the radius sums.  BER: 1e-7.  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import scipy.io as io
import torch

import _ref_awgn as R
import _ref_awgn_baseline_info as B
import _ref_awgn_info as A

pytestmark = pytest.mark.gpu

Z_TOL = 3 * B.Z_DEV     # bit
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _dev(xs, key, dtype=None):
    return _t(np.stack([np.asarray(x[key]) for x in xs]), dtype)


def _z(xs):
    """The runs' tracks in the launch's layout: complex [R,Nz] (interleaved) or float [R,2,Nz] (planar)."""
    z = _dev(xs, "z")
    return z if xs[0]["interleaved"] else torch.stack([z.real, z.imag], 1).contiguous()


def _call(xs, **over):
    from vae_equalizer_amd.engine import awgn_track_info
    kw = dict(z=_z(xs), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), var=_dev(xs, "var"), shift=_dev(xs, "shift"), edge=xs[0]["edge"])
    kw.update(over)
    return awgn_track_info(**kw)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One kernel launch per planted launch, shared by the tests; -> dict of numpy arrays [R]."""
    return {k: v.cpu().numpy() for k, v in _call(B.build_launch(name)[0]).items()}


def _dev_max(got, models, keys=FIG):
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


def _check_figures(tag, got, models):
    dev = _dev_max(got, models)
    print(f"{tag}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()) + f" (bound {Z_TOL:.2e})")
    assert dev["AIR"] <= Z_TOL and dev["GMI"] <= Z_TOL
    assert dev["NGMI"] <= Z_TOL and dev["BER"] <= 1e-7


@pytest.mark.parametrize("name", B.LAUNCHES)
def test_counts_equal_the_model(name):
    got, models = _run(name), B.build_launch(name)[1]
    print(f"{name}: " + ", ".join(f"{k} {got[k].tolist()}" for k in CNT) + f"; model {[[m[k] for m in models] for k in CNT]}")
    _check_counts_and_nan(got, models)


@pytest.mark.parametrize("name", B.LAUNCHES)
def test_figures(name):
    _check_figures(name, _run(name), B.build_launch(name)[1])


def test_empty_window_zero_track_and_a_kept_run_in_one_launch():
    """shift = -e (data[:, e:0] is empty), a run whose z is zero throughout (no normalisation), and a run that keeps its symbols between them."""
    for name in ("D38-e11-dz0-il0-n8", "D38-e31-dz1-il1-n4"):
        xs = [dict(x) for x in B.build_launch(name)[0]]
        xs[0]["shift"] = -xs[0]["edge"]
        xs[2]["z"] = np.zeros_like(xs[2]["z"])
        xs = [xs[0], xs[1], xs[2]]
        got = {k: v.cpu().numpy() for k, v in _call(xs).items()}
        models = [B.model(x) for x in xs]
        print(f"{name}: " + ", ".join(f"{k} {got[k].tolist()}" for k in FIG + CNT))
        assert [m["kept"] for m in models] == [0, 38, 0]
        _check_counts_and_nan(got, models)
        _check_figures(name, got, models)


def test_shifts_nobody_clamps():
    """-12 and +11, what find_shift_symb(., ., 24) can return, at e = 31."""
    xs, models = B.build_launch("wide")
    got = {k: v.cpu().numpy() for k, v in _call(xs[:1]).items()}              # Nz = Nd + 1
    got0 = {k: v.cpu().numpy() for k, v in _call(xs[1:]).items()}
    print("wide: " + ", ".join(f"{k} {got[k].tolist()} {got0[k].tolist()}" for k in FIG + CNT))
    assert [m["kept"] for m in models] == [250, 227, 250]
    _check_counts_and_nan(got, models[:1])
    _check_figures("wide (Nz = Nd + 1)", got, models[:1])
    _check_counts_and_nan(got0, models[1:])
    _check_figures("wide (Nz = Nd)", got0, models[1:])


@pytest.mark.parametrize("name", ["D1008-e31-dz1-il1-n8", "D247-e11-dz0-il0-n4"])
def test_two_calls_give_identical_bits_and_a_batch_the_bits_of_single_calls(name):
    xs = B.build_launch(name)[0]
    a, b = _call(xs), _call(xs)
    singles = [_call([x]) for x in xs]
    print(f"{name}: GMI {a['GMI'].tolist()} {b['GMI'].tolist()} {[s['GMI'].item() for s in singles]}")
    for k in FIG + CNT:
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), k
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(torch.cat([s[k] for s in singles]), nan=-1.0)), k


def test_layout_follows_from_the_dtype_and_shapes_are_checked():
    from vae_equalizer_amd.engine import awgn_track_info
    xs = B.build_launch("D38-e11-dz0-il0-n4")[0]
    z = _dev(xs, "z")
    a, b = _call(xs, z=z), _call(xs, z=torch.stack([z.real, z.imag], 1).contiguous())
    for k in FIG + CNT:
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), k
    with pytest.raises(ValueError):
        _call(xs, z=torch.stack([z.real, z.imag], 2).contiguous())          # a float [R,Nz,2] is neither layout
    from vae_equalizer_amd._native import VaeqError
    with pytest.raises(VaeqError):
        _call(xs, z=z[:, :-1].contiguous())                                   # Nz = Nd - 1


# ------------------------------------------------------------------ through the validators, on conditioned frames
def _ratio(info):
    return info["sym_err"].float() / info["kept"].float()


@pytest.mark.parametrize("i", range(len(B.CMA_BATCHES)), ids=lambda i: f"K{B.CMA_BATCHES[i]['K']}")
def test_cma_validator_ser_is_sym_err_over_kept(i):
    from vae_equalizer_amd.engine import awgn_cma_validate, awgn_track_info
    b, frames = B.CMA_BATCHES[i], B.cma_batch(i)
    rx, h, data = (_t(np.stack([f[k] for f in frames])) for k in ("rx", "h", "data"))
    ser, shift, y = awgn_cma_validate(rx, h, data, frames[0]["levels"], b["sps"], b["n_shift"], want_cpe=True)
    P = np.full(b["n_lev"], 1.0 / b["n_lev"], np.float32)
    info = awgn_track_info(y, data, frames[0]["levels"], P, 0.01, shift, 11)
    yh = y.cpu().numpy()
    models = [B.track_info(yh[r, 0] + 1j * yh[r, 1], f["data"], P, f["levels"], 0.01, int(shift[r]), 11) for r, f in enumerate(frames)]
    print(f"K{b['K']}: shift {shift.tolist()} SER {ser.tolist()} sym_err / kept {_ratio(info).tolist()} kept {info['kept'].tolist()} hyp {info['hyp'].tolist()}"
          f" GMI {info['GMI'].tolist()} model {[m['GMI'] for m in models]}")
    assert shift.tolist() == [r["lag"] for r in b["runs"]] and info["kept"].tolist() == [b["K"] - 22 - r["lag"] for r in b["runs"]]
    assert torch.equal(_ratio(info), ser)
    assert info["sym_err"].tolist() == [r["n_err"] for r in b["runs"]] == [m["sym_err"] for m in models]
    assert info["hyp"].tolist() == [m["hyp"] for m in models] and info["bit_err"].tolist() == [m["bit_err"] for m in models]


def test_lmmse_validator_ser_is_sym_err_over_kept():
    """Three conditioned frames and _ref_awgn.longer_slice_frame, whose one extra sample of the slice decides a symbol: Nz = N + 1."""
    from vae_equalizer_amd.engine import awgn_lmmse_eval, awgn_track_info
    K, N, n_cut, n_shift, n_lev = B.LMMSE_CASE
    frames = B.lmmse_frames()
    rx, data = (_t(np.stack([f[k] for f in frames])) for k in ("rx", "data"))
    taps = torch.from_numpy(np.stack([f["taps"] for f in frames]))
    ser, shift, dec, out = awgn_lmmse_eval(rx, taps, data, frames[0]["levels"], n_shift, n_cut, want_out=True)
    P = np.full(n_lev, 0.25, np.float32)
    info = awgn_track_info(out, data, frames[0]["levels"], P, 0.01, shift, n_cut + 11)
    oh = out.cpu().numpy()
    models = [B.track_info(oh[r], f["data"], P, f["levels"], 0.01, int(shift[r]), n_cut + 11) for r, f in enumerate(frames)]
    print(f"LMMSE: shift {shift.tolist()} SER {ser.tolist()} sym_err / kept {_ratio(info).tolist()} kept {info['kept'].tolist()} sym_err {info['sym_err'].tolist()}")
    assert tuple(out.shape) == (4, N + 1) and info["kept"].tolist() == [N - 22 - 2 * n_cut - int(s) for s in shift]
    assert torch.equal(_ratio(info), ser)
    assert info["sym_err"].tolist() == [4, 5, 6, 3] == [m["sym_err"] for m in models]      # the last: 4 if the extra sample were left out of the scale
    assert info["hyp"].tolist() == [m["hyp"] for m in models] and info["bit_err"].tolist() == [m["bit_err"] for m in models]


@pytest.mark.parametrize("case", B.DFE_CASES, ids=lambda c: f"n{c[0]}-K2_{c[1]}-N{c[2]}")
def test_dfe_soft_sequence_and_its_figures(case):
    from vae_equalizer_amd.engine import awgn_dfe, awgn_dfe_soft, awgn_track_info
    n_lev, K2, N, outliers = case
    frames = B.dfe_frames(case)
    lev = frames[0]["levels"]
    ffp = np.stack([f["ff"] for f in frames])
    rx = _t(np.stack([ffp.real, ffp.imag], 1).astype(np.float32))               # the feed-forward output itself, through a one-tap identity FIR
    fb = torch.from_numpy(np.stack([f["fb"] for f in frames]))
    data = _t(np.stack([f["data"] for f in frames]))
    r = awgn_dfe(rx, torch.tensor([1.0 + 0.0j], dtype=torch.cfloat), fb, _t(np.stack([f["init"] for f in frames])), lev, data, 24, 20, want_ff=True)
    z = awgn_dfe_soft(r["ff"], fb, r["dec"], lev)
    zh, ffh, dec = z.cpu().numpy(), r["ff"].cpu().numpy(), r["dec"].cpu().numpy().astype(np.int64)
    l32 = lev.astype(np.float32)
    for i, f in enumerate(frames):
        assert np.array_equal(dec[i], f["expected"]) and np.array_equal(ffh[i], f["ff"])
        c = (l32[dec[i, :K2] // n_lev] + 1j * l32[dec[i, :K2] % n_lev]).astype(np.complex64)
        assert np.array_equal(zh[i, :K2], c)                                    # exactly the state the reference holds there
        near = R.slice_axis(zh[i].real, lev)[0] * n_lev + R.slice_axis(zh[i].imag, lev)[0]
        assert np.array_equal(near[K2:], dec[i, K2:])
        model = B.dfe_soft(ffh[i], f["fb"], dec[i], lev)
        err, bound = np.abs(zh[i] - model)[K2:], B.dfe_soft_bound(ffh[i], f["fb"], dec[i], lev)[K2:]
        print(f"run {i}: max |z - model| {err.max():.3e}, largest fraction of its bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()
    P = np.full(n_lev, 1.0 / n_lev, np.float32)
    info = awgn_track_info(z, data, lev, P, 0.01, r["shift"], 31)
    print(f"DFE: shift {r['shift'].tolist()} SER {r['ser'].tolist()} sym_err / kept {_ratio(info).tolist()} kept {info['kept'].tolist()} GMI {info['GMI'].tolist()}")
    assert info["kept"].tolist() == [N - 62 - int(s) for s in r["shift"]] and torch.equal(_ratio(info), r["ser"])
    assert (info["sym_err"] > 0).all() and torch.isfinite(info["GMI"]).all()


# ------------------------------------------------------------------ the host layers
def _check_info(info, ser, shape, kept):
    assert set(info) == set(FIG + CNT)
    for k in FIG + CNT:
        assert tuple(info[k].shape) == shape and info[k].device.type == "cpu", k
        assert info[k].dtype == (torch.float32 if k in FIG else torch.int64), k
    assert torch.equal(info["kept"], kept)
    # SER kept is a whole number of symbols; it is rounded back to one because the float32 SER times kept misses it by up to 1e-6, which would
    # turn a difference of exactly one symbol into 1.0000005
    assert ((info["sym_err"].double() - torch.round(ser.double() * info["kept"].double())).abs() <= 1).all()
    assert torch.isfinite(info["AIR"]).all() and torch.isfinite(info["GMI"]).all()


def _check_ngmi(info, H, n_lev):
    want = 1 - (2 * H - info["GMI"].double().numpy()) / (2 * np.log2(n_lev))
    err = np.abs(info["NGMI"].double().numpy() - want)
    # the host forms H, 2 H - GMI, the quotient and the difference in float32: four roundings of values no larger than |NGMI| + 1, half a unit
    # in the last place each (tests/test_awgn_info_gpu.py)
    tol = 4 * 2.0 ** -24 * (np.abs(want) + 1)
    print(f"NGMI recomputed from the pmf: max |difference| {err.max():.3e} (largest bound {tol.max():.3e})")
    assert (err <= tol).all()


@pytest.mark.parametrize("generator", ["numpy", "hip"])
def test_run_awgn_cma_batch_reports_the_figures_of_its_validations(generator, monkeypatch):
    from vae_equalizer_amd import func_CMA_MQAM_shaping as cm
    from vae_equalizer_amd.shared_funcs import qam_tables
    nus = [0.0, 0.1222578]
    runs = [dict(SNR=22, nu=nu, lr_optim=0.5e-4, seed=500 + i) for i, nu in enumerate(nus)]
    args = (runs, "16-QAM", 2, 25, 2000, 1000, 4, 2, "h1")
    ser0 = cm.run_awgn_cma_batch(*args, generator=generator, seed=11)
    shifts, orig = [], cm.awgn_track_info

    def rec(z, data, amp, P, var, shift, edge=11):
        shifts.append((torch.as_tensor(shift).cpu().long(), edge, [float(v) for v in var]))
        return orig(z, data, amp, P, var, shift, edge)
    monkeypatch.setattr(cm, "awgn_track_info", rec)
    ser, info = cm.run_awgn_cma_batch(*args, generator=generator, seed=11, want_info=True)
    print(f"run_awgn_cma_batch[{generator}]: SER {ser.tolist()} shift {[s[0].tolist() for s in shifts]} " + " ".join(f"{k} {info[k].tolist()}" for k in FIG + CNT))
    assert isinstance(ser0, torch.Tensor) and len(shifts) == 2 and all(s[1] == 11 and s[2] == [10 ** -2.2] * 2 for s in shifts)
    assert torch.equal(torch.nan_to_num(ser, nan=-1.0), torch.nan_to_num(ser0, nan=-1.0))     # the opt-in changes nothing it does not add
    _check_info(info, ser, (2, 2), 1978 - torch.stack([s[0] for s in shifts], 1))
    _check_ngmi(info, np.array([A.entropy(qam_tables("16-QAM", nu)["P"]) for nu in nus])[:, None], 4)


@pytest.mark.parametrize("generator", ["numpy", "hip"])
def test_run_dfe_batch_reports_the_figures_of_both_curves(generator):
    from vae_equalizer_amd import DFE_MQAM_shaping as D
    from vae_equalizer_amd import channel as ch
    args = ([16, 20], 2, 4000, "16-QAM")
    kw = dict(nu=0.0872449, seed=5, generator=generator)
    r0 = D.run_dfe_batch(*args, **kw)
    r = D.run_dfe_batch(*args, **kw, want_info=True)
    assert set(r) == set(r0) | {"info_mmse", "info_dfe"}
    P = ch.pcs_probabilities(D.qam_constants("16-QAM")["amp_levels"].numpy(), 0.0872449)
    for tag in ("mmse", "dfe"):
        info, ser = r["info_" + tag], r["SER_" + tag]
        print(f"run_dfe_batch[{generator}] {tag}: SER {ser.tolist()} shift {r['shift_' + tag].tolist()} " + " ".join(f"{k} {info[k].tolist()}" for k in FIG + CNT))
        assert torch.equal(ser, r0["SER_" + tag]) and np.array_equal(r["shift_" + tag], r0["shift_" + tag])
        _check_info(info, ser, (2, 2), 4000 - 62 - torch.from_numpy(r["shift_" + tag]).long())
        _check_ngmi(info, A.entropy(P), 4)


def test_dfe_script_main_returns_the_dicts_only_when_asked(monkeypatch):
    from vae_equalizer_amd import DFE_MQAM_shaping as D
    monkeypatch.setattr(D, "SNR_vec", np.array([18])); monkeypatch.setattr(D, "num_epochs", 1); monkeypatch.setattr(D, "N_valid", 4000)
    monkeypatch.setattr(D, "base_seed", 3)
    assert D.info_metrics is False
    a = D.main()
    monkeypatch.setattr(D, "info_metrics", True)
    b = D.main()
    assert len(a) == 2 and len(b) == 4 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(b[2]) == set(b[3]) == set(FIG + CNT) and tuple(b[2]["GMI"].shape) == (1, 1)


def test_processing_want_info_is_keyword_only_and_per_run():
    from vae_equalizer_amd import func_CMA_MQAM_shaping as cm
    args = ("16-QAM", 2, 22, 0.0, 25, 0.5e-4, 2000, 1000, 2, 2, "h1")
    ser0 = cm.processing(*args, seed=9, verbose=False)
    ser, info = cm.processing(*args, seed=9, verbose=False, want_info=True)
    print("processing:", ser.tolist(), {k: v.tolist() for k, v in info.items()})
    assert isinstance(ser0, torch.Tensor) and torch.equal(ser0, ser)
    assert tuple(ser.shape) == (1,) and all(tuple(info[k].shape) == (1,) for k in FIG + CNT)
    with pytest.raises(TypeError):
        cm.processing(*args, None, None, False, None, True)
    with pytest.raises(TypeError):
        cm.processing(*args, seed=9, verbose=False, want_infos=True)             # an option nobody knows is refused like a misspelt keyword


CMA_KEYS = {"SER", "SNR", "M", "lr", "nu"}


@pytest.mark.parametrize("on", [False, True])
def test_eval_run_cma_script_info_metrics(tmp_path, monkeypatch, on):
    from vae_equalizer_amd import Eval_run_shaping_cma as ev
    monkeypatch.setattr(ev, "iter", 2); monkeypatch.setattr(ev, "num_epochs", 4); monkeypatch.setattr(ev, "N_valid", 2000)
    monkeypatch.setattr(ev, "train_len", 1000); monkeypatch.setattr(ev, "mod", "16-QAM")
    monkeypatch.setattr(ev, "savePATH", str(tmp_path) + "/"); monkeypatch.setattr(ev, "base_seed", 3); monkeypatch.setattr(ev, "info_metrics", on)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    print(f"info_metrics={on}: keys {sorted(m.dtype.names)}" + (f" GMI {d['GMI'].ravel().tolist()} BER {d['BER'].ravel().tolist()}" if on else ""))
    assert set(m.dtype.names) == (CMA_KEYS | {"GMI", "NGMI", "AIR", "BER"} if on else CMA_KEYS) and set(d) == set(m.dtype.names)
    assert d["SER"].shape == (1, 1, 1, 1, 1, 1, 2, 2)
    if on:
        for k in ("GMI", "NGMI", "AIR", "BER"):
            assert d[k].shape == d["SER"].shape and d[k].dtype == np.float32 and np.isfinite(d[k]).all(), k

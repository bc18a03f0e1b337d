"""vaeq_dp_epilogue_llr (the per-bit a-posteriori LLRs of a DP frame) against the float64 model tests/_ref_llr.py, through engine.dp_epilogue_llr,
engine.label_bits and run_dp_batch(want_llr=True).

Launches are tests/_ref_info.py's: R = 3 runs, N in {43, 47, 400, 1030} (shorter than, and five tiles of, the 256-symbol tile), batch_len in
{0, 20, 100}, n_lev in {2, 4, 8}, shifts -10 / 0 / +10 unequal between the polarisations, both r, every hypothesis, uniform and heavily shaped
pmf.  tests/test_ref_llr_host.py pins the model to the information-rate models on the CPU.

Bounds.  q-mode: an LLR is ln 2 times a difference of two float32 log2 of set sums of the same float32 q, each good to the project's Q_TOL =
1e-4 bit (tests/test_epilogue_info_gpu.py): 2 Q_TOL ln 2 nats.  y-mode: |kernel - model| / max(1, |model|) <= 4 Y_LLR_DEV, Y_LLR_DEV the cost of
float32 in the kernel's operation order computed on the CPU; the factor allows for the device's exp2 / log2 (1-ulp approximations where numpy
rounds correctly) and for contraction to fused multiply-adds.  The GMI recomputed from the kernel's LLRs is 1-Lipschitz in each of its 2 b
terms per symbol, so it lies within 2 b (LLR bound in bit) plus the information-rate kernel's own bound of that kernel's GMI.
Measured on the MI355X: q-mode 6.2e-7 nats at most, y-mode 3.6e-7 relative with |lam| up to 400 nats.  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_epilogue as E
import _ref_info as I
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
Q_TOL = 1e-4                    # bit, the project's bound for one float32 log2 (set by the issue)
Q_LLR_TOL = 2 * Q_TOL * LN2     # nats: a difference of two
Y_LLR_TOL = 4 * L.Y_LLR_DEV     # relative to max(1, |lam|)
Y_INFO_TOL = 3 * I.Y_DEV        # bit: tests/test_epilogue_info_gpu.py's bound of the information-rate kernel's y-mode GMI


def _dev(xs, key, dtype=None):
    a = np.stack([np.asarray(x[key]) for x in xs])
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _src(xs, mode):
    if mode == "q":
        return dict(q=_dev(xs, "q"))
    return dict(y=_dev(xs, "y"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"))


def _llr(xs, mode, hyp, **over):
    from vae_equalizer_amd.engine import dp_epilogue_llr
    kw = dict(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), r=_dev(xs, "r"), hyp=torch.as_tensor(np.asarray(hyp)).cuda(),
              batch_len=xs[0]["batch_len"], **_src(xs, mode))
    kw.update(over)
    return dp_epilogue_llr(**kw)


def _info(xs, mode):
    from vae_equalizer_amd.engine import dp_epilogue_info
    return dp_epilogue_info(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), r=_dev(xs, "r"),
                            batch_len=xs[0]["batch_len"], **_src(xs, mode))


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    """-> (planes[R,2,2b,N] float64, mask[R,2,N]) under the information-rate model's hypotheses; computed once, never modified."""
    xs, mq, my = I.build_launch(name)
    out = []
    for x, m in zip(xs, mq if mode == "q" else my):
        if mode == "q":
            out.append(L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], m["hyp"], x["batch_len"]))
        else:
            out.append(L.dp_llr_y(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], m["hyp"], x["batch_len"]))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    """One information-rate launch and one LLR launch under its hypotheses per (launch, mode), shared by the tests."""
    xs = I.build_launch(name)[0]
    fig = {k: v.cpu().numpy() for k, v in _info(xs, mode).items()}
    return fig, _llr(xs, mode, fig["hyp"]).cpu().numpy()


def _erasures_are_plus_zero(got, mask):
    m = np.broadcast_to(mask[:, :, None, :], got.shape)
    return not got.view(np.uint32)[~m].any()


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_q_mode_against_the_model(name):
    (fig, got), (want, mask) = _run(name, "q"), _model(name, "q")
    models = I.build_launch(name)[1]
    assert np.array_equal(fig["hyp"], np.stack([m["hyp"] for m in models]))
    m = np.broadcast_to(mask[:, :, None, :], want.shape)
    dev = float(np.abs(got.astype(np.float64) - want)[m].max()) if m.any() else 0.0
    print(f"q-mode {name}: max |kernel - model| {dev:.3e} nats over {int(m.sum())} kept entries, largest |lam| {np.abs(want).max():.1f}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert dev <= Q_LLR_TOL
    assert _erasures_are_plus_zero(got, mask)


@pytest.mark.parametrize("name", I.LAUNCHES)
def test_y_mode_against_the_model(name):
    (fig, got), (want, mask) = _run(name, "y"), _model(name, "y")
    models = I.build_launch(name)[2]
    assert np.array_equal(fig["hyp"], np.stack([m["hyp"] for m in models]))
    dev = L.rel_dev(got, want, mask)
    print(f"y-mode {name}: max |kernel - model| / max(1, |model|) {dev:.3e}, largest |lam| {np.abs(want).max():.1f} nats")
    assert np.isfinite(got).all()
    assert dev <= Y_LLR_TOL
    assert _erasures_are_plus_zero(got, mask)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", I.LAUNCHES)
def test_every_hypothesis_is_a_plane_transform_of_the_first(name, mode):
    """hyp = h gives, bit for bit, the hyp = 0 output with planes exchanged and top-bit planes negated; hyp = 8 + h gives the bits of h."""
    xs = I.build_launch(name)[0]
    mask = _model(name, mode)[1]
    m = np.broadcast_to(mask[:, :, None, :], (3, 2, 2 * L.nbits(xs[0]["n"]), mask.shape[-1]))
    base = _llr(xs, mode, np.zeros((3, 2), np.int64)).cpu().numpy()
    for h in range(8):
        got = _llr(xs, mode, np.full((3, 2), h, np.int64)).cpu().numpy()
        want = np.where(m, L.retransform(base, h, xs[0]["n"]), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, mode, h)
        got8 = _llr(xs, mode, np.full((3, 2), 8 + h, np.int64)).cpu().numpy()
        assert np.array_equal(got8.view(np.uint32), got.view(np.uint32)), (name, mode, 8 + h)


def _gmi_and_sign_errors(llr, bits, mask, P):
    """Host float64, per (run, polarisation): GMI recomputed from LLRs and TX label bits, and the LLR signs that disagree with the bits."""
    R = llr.shape[0]
    gmi, err = np.full((R, 2), np.nan), np.zeros((R, 2), np.int64)
    for i in range(R):
        for p in range(2):
            gmi[i, p] = L.gmi_from_llr(llr[i, p], bits[i, p], mask[i, p], I.entropy(P[i]))
            err[i, p] = L.sign_errors(llr[i, p], bits[i, p], mask[i, p])
    return gmi, err


def _gmi_tol(mode, n, llr, mask):
    """2 b (LLR bound in bit) + the information-rate kernel's own bound."""
    b2 = 2 * L.nbits(n)
    if mode == "q":
        return b2 * (Q_LLR_TOL / LN2) + Q_TOL
    big = float(np.abs(llr[np.broadcast_to(mask[:, :, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return b2 * (Y_LLR_TOL * max(1.0, big) / LN2) + Y_INFO_TOL


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", I.LAUNCHES)
def test_sign_errors_and_gmi_are_the_information_rate_kernels(name, mode):
    from vae_equalizer_amd.engine import label_bits
    xs = I.build_launch(name)[0]
    fig, got = _run(name, mode)
    mask = _model(name, mode)[1]
    bits = label_bits(_dev(xs, "tx"), xs[0]["n"])
    assert bits.dtype == torch.int8 and bits.is_cuda and tuple(bits.shape) == got.shape
    bits = bits.cpu().numpy().astype(np.int64)
    assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], x["n"]) for x in xs]))
    gmi, err = _gmi_and_sign_errors(got, bits, mask, [x["P"] for x in xs])
    tol = _gmi_tol(mode, xs[0]["n"], got, mask)
    kept = fig["kept"] > 0
    d = float(np.abs(gmi - fig["GMI"])[kept].max()) if kept.any() else 0.0
    print(f"{mode}-mode {name}: sign errors {err.tolist()} bit_err {fig['bit_err'].tolist()}; max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"])
    assert np.array_equal(err, fig["bit_err"])
    assert np.array_equal(np.isnan(gmi), ~kept) and d <= tol


@pytest.mark.parametrize("n", [2, 8])
def test_an_exact_zero_in_q_gives_finite_llrs(n):
    """A stored posterior of exactly 0 at a transmitted level: at n_lev = 2 a whole set sum is 0 and costs 126 bit, not infinity."""
    x = dict(I.make_run(seed=7, N=300, n=n, shift=(0, 0), r=0, hyp=0, batch_len=None, nu=0.0, var=(0.004, 0.004), n_err=(0, 0)))
    t = int(E.tx_levels(x["tx"], n)[0, 0, 100])
    q = x["q"].copy()
    q[0, t, 100] = 0.0
    x["q"] = q
    got = _llr([x], "q", np.zeros((1, 2), np.int64)).cpu().numpy()[0]
    want, mask = L.dp_llr_q(q, n, x["shift"], 0, (0, 0))
    dev = float(np.abs(got - want).max())
    print(f"exact zero, n_lev {n}: LLRs of the symbol {got[0, :, 100].tolist()} model {want[0, :, 100].tolist()}; max |kernel - model| {dev:.3e}")
    assert mask[0, 100] and np.isfinite(got).all() and dev <= Q_LLR_TOL
    if n == 2:
        assert 122 * LN2 < abs(want[0, 0, 100]) <= 126 * LN2                  # ln 2 (-126 - log2 of the other posterior, 0.1 .. 0.45)


def test_an_empty_window_gives_all_zeros():
    x = I.make_run(seed=11, N=60, n=8, shift=(10, 10), r=0, hyp=0, batch_len=20, nu=0.0, var=(0.004, 0.004), n_err=(0, 0))
    for mode in ("q", "y"):
        got = _llr([x], mode, np.full((1, 2), 5, np.int64)).cpu().numpy()
        assert got.shape == (1, 2, 6, 60) and not got.view(np.uint32).any(), mode


@pytest.mark.parametrize("name", ["N1030-B0-n8", "N400-B100-n4"])
def test_two_calls_and_single_run_calls_give_identical_bits(name):
    xs = I.build_launch(name)[0]
    hyp = np.array([[1, 6], [4, 3], [7, 2]], np.int64)
    for mode in ("q", "y"):
        a, b = _llr(xs, mode, hyp), _llr(xs, mode, hyp)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), mode
        for i in range(3):
            one = _llr(xs[i:i + 1], mode, hyp[i:i + 1])
            assert torch.equal(one.view(torch.int32), a[i:i + 1].view(torch.int32)), (mode, i)


def test_both_or_neither_source_is_refused():
    from vae_equalizer_amd.engine import dp_epilogue_llr
    xs = I.build_launch("N43-B0-n2")[0]
    hyp = np.zeros((3, 2), np.int64)
    with pytest.raises(ValueError):
        _llr(xs, "q", hyp, y=_dev(xs, "y"))
    with pytest.raises(ValueError):
        dp_epilogue_llr(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), r=_dev(xs, "r"), hyp=torch.zeros(3, 2).cuda())


# ------------------------------------------------------------------ run_dp_batch(want_llr=True)
NUS = [0.0, 0.0270955, 0.1222578]


def _batch(**over):
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    runs = [DPRun(22 + i, NUS[i], 0.01, 0.3, 2.5e-3, 90e9, seed=300 + i) for i in range(3)]
    kw = dict(mod="64-QAM", sps=2, M_est=25, batch_len=100, N_frame_max=1000, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24,
              tau_pmd=0.1e-12 * np.sqrt(1000), phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170)
    kw.update(over)
    return run_dp_batch(runs, **kw)


def test_run_dp_batch_returns_the_last_frames_llrs():
    """want_llr=True with keep_last: "llr" is dp_epilogue_llr on the returned last frame (q-mode: its q is materialised) under the hypothesis of
    that frame's info, the bits are label_bits of its TX reference, the GMI recomputed from both is the reported one, and nothing else changes."""
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.engine import dp_epilogue_llr, label_bits
    a = _batch(keep_last=True, want_info=True, want_llr=True)
    b = _batch(keep_last=True, want_info=True, want_llr=False)
    assert "llr" not in b and set(a) - set(b) == {"llr"}
    for k in ("SER", "Var_est", "var"):
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), k
    for k in a["info"]:
        assert torch.equal(torch.nan_to_num(a["info"][k], nan=-1.0), torch.nan_to_num(b["info"][k], nan=-1.0)), k
    for k in ("q", "y", "data", "rx", "shift_q", "r_q", "shift_c", "r_c", "SER"):
        assert torch.equal(a["last"][k], b["last"][k]), k
    assert torch.equal(a["engine"].W, b["engine"].W)
    last, out = a["last"], a["llr"]
    llr, bits, hyp = out["llr"], out["bits"], out["hyp"]
    assert llr.is_cuda and llr.dtype == torch.float32 and tuple(llr.shape) == (3, 2, 6, 1000)
    assert bits.is_cuda and bits.dtype == torch.int8 and tuple(bits.shape) == (3, 2, 6, 1000) and tuple(hyp.shape) == (3, 2)
    assert torch.equal(hyp.cpu(), a["info"]["hyp"][:, :, -1])
    tabs = [sfun.qam_tables("64-QAM", nu) for nu in NUS]
    again = dp_epilogue_llr(q=last["q"], amp_levels=tabs[0]["amps"], shift=last["shift_q"], r=last["r_q"], hyp=hyp, batch_len=100)
    assert torch.equal(llr.view(torch.int32), again.view(torch.int32))
    assert torch.equal(bits, label_bits(last["data"], 8))
    # the kept window from the frame's own alignment, the GMI from the returned LLRs and bits in float64
    sh, r = last["shift_q"].cpu().numpy(), last["r_q"].cpu().numpy()
    mask = np.zeros((3, 2, 1000), bool)
    for i in range(3):
        idx = E.kept_indices(1000, sh[i], 100)
        for p in range(2):
            m = idx + int(sh[i, p])
            mask[i, p, idx[(m >= 0) & (m < 1000)]] = True
    llr_n, bits_n = llr.cpu().numpy(), bits.cpu().numpy().astype(np.int64)
    gmi, err = _gmi_and_sign_errors(llr_n, bits_n, mask, [t["P"] for t in tabs])
    want = a["info"]["GMI"][:, :, -1].numpy()
    tol = _gmi_tol("q", 8, llr_n, mask)
    print(f"run_dp_batch last frame: GMI from the LLRs {gmi.tolist()} reported {want.tolist()} (bound {tol:.2e}); sign errors {err.tolist()}")
    assert np.array_equal(mask.sum(-1), a["info"]["kept"][:, :, -1].numpy()) and (mask.sum(-1) > 800).all()
    assert not llr_n.view(np.uint32)[~np.broadcast_to(mask[:, :, None, :], llr_n.shape)].any()
    assert np.array_equal(err, a["info"]["bit_err"][:, :, -1].numpy())
    assert np.abs(gmi - want).max() <= tol


def test_run_dp_batch_llrs_do_not_depend_on_the_stream_schedule(monkeypatch):
    """generator="hip" without keep_last: the three-stream path (y-mode LLRs made on the epilogue stream) and the serial order agree bit for bit."""
    monkeypatch.delenv("VAEQ_SERIAL_FRAMES", raising=False)
    a = _batch(generator="hip", want_llr=True)
    monkeypatch.setenv("VAEQ_SERIAL_FRAMES", "1")
    b = _batch(generator="hip", want_llr=True)
    c = _batch(generator="hip", want_llr=False)
    assert "llr" not in c and "info" not in a
    assert torch.equal(torch.nan_to_num(a["SER"], nan=-1.0), torch.nan_to_num(b["SER"], nan=-1.0))
    assert torch.equal(torch.nan_to_num(b["SER"], nan=-1.0), torch.nan_to_num(c["SER"], nan=-1.0))
    assert torch.equal(b["Var_est"], c["Var_est"])
    for k in ("llr", "bits", "hyp"):
        x, y = a["llr"][k], b["llr"][k]
        assert x.is_cuda and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k
    assert a["llr"]["llr"].abs().max().item() > 1.0 and torch.isfinite(a["llr"]["llr"]).all()

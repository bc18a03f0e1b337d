"""vaeq_awgn_llr (the per-bit a-posteriori LLRs of an AWGN validation frame) against the float64 model tests/_ref_llr.py, through engine.awgn_llr,
AWGNEngine.llr and NNEngine.llr.

Launches are tests/_ref_awgn_info.py's: R = 3 runs with shifts -10 / 0 / +10, N in {23, 24, 33, 60, 257, 1030, 2100} (11 / 1 / 0 kept symbols, one
symbol in the second round of the 256-thread workgroup, several rounds), n_lev in {2, 4, 8}, component gains 0.7 / 1.9, the four hypotheses.

Bounds, as in tests/test_epilogue_llr_gpu.py.  q-mode: 2 Q_TOL ln 2 nats.  y-mode: |kernel - model| / max(1, |model|) <= 4 Y_LLR_DEV_AWGN, the cost
of float32 in the kernel's operation order computed on the CPU (the float32 sum behind m_c moves the scale of every sample; the factor allows
for the device's exp2 / log2, contraction, and the device's order of the 256 partial sums).  GMI from the LLRs: 2 b (LLR bound in bit) plus the
bound of vaeq_awgn_info's own GMI.  Measured on the MI355X: q-mode 5.9e-7 nats at most, y-mode 3.7e-6 relative.  Every test prints its figures before it
asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_awgn_info as A
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
Q_TOL = 1e-4                        # bit, the project's bound for one float32 log2
Q_LLR_TOL = 2 * Q_TOL * LN2         # nats
Y_LLR_TOL = 4 * L.Y_LLR_DEV_AWGN    # relative to max(1, |lam|)
Y_INFO_TOL = 3 * A.Y_DEV            # bit: tests/test_awgn_info_gpu.py's bound of vaeq_awgn_info's y-mode GMI


def _dev(xs, key):
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x[key]) for x in xs]))).cuda()


def _src(xs, mode):
    if mode == "q":
        return dict(q=_dev(xs, "q"))
    return dict(y=_dev(xs, "y"), amp_mean=_dev(xs, "amp_mean"), var=_dev(xs, "var"))


def _llr(xs, mode, hyp, **over):
    from vae_equalizer_amd.engine import awgn_llr
    kw = dict(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), hyp=torch.as_tensor(np.asarray(hyp)).cuda(), **_src(xs, mode))
    kw.update(over)
    return awgn_llr(**kw)


def _info(xs, mode):
    from vae_equalizer_amd.engine import awgn_info
    return awgn_info(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), **_src(xs, mode))


def _model_of(xs, mode, hyps):
    out = []
    for x, h in zip(xs, hyps):
        if mode == "q":
            out.append(L.awgn_llr_q(x["q"], x["n"], x["shift"], h))
        else:
            out.append(L.awgn_llr_y(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], h))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    """-> (planes[R,2b,N] float64, mask[R,N]) under the information-rate model's hypotheses; computed once, never modified."""
    xs, mq, my = A.build_launch(name)
    return _model_of(xs, mode, [m["hyp"] for m in (mq if mode == "q" else my)])


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    """One vaeq_awgn_info launch and one LLR launch under its hypotheses per (launch, mode), shared by the tests."""
    xs = A.build_launch(name)[0]
    fig = {k: v.cpu().numpy() for k, v in _info(xs, mode).items()}
    return fig, _llr(xs, mode, fig["hyp"]).cpu().numpy()


def _zeros_exactly_outside(got, mask):
    m = np.broadcast_to(mask[:, None, :], got.shape)
    return not got.view(np.uint32)[~m].any()


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_q_mode_against_the_model(name):
    (fig, got), (want, mask) = _run(name, "q"), _model(name, "q")
    xs, models = A.build_launch(name)[:2]
    assert [int(h) for h in fig["hyp"]] == [m["hyp"] for m in models]
    m = np.broadcast_to(mask[:, None, :], want.shape)
    dev = float(np.abs(got.astype(np.float64) - want)[m].max()) if m.any() else 0.0
    print(f"q-mode {name}: max |kernel - model| {dev:.3e} nats over {int(m.sum())} kept entries, largest |lam| {np.abs(want).max():.1f}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert dev <= Q_LLR_TOL
    for i, x in enumerate(xs):                                                # exact zeros lie outside [11, 11 + len), and only there
        ln = max(0, got.shape[-1] - 22 - x["shift"]) if 11 + x["shift"] > 0 else 0
        assert int(mask[i].sum()) == ln and mask[i, 11:11 + ln].all()
    assert _zeros_exactly_outside(got, mask) and (got[m] != 0).all()


@pytest.mark.parametrize("name", A.LAUNCHES)
def test_y_mode_against_the_model(name):
    (fig, got), (want, mask) = _run(name, "y"), _model(name, "y")
    models = A.build_launch(name)[2]
    assert [int(h) for h in fig["hyp"]] == [m["hyp"] for m in models]
    dev = L.rel_dev(got, want, mask)
    print(f"y-mode {name}: max |kernel - model| / max(1, |model|) {dev:.3e}, largest |lam| {np.abs(want).max():.1f} nats")
    assert np.isfinite(got).all()
    assert dev <= Y_LLR_TOL
    assert _zeros_exactly_outside(got, mask)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", A.LAUNCHES)
def test_every_hypothesis_is_a_plane_transform_of_the_first(name, mode):
    """hyp = h gives, bit for bit, the hyp = 0 output with planes exchanged and top-bit planes negated; hyp = 4 + h gives the bits of h."""
    xs = A.build_launch(name)[0]
    mask = _model(name, mode)[1]
    base = _llr(xs, mode, np.zeros(3, np.int64)).cpu().numpy()
    m = np.broadcast_to(mask[:, None, :], base.shape)
    for h in range(4):
        got = _llr(xs, mode, np.full(3, h, np.int64)).cpu().numpy()
        want = np.where(m, L.retransform(base, h, xs[0]["n"]), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, mode, h)
        got4 = _llr(xs, mode, np.full(3, 4 + h, np.int64)).cpu().numpy()
        assert np.array_equal(got4.view(np.uint32), got.view(np.uint32)), (name, mode, 4 + h)


def _gmi_tol(mode, n, llr, mask):
    b2 = 2 * L.nbits(n)
    if mode == "q":
        return b2 * (Q_LLR_TOL / LN2) + Q_TOL
    big = float(np.abs(llr[np.broadcast_to(mask[:, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return b2 * (Y_LLR_TOL * max(1.0, big) / LN2) + Y_INFO_TOL


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", A.LAUNCHES)
def test_sign_errors_and_gmi_are_awgn_infos(name, mode):
    from vae_equalizer_amd.engine import label_bits
    xs = A.build_launch(name)[0]
    fig, got = _run(name, mode)
    mask = _model(name, mode)[1]
    bits = label_bits(_dev(xs, "tx"), xs[0]["n"])
    assert bits.dtype == torch.int8 and bits.is_cuda and tuple(bits.shape) == got.shape
    bits = bits.cpu().numpy().astype(np.int64)
    assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], x["n"]) for x in xs]))
    gmi = np.array([L.gmi_from_llr(got[i], bits[i], mask[i], A.entropy(x["P"])) for i, x in enumerate(xs)])
    err = np.array([L.sign_errors(got[i], bits[i], mask[i]) for i in range(3)])
    tol = _gmi_tol(mode, xs[0]["n"], got, mask)
    kept = fig["kept"] > 0
    d = float(np.abs(gmi - fig["GMI"])[kept].max()) if kept.any() else 0.0
    print(f"{mode}-mode {name}: sign errors {err.tolist()} bit_err {fig['bit_err'].tolist()}; max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"])
    assert np.array_equal(err, fig["bit_err"])
    assert np.array_equal(np.isnan(gmi), ~kept) and d <= tol


def test_empty_windows_and_a_zero_row_give_all_zeros():
    """shift = -11 (an empty window), a y whose Q component is zero throughout (no normalisation: y-mode only), and a run that keeps its symbols
    between them, in one launch."""
    xs = [dict(x) for x in A.build_launch("N60-n8")[0]]
    xs[0]["shift"] = -11
    y = xs[2]["y"].copy()
    y[1] = 0
    xs[2]["y"] = y
    for mode in ("q", "y"):
        got = _llr(xs, mode, np.array([1, 2, 3])).cpu().numpy()
        want, mask = _model_of(xs, mode, [1, 2, 3])
        print(f"{mode}-mode: kept {mask.sum(-1).tolist()}")
        assert mask.sum(-1).tolist() == ([0, 38, 28] if mode == "q" else [0, 38, 0])
        assert _zeros_exactly_outside(got, mask) and not got[0].any()
        if mode == "q":
            assert np.abs(got - want).max() <= Q_LLR_TOL
        else:
            assert not got[2].any() and L.rel_dev(got, want, mask) <= Y_LLR_TOL


@pytest.mark.parametrize("name", ["N2100-n8", "N257-n4"])
def test_two_calls_and_single_run_calls_give_identical_bits(name):
    xs = A.build_launch(name)[0]
    hyp = np.array([3, 0, 2])
    for mode in ("q", "y"):
        a, b = _llr(xs, mode, hyp), _llr(xs, mode, hyp)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), mode
        for i in range(3):
            one = _llr(xs[i:i + 1], mode, hyp[i:i + 1])
            assert torch.equal(one.view(torch.int32), a[i:i + 1].view(torch.int32)), (mode, i)


def test_both_or_neither_source_is_refused():
    from vae_equalizer_amd.engine import awgn_llr
    xs = A.build_launch("N23-n2")[0]
    with pytest.raises(ValueError):
        _llr(xs, "q", np.zeros(3, np.int64), y=_dev(xs, "y"), amp_mean=_dev(xs, "amp_mean"), var=_dev(xs, "var"))
    with pytest.raises(ValueError):
        awgn_llr(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), hyp=torch.zeros(3).cuda())


def test_awgn_engine_llr_is_awgn_llr_with_the_engines_demapper():
    from vae_equalizer_amd.engine import AWGNEngine
    xs = A.build_launch("N1030-n8")[0]
    eng = AWGNEngine(3, 25, xs[0]["amp"], np.stack([v["P"] for v in xs]), [float(v["amp_mean"]) for v in xs], [float(v["var"]) for v in xs], "cuda:0", 2)
    hyp = np.array([1, 3, 2])
    a = eng.llr(_dev(xs, "y"), _dev(xs, "shift"), hyp)
    b = _llr(xs, "y", hyp)
    assert tuple(a.shape) == (3, 6, 1030) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("batch_norm", [False, True])
def test_nn_engine_llr_is_awgn_llr_on_the_eval_forwards_posteriors(batch_norm):
    from vae_equalizer_amd.engine import NNEngine, awgn_llr
    n, N = 8, 300
    eng = NNEngine(3, 25, 25, 3, A.amp_levels(n), "cuda:0", 2, batch_norm=batch_norm)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    eng.init_parameters(generator=g)
    x = torch.randn(3, 2, 2 * N, generator=g, device="cuda")
    shift, hyp = torch.tensor([-3, 0, 7]).cuda(), torch.tensor([2, 1, 3]).cuda()
    q = eng.forward(x)
    a = eng.llr(x, shift, hyp)
    b = awgn_llr(q=q, amp_levels=eng.amp, shift=shift, hyp=hyp)
    want, mask = _model_of([dict(q=q[i].cpu().numpy(), n=n, shift=int(shift[i])) for i in range(3)], "q", hyp.tolist())
    dev = float(np.abs(a.cpu().numpy() - want).max())
    print(f"NNEngine.llr (batch_norm {batch_norm}): max |kernel - model| {dev:.3e} nats, largest |lam| {np.abs(want).max():.2f}")
    assert tuple(a.shape) == (3, 6, N) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert dev <= Q_LLR_TOL and _zeros_exactly_outside(a.cpu().numpy(), mask)

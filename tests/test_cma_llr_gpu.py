"""vaeq_cma_epilogue_llr (the per-bit a-posteriori LLRs of a frame of the constant-modulus DP baselines) against the float64 model
tests/_ref_baseline_llr.py, through engine.cma_epilogue_llr, engine.label_bits and cma_runs.run_cma_batch(want_llr=True).

Launches are tests/_ref_cma_info.py's: R = 3 runs, N in {43, 47, 400, 1030}, n_lev in {2, 4, 8}, constellation-stage shifts (-10, 0) / (0, 10) /
(10, -10), soft-demapper-stage shifts (0, 0) / (2, -1) / (-3, 3), both r_c and r_q, every hypothesis, a window scale the mean-radius factor has to
undo inside W_c and must leave alone outside it.  tests/test_ref_baseline_llr_host.py pins the model to the information-rate model on the CPU.

Bounds.  |kernel - model| / max(1, |model|) <= 4 Y_LLR_DEV_CMA, Y_LLR_DEV_CMA the cost of float32 in the kernel's operation order computed on the
CPU; the factor (tests/test_epilogue_llr_gpu.py's) allows for the device's exp2 / log2 and for contraction to fused multiply-adds.  The GMI
recomputed from the kernel's LLRs is 1-Lipschitz in each of its 2 b terms per symbol, so it lies within 2 b (LLR bound in bit) plus the
information-rate kernel's own bound, 3 CMA_DEV, of that kernel's GMI.  test_every_entry_of_a_nan_filled_buffer_is_written hands the C entry point
a NaN-filled buffer of its own (engine.cma_epilogue_llr allocates its output itself).
Measured on the MI355X: 1.46e-6 relative at most with |lam| up to 399 nats, GMI from the LLRs within 2.8e-6 bit of the information-rate kernel's
(DESIGN.md section 5).  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_baseline_llr as B
import _ref_cma_info as C
import _ref_epilogue as E
import _ref_info as I
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
Y_LLR_TOL = 4 * B.Y_LLR_DEV_CMA    # relative to max(1, |lam|)
INFO_TOL = 3 * C.CMA_DEV           # bit: tests/test_cma_info_gpu.py's bound of the information-rate kernel's GMI
ALIGN = ("shift_c", "r_c", "shift_q", "r_q")


def _dev(xs, key, dtype=None):
    a = np.stack([np.asarray(x[key]) for x in xs])
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _llr(xs, hyp, **over):
    from vae_equalizer_amd.engine import cma_epilogue_llr
    kw = dict(y=_dev(xs, "y"), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"),
              **{k: _dev(xs, k) for k in ALIGN}, hyp=torch.as_tensor(np.asarray(hyp)).cuda())
    kw.update(over)
    return cma_epilogue_llr(**kw)


def _info(xs, **over):
    from vae_equalizer_amd.engine import cma_epilogue_info
    kw = dict(y=_dev(xs, "y"), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"),
              **{k: _dev(xs, k) for k in ALIGN})
    kw.update(over)
    return cma_epilogue_info(**kw)


def _model_of(xs, hyps):
    out = [B.cma_llr(x, h) for x, h in zip(xs, hyps)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (planes[R,2,2b,N] float64, mask[R,2,N]) under the information-rate model's hypotheses; computed once, never modified."""
    xs, ms = C.build_launch(name)
    return _model_of(xs, [m["hyp"] for m in ms])


@functools.lru_cache(maxsize=None)
def _run(name):
    """One information-rate launch and one LLR launch under its hypotheses per launch, shared by the tests."""
    xs = C.build_launch(name)[0]
    fig = {k: v.cpu().numpy() for k, v in _info(xs).items()}
    return fig, _llr(xs, fig["hyp"]).cpu().numpy()


def _erasures_are_plus_zero(got, mask):
    m = np.broadcast_to(mask[:, :, None, :], got.shape)
    return not got.view(np.uint32)[~m].any()


def _bits(a):
    return a.view(np.uint32) if isinstance(a, np.ndarray) else a.view(torch.int32)


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_against_the_model(name):
    (fig, got), (want, mask) = _run(name), _model(name)
    models = C.build_launch(name)[1]
    assert np.array_equal(fig["hyp"], np.stack([m["hyp"] for m in models]))
    dev = L.rel_dev(got, want, mask)
    print(f"{name}: max |kernel - model| / max(1, |model|) {dev:.3e} (bound {Y_LLR_TOL:.2e}), largest |lam| {np.abs(want).max():.1f} nats")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert not np.isnan(got).any() and np.isfinite(got).all()
    assert dev <= Y_LLR_TOL
    assert _erasures_are_plus_zero(got, mask)


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_every_entry_of_a_nan_filled_buffer_is_written(name):
    """The C entry point itself on a buffer of the test's own, NaN throughout: it leaves the bits engine.cma_epilogue_llr returns."""
    from vae_equalizer_amd import _native as nat
    xs = C.build_launch(name)[0]
    fig, want = _run(name)
    N, n = xs[0]["y"].shape[-1], xs[0]["n"]
    buf = torch.full((3, 2, 2 * L.nbits(n), N), float("nan"), dtype=torch.float32, device="cuda")
    t = dict(y=_dev(xs, "y"), tx=_dev(xs, "tx", torch.float16), amp=_dev(xs[:1], "amp", torch.float32)[0].contiguous(), var=_dev(xs, "var", torch.float32),
             nu_sc=_dev(xs, "nu_sc", torch.float32), hyp=torch.from_numpy(fig["hyp"]).cuda().to(torch.int32), **{k: _dev(xs, k, torch.int32) for k in ALIGN})
    i32 = torch.int32
    nat.check(nat.lib().vaeq_cma_epilogue_llr(3, N, n, nat.ptr(t["y"]), nat.ptr(t["tx"], torch.float16), nat.ptr(t["amp"]), nat.ptr(t["var"]),
                                              nat.ptr(t["nu_sc"]), nat.ptr(t["shift_c"], i32), nat.ptr(t["r_c"], i32), nat.ptr(t["shift_q"], i32),
                                              nat.ptr(t["r_q"], i32), nat.ptr(t["hyp"], i32), nat.ptr(buf), nat.current_stream(buf.device)),
              "vaeq_cma_epilogue_llr")
    got = buf.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_every_hypothesis_is_a_plane_transform_of_the_first(name):
    """hyp = h gives, bit for bit, the hyp = 0 output with planes exchanged and top-bit planes negated; hyp = 8 + h gives the bits of h."""
    xs = C.build_launch(name)[0]
    mask = _model(name)[1]
    m = np.broadcast_to(mask[:, :, None, :], (3, 2, 2 * L.nbits(xs[0]["n"]), mask.shape[-1]))
    base = _llr(xs, np.zeros((3, 2), np.int64)).cpu().numpy()
    for h in range(8):
        got = _llr(xs, np.full((3, 2), h, np.int64)).cpu().numpy()
        want = np.where(m, L.retransform(base, h, xs[0]["n"]), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (name, h)
        got8 = _llr(xs, np.full((3, 2), 8 + h, np.int64)).cpu().numpy()
        assert np.array_equal(_bits(got8), _bits(got)), (name, 8 + h)


def _gmi_and_sign_errors(llr, bits, mask, P):
    """Host float64, per (run, polarisation): GMI recomputed from LLRs and TX label bits, and the LLR signs that disagree with the bits."""
    R = llr.shape[0]
    gmi, err = np.full((R, 2), np.nan), np.zeros((R, 2), np.int64)
    for i in range(R):
        for p in range(2):
            gmi[i, p] = L.gmi_from_llr(llr[i, p], bits[i, p], mask[i, p], I.entropy(P[i]))
            err[i, p] = L.sign_errors(llr[i, p], bits[i, p], mask[i, p])
    return gmi, err


def _gmi_tol(n, llr, mask):
    """2 b (LLR bound in bit) + the information-rate kernel's own bound (the form of tests/test_epilogue_llr_gpu.py's _gmi_tol)."""
    big = float(np.abs(llr[np.broadcast_to(mask[:, :, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return 2 * L.nbits(n) * (Y_LLR_TOL * max(1.0, big) / LN2) + INFO_TOL


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_sign_errors_and_gmi_are_the_information_rate_kernels(name):
    from vae_equalizer_amd.engine import label_bits
    xs = C.build_launch(name)[0]
    fig, got = _run(name)
    mask = _model(name)[1]
    bits = label_bits(_dev(xs, "tx"), xs[0]["n"])
    assert bits.dtype == torch.int8 and bits.is_cuda and tuple(bits.shape) == got.shape
    bits = bits.cpu().numpy().astype(np.int64)
    assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], x["n"]) for x in xs]))
    gmi, err = _gmi_and_sign_errors(got, bits, mask, [x["P"] for x in xs])
    tol = _gmi_tol(xs[0]["n"], got, mask)
    d = float(np.abs(gmi - fig["GMI"]).max())
    print(f"{name}: sign errors {err.tolist()} bit_err {fig['bit_err'].tolist()}; max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"]) and (fig["kept"] > 0).all()
    assert np.array_equal(err, fig["bit_err"])
    assert d <= tol


def _twin(name, k):
    """Run k of the launch built again with scale_edges=True: same seed, same TX, the samples outside W_c divided by s too."""
    x = C.build_launch(name)[0][k]
    spec = C.launches()[name][k]
    kw = {a: b for a, b in spec.items() if a != "seed"}
    for sd in range(spec["seed"], spec["seed"] + 200):
        if np.array_equal(C.make_run(sd, **kw)["y"], x["y"]):
            return x, C.make_run(sd, **kw, scale_edges=True)
    raise AssertionError("the launch's seed is not among those build_run tries")


@pytest.mark.parametrize("name,k", [("N400-n8", 0), ("N1030-n4", 1), ("N47-n8", 2)])
def test_only_the_window_of_the_constellation_stage_is_scaled(name, k):
    """A twin whose samples outside W_c are divided by s as well: fac is the same float (W_c is the same), so the kept entries whose stage-c index
    lies in W_c keep their bits and the others -- which a kernel that scaled everything, or nothing, would get wrong -- follow the twin's own model."""
    x, tw = _twin(name, k)
    hyp = np.asarray(C.build_launch(name)[1][k]["hyp"])[None]
    assert np.array_equal(x["tx"], tw["tx"]) and not np.array_equal(x["y"], tw["y"])
    a, b = _llr([x], hyp).cpu().numpy(), _llr([tw], hyp).cpu().numpy()
    (want_a, mask), (want_b, mask_b) = _model_of([x], hyp), _model_of([tw], hyp)
    N = x["y"].shape[-1]
    W = C.window_c(N, x["shift_c"])
    outside = np.zeros((1, 2, N), bool)
    for p in range(2):
        m = np.arange(N) + int(x["shift_q"][p])
        outside[0, p] = mask[0, p] & ~((m >= W.start) & (m < W.stop))
    differ = (_bits(a) != _bits(b)).any(2)
    dev_own, dev_twin = L.rel_dev(b, want_b, mask_b), L.rel_dev(b, want_a, mask)
    print(f"{name} run {k}: {int(outside.sum())} kept entries outside W_c, {int(differ.sum())} differ; twin against its own model {dev_own:.3e}, "
          f"against the unscaled run's {dev_twin:.3e}")
    assert np.array_equal(mask, mask_b) and outside.sum() >= 10
    assert np.array_equal(differ, outside)
    assert dev_own <= Y_LLR_TOL and L.rel_dev(a, want_a, mask) <= Y_LLR_TOL
    assert dev_twin > 100 * Y_LLR_TOL


def test_zero_output_gives_all_zeros_and_disturbs_no_other_run():
    xs = C.build_launch("N400-n8")[0]
    hyp = np.array([[1, 6], [4, 3], [7, 2]], np.int64)
    base = _llr(xs, hyp)
    y = _dev(xs, "y").clone()
    y[1] = 0
    got = _llr(xs, hyp, y=y)
    assert not _bits(got[1]).any()                                            # +0.0 everywhere, no NaN left
    assert torch.equal(_bits(got[[0, 2]]), _bits(base[[0, 2]])) and base[1].abs().max() > 1


def test_shifts_are_clamped():
    """An alignment outside what the epilogue can return is clamped to +-10, as the information-rate kernel clamps its own: no index leaves the row."""
    xs = C.build_launch("N43-n4")[0]
    hyp = np.zeros((3, 2), np.int64)
    sc, sq = _dev(xs, "shift_c").clone(), _dev(xs, "shift_q").clone()
    sc[0, 0], sq[2, 1] = -10, 10
    want = _llr(xs, hyp, shift_c=sc, shift_q=sq)
    sc[0, 0], sq[2, 1] = -1000, 2 ** 31 - 1
    got = _llr(xs, hyp, shift_c=sc, shift_q=sq)
    assert torch.equal(_bits(got), _bits(want)) and torch.isfinite(got).all()
    fig = _info(xs, shift_c=sc, shift_q=sq)
    assert torch.equal((got != 0).any(2).sum(-1).cpu(), fig["kept"].cpu())     # (no kept symbol's 2 b LLRs are all exactly zero)


@pytest.mark.parametrize("name", ["N1030-n8", "N43-n2"])
def test_two_calls_and_single_run_calls_give_identical_bits(name):
    xs = C.build_launch(name)[0]
    hyp = np.array([[1, 6], [4, 3], [7, 2]], np.int64)
    a, b = _llr(xs, hyp), _llr(xs, hyp)
    assert torch.equal(_bits(a), _bits(b))
    for i in range(3):
        one = _llr(xs[i:i + 1], hyp[i:i + 1])
        assert torch.equal(_bits(one), _bits(a[i:i + 1])), i


@pytest.mark.parametrize("name", ["N43-n8", "N400-n4"])
def test_both_grids_give_the_bits_of_the_small_launch(name):
    """Up to 512 runs the two polarisations of a run go to two workgroups, beyond that to one: 512 and 513 runs, the launch's three repeated,
    give every run the bits it has in the launch of three."""
    xs = C.build_launch(name)[0]
    hyp = np.array([[1, 6], [4, 3], [7, 2]], np.int64)
    base = _llr(xs, hyp)
    for R in (512, 513):
        got = _llr([xs[i % 3] for i in range(R)], hyp[np.arange(R) % 3])
        assert tuple(got.shape) == (R,) + tuple(base.shape[1:])
        assert torch.equal(_bits(got), _bits(base[torch.arange(R, device="cuda") % 3])), R


def test_shapes_are_checked():
    from vae_equalizer_amd._native import VaeqError
    xs = C.build_launch("N43-n2")[0]
    hyp = np.zeros((3, 2), np.int64)
    with pytest.raises(ValueError):
        _llr(xs, hyp, data=_dev(xs, "tx")[..., :-1])
    with pytest.raises(VaeqError):
        _llr(xs, hyp, y=_dev(xs, "y")[..., :42].contiguous(), data=_dev(xs, "tx")[..., :42].contiguous())   # N < 43


# ------------------------------------------------------------------ run_cma_batch(want_llr=True)
RUN_KW = dict(mod="64-QAM", sps=2, M_est=25, batch_len=100, N_train_max=400, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24,
              tau_pmd=0.1e-12 * np.sqrt(1000), phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170, generator="hip")
NUS = (0.0, 0.0270955)


def _same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize("mode,lr", [("CMA", 1e-4), ("CMAflex", 1e-5)])       # step sizes at which two frames do not diverge
def test_run_cma_batch_returns_the_last_frames_llrs(mode, lr):
    from vae_equalizer_amd import cma_runs
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.dp_runs import DPRun
    runs = [DPRun(22 + 2 * i, NUS[i], 0.01, 0.3, lr, 90e9, seed=500 + i) for i in range(2)]
    a = cma_runs.run_cma_batch(runs, mode, want_info=True, want_llr=True, **RUN_KW)
    b = cma_runs.run_cma_batch(runs, mode, want_info=True, **RUN_KW)
    c = cma_runs.run_cma_batch(runs, mode, want_llr=True, **RUN_KW)
    d = cma_runs.run_cma_batch(runs, mode, **RUN_KW)
    assert set(a) - set(b) == {"llr"} and set(c) - set(d) == {"llr"} and "info" not in c and "llr" not in b
    for other in (b, c, d):
        assert _same_bits(a["SER"], other["SER"]) and torch.equal(a["Var_est"], other["Var_est"]) and torch.equal(a["var"], other["var"])
        assert torch.equal(a["h"], other["h"])
    for k in a["info"]:
        assert _same_bits(a["info"][k], b["info"][k]), k
    N = RUN_KW["N_train_max"] - 2 * cma_runs.N_CUT
    llr, bits, hyp = a["llr"]["llr"], a["llr"]["bits"], a["llr"]["hyp"]
    assert llr.is_cuda and llr.dtype == torch.float32 and tuple(llr.shape) == (2, 2, 6, N)
    assert bits.is_cuda and bits.dtype == torch.int8 and tuple(bits.shape) == (2, 2, 6, N) and tuple(hyp.shape) == (2, 2)
    assert torch.equal(hyp.cpu(), a["info"]["hyp"][:, :, -1])
    for k in ("llr", "bits", "hyp"):                                           # the hypothesis is the same call's whether want_info is on or not
        assert torch.equal(a["llr"][k], c["llr"][k]), k
    assert set(np.unique(bits.cpu().numpy())) <= {0, 1} and torch.isfinite(llr).all()
    # the kept window [11, N - 11 - max|shift_q|) is a prefix-free block: recover it from the erasures, and check it against the reported count
    llr_n, bits_n = llr.cpu().numpy(), bits.cpu().numpy().astype(np.int64)
    kept = a["info"]["kept"][:, :, -1].numpy()
    mask = np.zeros((2, 2, N), bool)
    for i in range(2):
        for p in range(2):
            mask[i, p, E.EDGE:E.EDGE + int(kept[i, p])] = True
    assert (kept > N - 2 * E.EDGE - 11).all()
    assert not _bits(llr_n)[~np.broadcast_to(mask[:, :, None, :], llr_n.shape)].any()
    assert (llr_n != 0).any(2)[mask].all()
    tabs = [sfun.qam_tables("64-QAM", nu) for nu in NUS]
    gmi, err = _gmi_and_sign_errors(llr_n, bits_n, mask, [t["P"] for t in tabs])
    want = a["info"]["GMI"][:, :, -1].numpy()
    tol = _gmi_tol(8, llr_n, mask)
    print(f"run_cma_batch[{mode}] last frame: GMI from the LLRs {gmi.tolist()} reported {want.tolist()} (bound {tol:.2e}); sign errors {err.tolist()} "
          f"bit_err {a['info']['bit_err'][:, :, -1].tolist()}")
    assert np.array_equal(err, a["info"]["bit_err"][:, :, -1].numpy())
    assert np.abs(gmi - want).max() <= tol


def test_run_cma_batch_bits_are_the_label_bits_of_the_cut_reference(monkeypatch):
    """bits == label_bits of the [10:-10]-cut TX reference the epilogue got, and llr is cma_epilogue_llr on that frame's y and alignment."""
    from vae_equalizer_amd import cma_runs, engine
    from vae_equalizer_amd.dp_runs import DPRun
    runs = [DPRun(22 + 2 * i, NUS[i], 0.01, 0.3, 1e-4, 90e9, seed=500 + i) for i in range(2)]
    seen = []
    inner = cma_runs.cma_frame_epilogue

    def spy(out_const, data, *a, **k):
        seen.append((data, k.get("want_llr", False)))
        return inner(out_const, data, *a, **k)
    monkeypatch.setattr(cma_runs, "cma_frame_epilogue", spy)
    r = cma_runs.run_cma_batch(runs, "CMAbatch", want_llr=True, **RUN_KW)
    assert [s[1] for s in seen] == [False, True]                               # the last frame only
    d = seen[-1][0][..., cma_runs.N_CUT:-cma_runs.N_CUT]
    assert torch.equal(r["llr"]["bits"], engine.label_bits(d, 8))

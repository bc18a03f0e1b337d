"""vaeq_awgn_track_llr (the per-bit a-posteriori LLRs of an AWGN baseline's soft sequence) against the float64 model tests/_ref_baseline_llr.py,
through engine.awgn_track_llr, engine.label_bits, DFE_MQAM_shaping.run_dfe_batch(want_llr=True) and awgn_cma_validate's CPE output.

Launches are tests/_ref_awgn_baseline_info.py's: R = 3 runs with shifts -10 / 0 / +10, Nd - 2 e in {1, 2, 11, 38, 247, 1008} (11 / 1 / 0 kept
symbols up to one symbol in the second round of the 256-thread workgroup), e in {11, 31}, Nz - Nd in {0, 1}, both layouts, n_lev in {2, 4, 8},
every hypothesis, and "wide" (shifts -12 / +11 that nobody clamps).  tests/test_ref_baseline_llr_host.py pins the model to the information-rate
model on the CPU.

Bounds.  |kernel - model| / max(1, |model|) <= 4 Y_LLR_DEV_TRACK (the cost of float32 in the kernel's operation order, computed on the CPU; the
factor is tests/test_epilogue_llr_gpu.py's).  The GMI recomputed from the kernel's LLRs lies within 2 b (LLR bound in bit) + 3 Z_DEV, the
information-rate kernel's own bound, of that kernel's GMI.  Measured on the MI355X: 5.34e-6 relative at most with |lam| up to 627 nats, GMI from
the LLRs within 8.1e-6 bit of the information-rate kernel's.  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_awgn_baseline_info as T
import _ref_awgn_info as A
import _ref_baseline_llr as B
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
Y_LLR_TOL = 4 * B.Y_LLR_DEV_TRACK  # relative to max(1, |lam|)
INFO_TOL = 3 * T.Z_DEV             # bit: tests/test_awgn_baseline_info_gpu.py's bound of the information-rate kernel's GMI


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _dev(xs, key, dtype=None):
    return _t(np.stack([np.asarray(x[key]) for x in xs]), dtype)


def _z(xs):
    """The runs' tracks in the launch's layout: complex [R,Nz] (interleaved) or float [R,2,Nz] (planar)."""
    z = _dev(xs, "z")
    return z if xs[0]["interleaved"] else torch.stack([z.real, z.imag], 1).contiguous()


def _groups(name):
    """The launch as calls of one Nz each ("wide" mixes Nz = Nd + 1 and Nz = Nd) -> [(xs, models)]."""
    xs, ms = T.build_launch(name)
    if name == "wide":
        return [(xs[:1], ms[:1]), (xs[1:], ms[1:])]
    return [(xs, ms)]


def _llr(xs, hyp, **over):
    from vae_equalizer_amd.engine import awgn_track_llr
    kw = dict(z=_z(xs), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], var=_dev(xs, "var"), shift=_dev(xs, "shift"),
              hyp=torch.as_tensor(np.asarray(hyp)).cuda(), edge=xs[0]["edge"])
    kw.update(over)
    return awgn_track_llr(**kw)


def _info(xs, **over):
    from vae_equalizer_amd.engine import awgn_track_info
    kw = dict(z=_z(xs), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), var=_dev(xs, "var"), shift=_dev(xs, "shift"), edge=xs[0]["edge"])
    kw.update(over)
    return awgn_track_info(**kw)


def _model_of(xs, hyps):
    out = [B.track_llr(x, h) for x, h in zip(xs, hyps)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def _run(name):
    """Per call of the launch: (figures of one information-rate launch, the LLRs of one launch under its hypotheses, model planes, mask, xs, models);
    computed once, shared by the tests, never modified."""
    out = []
    for xs, ms in _groups(name):
        fig = {k: v.cpu().numpy() for k, v in _info(xs).items()}
        want, mask = _model_of(xs, [m["hyp"] for m in ms])
        out.append((fig, _llr(xs, fig["hyp"]).cpu().numpy(), want, mask, xs, ms))
    return out


def _bits(a):
    return a.view(np.uint32) if isinstance(a, np.ndarray) else a.view(torch.int32)


def _erasures_are_plus_zero(got, mask):
    return not _bits(got)[~np.broadcast_to(mask[:, None, :], got.shape)].any()


ALL = T.LAUNCHES + ["wide"]


@pytest.mark.parametrize("name", ALL)
def test_against_the_model(name):
    for fig, got, want, mask, xs, ms in _run(name):
        assert np.array_equal(fig["hyp"], [m["hyp"] for m in ms])
        dev = L.rel_dev(got, want, mask)
        print(f"{name}: kept {mask.sum(-1).tolist()}, max |kernel - model| / max(1, |model|) {dev:.3e} (bound {Y_LLR_TOL:.2e}), largest |lam| "
              f"{np.abs(want).max():.1f} nats")
        assert got.dtype == np.float32 and got.shape == want.shape == (len(xs), 2 * L.nbits(xs[0]["n"]), xs[0]["tx"].shape[-1])
        assert np.isfinite(got).all()
        assert dev <= Y_LLR_TOL
        assert _erasures_are_plus_zero(got, mask)


@pytest.mark.parametrize("name", ALL)
def test_every_entry_of_a_nan_filled_buffer_is_written(name):
    """The C entry point itself on a buffer of the test's own, NaN throughout: it leaves the bits engine.awgn_track_llr returns."""
    from vae_equalizer_amd import _native as nat
    i32 = torch.int32
    for fig, want, _, _, xs, _ in _run(name):
        R, n, Nd, Nz = len(xs), xs[0]["n"], xs[0]["tx"].shape[-1], len(xs[0]["z"])
        il = xs[0]["interleaved"]
        z = _z(xs)
        z = (torch.view_as_real(z) if il else z).contiguous()
        buf = torch.full((R, 2 * L.nbits(n), Nd), float("nan"), dtype=torch.float32, device="cuda")
        tx, amp, var = _dev(xs, "tx", torch.float16), _t(np.asarray(xs[0]["amp"]), torch.float32), _dev(xs, "var", torch.float32)
        shift, hyp = _dev(xs, "shift", i32), _t(fig["hyp"], i32)
        nat.check(nat.lib().vaeq_awgn_track_llr(R, Nz, Nd, n, xs[0]["edge"], int(il), nat.ptr(z), nat.ptr(tx, torch.float16), nat.ptr(amp), nat.ptr(var),
                                                nat.ptr(shift, i32), nat.ptr(hyp, i32), nat.ptr(buf), nat.current_stream(buf.device)),
                  "vaeq_awgn_track_llr")
        got = buf.cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ALL)
def test_every_hypothesis_is_a_plane_transform_of_the_first(name):
    """hyp = h gives, bit for bit, the hyp = 0 output with planes exchanged and top-bit planes negated; hyp = 4 + h gives the bits of h."""
    for _, _, want, mask, xs, _ in _run(name):
        m = np.broadcast_to(mask[:, None, :], want.shape)
        base = _llr(xs, np.zeros(len(xs), np.int64)).cpu().numpy()
        for h in range(4):
            got = _llr(xs, np.full(len(xs), h, np.int64)).cpu().numpy()
            exp = np.where(m, L.retransform(base, h, xs[0]["n"]), np.float32(0.0)).astype(np.float32)
            assert np.array_equal(_bits(got), _bits(exp)), (name, h)
            got4 = _llr(xs, np.full(len(xs), 4 + h, np.int64)).cpu().numpy()
            assert np.array_equal(_bits(got4), _bits(got)), (name, 4 + h)


def _gmi_and_sign_errors(llr, bits, mask, P):
    R = llr.shape[0]
    gmi, err = np.full(R, np.nan), np.zeros(R, np.int64)
    for i in range(R):
        gmi[i] = L.gmi_from_llr(llr[i], bits[i], mask[i], A.entropy(P[i]))
        err[i] = L.sign_errors(llr[i], bits[i], mask[i])
    return gmi, err


def _gmi_tol(n, llr, mask):
    """2 b (LLR bound in bit) + the information-rate kernel's own bound (the form of tests/test_epilogue_llr_gpu.py's _gmi_tol)."""
    big = float(np.abs(llr[np.broadcast_to(mask[:, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return 2 * L.nbits(n) * (Y_LLR_TOL * max(1.0, big) / LN2) + INFO_TOL


def _consistent(tag, llr, bits, mask, P, n, fig):
    """Mask count == kept, sign errors == bit_err, GMI from the LLRs within the bound of the information-rate kernel's."""
    gmi, err = _gmi_and_sign_errors(llr, bits, mask, P)
    tol = _gmi_tol(n, llr, mask)
    kept = np.asarray(fig["kept"]) > 0
    d = float(np.abs(gmi - np.asarray(fig["GMI"], np.float64))[kept].max()) if kept.any() else 0.0
    print(f"{tag}: kept {np.asarray(fig['kept']).tolist()} sign errors {err.tolist()} bit_err {np.asarray(fig['bit_err']).tolist()}; "
          f"max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"])
    assert np.array_equal(err, fig["bit_err"])
    assert np.array_equal(np.isnan(gmi), ~kept) and d <= tol


@pytest.mark.parametrize("name", ALL)
def test_sign_errors_and_gmi_are_the_information_rate_kernels(name):
    from vae_equalizer_amd.engine import label_bits
    for fig, got, _, mask, xs, _ in _run(name):
        bits = label_bits(_dev(xs, "tx"), xs[0]["n"])
        assert bits.dtype == torch.int8 and bits.is_cuda and tuple(bits.shape) == got.shape
        bits = bits.cpu().numpy().astype(np.int64)
        assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], x["n"]) for x in xs]))
        _consistent(name, got, bits, mask, [x["P"] for x in xs], xs[0]["n"], fig)


def test_an_empty_window_and_a_zero_slice_give_all_zeros():
    """D = 1 at shift +10 keeps nothing (the launch grid's own third run); shift = -e is the reference's empty -0 slice; a run whose slice is zero
    throughout has no normalisation.  The run between them keeps its symbols."""
    for name in ("D1-e11-dz0-il0-n8", "D1-e31-dz1-il1-n4"):
        fig, got, _, mask, xs, ms = _run(name)[0]
        assert [m["kept"] for m in ms] == [11, 1, 0] and not _bits(got[2]).any() and _bits(got[1]).any()
    for name in ("D38-e11-dz0-il0-n8", "D38-e31-dz1-il1-n4"):
        xs = [dict(x) for x in T.build_launch(name)[0]]
        base = _llr(xs, [1, 2, 3])
        xs[0]["shift"] = -xs[0]["edge"]
        z = np.array(xs[2]["z"])
        ri = T.window(len(z), xs[2]["tx"].shape[-1], xs[2]["edge"], xs[2]["shift"])[0]
        z[ri] = 0                                                              # the slice only: what lies outside it is not looked at
        xs[2]["z"] = z
        got = _llr(xs, [1, 2, 3])
        assert not _bits(got[0]).any() and not _bits(got[2]).any(), name
        assert torch.equal(_bits(got[1]), _bits(base[1])) and base[0].abs().max() > 1 and base[2].abs().max() > 1


@pytest.mark.parametrize("name", ["D1008-e31-dz1-il1-n8", "D247-e11-dz0-il0-n4"])
def test_two_calls_and_single_run_calls_give_identical_bits(name):
    xs = T.build_launch(name)[0]
    hyp = np.array([1, 2, 3], np.int64)
    a, b = _llr(xs, hyp), _llr(xs, hyp)
    assert torch.equal(_bits(a), _bits(b))
    for i in range(3):
        assert torch.equal(_bits(_llr(xs[i:i + 1], hyp[i:i + 1])), _bits(a[i:i + 1])), i


def test_layout_follows_from_the_dtype_and_shapes_are_checked():
    from vae_equalizer_amd._native import VaeqError
    xs = T.build_launch("D38-e11-dz0-il0-n4")[0]
    z = _dev(xs, "z")
    hyp = np.array([3, 0, 1], np.int64)
    a, b = _llr(xs, hyp, z=z), _llr(xs, hyp, z=torch.stack([z.real, z.imag], 1).contiguous())
    assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError):
        _llr(xs, hyp, z=torch.stack([z.real, z.imag], 2).contiguous())        # a float [R,Nz,2] is neither layout
    with pytest.raises(VaeqError):
        _llr(xs, hyp, z=z[:, :-1].contiguous())                               # Nz = Nd - 1


# ------------------------------------------------------------------ the host layers
def _window_mask(R, Nd, edge, shift):
    mask = np.zeros((R, Nd), bool)
    for r in range(R):
        mask[r, T.window(Nd, Nd, edge, int(shift[r]))[1]] = True
    return mask


def test_run_dfe_batch_returns_the_llrs_of_both_curves():
    from vae_equalizer_amd import DFE_MQAM_shaping as D
    from vae_equalizer_amd import channel as ch
    args = ([16, 20], 2, 1100, "16-QAM")
    kw = dict(nu=0.0872449, seed=5)
    r0 = D.run_dfe_batch(*args, **kw, want_info=True)
    r = D.run_dfe_batch(*args, **kw, want_info=True, want_llr=True)
    r1 = D.run_dfe_batch(*args, **kw, want_llr=True)
    r2 = D.run_dfe_batch(*args, **kw)
    assert set(r) == set(r0) | {"llr_mmse", "llr_dfe"} and set(r1) == set(r2) | {"llr_mmse", "llr_dfe"}
    for k in r0:                                                               # every pre-existing key, bit for bit
        for other in (r, r1, r2):
            if k not in other:
                assert k.startswith("info_") and other is not r
            elif k.startswith("info_"):
                for kk in r0[k]:
                    assert torch.equal(torch.nan_to_num(r0[k][kk], nan=-1.0), torch.nan_to_num(other[k][kk], nan=-1.0)), (k, kk)
            elif isinstance(r0[k], torch.Tensor):
                assert torch.equal(r0[k], other[k]), k
            else:
                assert np.array_equal(np.asarray(r0[k]), np.asarray(other[k])), k
    amps = D.qam_constants("16-QAM")["amp_levels"].numpy()
    P = ch.pcs_probabilities(amps, 0.0872449)
    for tag in ("mmse", "dfe"):
        out, fig = r["llr_" + tag], {k: v.reshape(4).numpy() for k, v in r["info_" + tag].items()}
        llr, bits, hyp = out["llr"], out["bits"], out["hyp"]
        assert llr.is_cuda and llr.dtype == torch.float32 and tuple(llr.shape) == (2, 2, 4, 1100)
        assert bits.is_cuda and bits.dtype == torch.int8 and tuple(bits.shape) == (2, 2, 4, 1100) and tuple(hyp.shape) == (2, 2)
        assert torch.equal(hyp.cpu(), r["info_" + tag]["hyp"])
        for k in ("llr", "bits", "hyp"):                                       # the hypothesis is the same call's whether want_info is on or not
            assert torch.equal(out[k], r1["llr_" + tag][k]), k
        mask = _window_mask(4, 1100, D.N_cut + 11, r["shift_" + tag].reshape(4))
        llr_n, bits_n = llr.reshape(4, 4, 1100).cpu().numpy(), bits.reshape(4, 4, 1100).cpu().numpy().astype(np.int64)
        assert _erasures_are_plus_zero(llr_n, mask) and np.isfinite(llr_n).all()
        _consistent(f"run_dfe_batch {tag}", llr_n, bits_n, mask, [P] * 4, 4, fig)


def test_cpe_output_of_the_constant_modulus_validation():
    """engine.awgn_track_llr on awgn_cma_validate(..., want_cpe=True)'s planar output is consistent with engine.awgn_track_info on it."""
    from vae_equalizer_amd.engine import awgn_cma_validate, awgn_track_info, awgn_track_llr, label_bits
    b, frames = T.CMA_BATCHES[0], T.cma_batch(0)
    rx, h, data = (_t(np.stack([f[k] for f in frames])) for k in ("rx", "h", "data"))
    lev = frames[0]["levels"]
    ser, shift, y = awgn_cma_validate(rx, h, data, lev, b["sps"], b["n_shift"], want_cpe=True)
    P = np.full(b["n_lev"], 1.0 / b["n_lev"], np.float32)
    fig = {k: v.cpu().numpy() for k, v in awgn_track_info(y, data, lev, P, 0.01, shift, 11).items()}
    llr = awgn_track_llr(y, data, lev, 0.01, shift, fig["hyp"], 11)
    assert tuple(llr.shape) == (3, 2 * L.nbits(b["n_lev"]), b["K"]) and llr.is_cuda
    mask = _window_mask(3, b["K"], 11, shift.cpu().numpy())
    llr_n = llr.cpu().numpy()
    yh = y.cpu().numpy()
    want = np.stack([B.track_llr(dict(z=(yh[r, 0] + 1j * yh[r, 1]).astype(np.complex64), tx=f["data"], amp=np.asarray(lev), var=np.float32(0.01),
                                      shift=int(shift[r]), edge=11, n=b["n_lev"]), fig["hyp"][r])[0] for r, f in enumerate(frames)])
    dev = L.rel_dev(llr_n, want, mask)
    print(f"CPE output K{b['K']}: shift {shift.tolist()} hyp {fig['hyp'].tolist()} max |kernel - model| / max(1, |model|) {dev:.3e}")
    assert dev <= Y_LLR_TOL and _erasures_are_plus_zero(llr_n, mask)
    _consistent("CPE output", llr_n, label_bits(data, b["n_lev"]).cpu().numpy().astype(np.int64), mask, [P] * 3, b["n_lev"], fig)
    assert fig["sym_err"].tolist() == [r["n_err"] for r in b["runs"]]

"""vaeq_awgn_info / _llr and vaeq_awgn_track_info / _llr over their envelope (tests/_info_envelope_cases.py) against the float64 models
tests/_ref_awgn_info.py, _ref_llr.py, _ref_awgn_baseline_info.py and _ref_baseline_llr.py, through the engine.py wrappers (the C ABI only where the
output buffer is filled with NaN first).  tests/test_ref_info_envelope_host.py asserts every case's preconditions on the CPU.

What the feature tests leave out: rows shorter than 23 symbols (N >= 1 is legal) and the ones that keep 0, 1, 2 and 10 symbols, every shift in
-10 .. 12 around the 256-thread round, a fixed-order sum over 78 terms per thread, shifts no int32 arithmetic survives (TrackWindow computes in 64
bits), ties of posteriors and of hypotheses, TX samples off the grid, subnormal posteriors, pmfs with zero entries, hypotheses outside 0 .. 3;
for the track pair edge in {0, 1}, edge near Nd / 2, both layouts and both Nz - Nd at each, and the int32 extremes of shift and edge.

Bounds: as in tests/test_info_envelope_gpu.py.  Counts equal the model's; erasures are +0.0 through the uint32 view; q-mode holds the project's
Q_TOL = 1e-4 bit and Q_LLR_TOL = 2 Q_TOL ln 2 nats (a case with a 126-bit term: Q_TOL per float32 log2 term of a symbol); y-mode holds, per run,
the larger of the pair's existing bound and FACTOR = 4 times the deviation of that run's float32 restatement from the float64 model.  Every test
prints its figures before it asserts; the last test prints the largest error of each pair and mode with its bound.
"""
import functools

import numpy as np
import pytest
import torch

import _info_envelope_cases as K
import _ref_awgn_baseline_info as T
import _ref_awgn_info as A
import _ref_baseline_llr as B
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
FACTOR = 4
Q_TOL = 1e-4
Q_LLR_TOL = 2 * Q_TOL * LN2
Y_TOL = {"awgn": 3 * A.Y_DEV, "track": 3 * T.Z_DEV}
Y_LLR_TOL = {"awgn": 4 * L.Y_LLR_DEV_AWGN, "track": 4 * B.Y_LLR_DEV_TRACK}
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")
WORST = {}
i32 = torch.int32


def _record(key, err, bound, where):
    if key not in WORST or err / bound > WORST[key][0] / WORST[key][1]:
        WORST[key] = (err, bound, where)


def _dev(xs, key, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x[key]) for x in xs]))).cuda()
    return t if dtype is None else t.to(dtype)


def _hyp(h):
    return h.cuda() if torch.is_tensor(h) else torch.as_tensor(np.asarray(h)).cuda()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b):
    """Two info dicts, or two LLR tensors, with the same bits (NaN figures equal NaN figures)."""
    if isinstance(a, dict):
        return all(torch.equal(torch.nan_to_num(a[k].float(), nan=-7.0), torch.nan_to_num(b[k].float(), nan=-7.0)) for k in FIG + CNT)
    return a.shape == b.shape and torch.equal(a.contiguous().view(i32), b.contiguous().view(i32))


def _erasures_are_plus_zero(got, mask):
    return not got.view(np.uint32)[~np.broadcast_to(mask[..., None, :], got.shape)].any()


def _check_counts(got, models, tag):
    print(f"{tag}: " + ", ".join(f"{k} {got[k].tolist()}" for k in CNT))
    for i, m in enumerate(models):
        for k in CNT:
            assert int(got[k][i]) == m[k], (tag, i, k, got[k][i], m[k])
        if m["kept"] == 0:
            for k in FIG:
                assert np.isnan(got[k][i]), (tag, i, k)


def _check_figures(pair, mode, tag, got, models, bounds):
    for i, m in enumerate(models):
        if m["kept"] == 0:
            continue
        d = {k: abs(float(got[k][i]) - m[k]) for k in FIG}
        ba, bg = bounds[i]
        print(f"{mode}-mode {tag} run {i} (kept {m['kept']}): " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()) + f"; bounds {ba:.2e} {bg:.2e}")
        _record((pair, mode, "AIR"), d["AIR"], ba, f"{tag} run {i}")
        _record((pair, mode, "GMI"), d["GMI"], bg, f"{tag} run {i}")
        assert d["AIR"] <= ba and d["GMI"] <= bg and d["NGMI"] <= bg and d["BER"] <= 1e-7, (tag, i, d)


def _check_llrs(pair, mode, tag, got, want, mask, bounds):
    """q-mode: |kernel - model| in nats; y-mode: relative to max(1, |model|); bounds[i] of run i."""
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and _erasures_are_plus_zero(got, mask)
    for i in range(len(got)):
        if mode == "q":
            m = np.broadcast_to(mask[i][None, :], want[i].shape)
            dev = float(np.abs(got[i].astype(np.float64) - want[i])[m].max()) if m.any() else 0.0
        else:
            dev = L.rel_dev(got[i], want[i], mask[i])
        print(f"{mode}-mode {tag} run {i}: LLR deviation {dev:.3e} (bound {bounds[i]:.3e}), largest |lam| {np.abs(want[i]).max():.1f} nats")
        _record((pair, mode, "LLR"), dev, bounds[i], f"{tag} run {i}")
        assert dev <= bounds[i], (tag, i)


def _gmi_tol(pair, mode, n, llr, mask):
    """2 b (LLR bound in bit) + the information-rate kernel's own bound: tests/test_awgn_llr_gpu.py's and tests/test_awgn_track_llr_gpu.py's."""
    b2 = 2 * L.nbits(n)
    if mode == "q":
        return b2 * (Q_LLR_TOL / LN2) + Q_TOL
    big = float(np.abs(llr[np.broadcast_to(mask[:, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return b2 * (Y_LLR_TOL[pair] * max(1.0, big) / LN2) + Y_TOL[pair]


def _check_consistency(pair, mode, tag, xs, fig, got, mask):
    from vae_equalizer_amd.engine import label_bits
    n = xs[0]["n"]
    bits = label_bits(_dev(xs, "tx"), n).cpu().numpy().astype(np.int64)
    assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], n) for x in xs]))
    gmi = np.array([L.gmi_from_llr(got[i], bits[i], mask[i], A.entropy(x["P"])) for i, x in enumerate(xs)])
    err = np.array([L.sign_errors(got[i], bits[i], mask[i]) for i in range(len(xs))])
    tol = _gmi_tol(pair, mode, n, got, mask)
    kept = fig["kept"] > 0
    d = float(np.abs(gmi - fig["GMI"])[kept].max()) if kept.any() else 0.0
    print(f"{mode}-mode {tag}: sign errors {err.tolist()} bit_err {fig['bit_err'].tolist()}; max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"]) and np.array_equal(err, fig["bit_err"])
    assert np.array_equal(np.isnan(gmi), ~kept) and d <= tol


# ------------------------------------------------------------------ the AWGN pair
def _src(xs, mode):
    if mode == "q":
        return dict(q=_dev(xs, "q"))
    return dict(y=_dev(xs, "y"), amp_mean=_dev(xs, "amp_mean"), var=_dev(xs, "var"))


def _info(xs, mode, **over):
    from vae_equalizer_amd.engine import awgn_info
    kw = dict(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), **_src(xs, mode))
    kw.update(over)
    return awgn_info(**kw)


def _llr(xs, mode, hyp, **over):
    from vae_equalizer_amd.engine import awgn_llr
    kw = dict(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), hyp=_hyp(hyp), **_src(xs, mode))
    kw.update(over)
    return awgn_llr(**kw)


def _llr_into_nan(xs, mode, hyp):
    """vaeq_awgn_llr through the C ABI into a buffer filled with NaN."""
    from vae_equalizer_amd import _native as nat
    n, R = xs[0]["n"], len(xs)
    src = _src(xs, mode)
    q, y, am, var = (src.get(k) for k in ("q", "y", "amp_mean", "var"))
    N = (q if y is None else y).shape[-1]
    buf = torch.full((R, 2 * L.nbits(n), N), float("nan"), dtype=torch.float32, device="cuda")
    f = lambda t: None if t is None else t.float().contiguous()
    q, y, am, var = f(q), f(y), f(am), f(var)
    amp = torch.as_tensor(np.asarray(xs[0]["amp"]), dtype=torch.float32).cuda()
    shift, hyp = _dev(xs, "shift", i32), _hyp(hyp).to(i32).contiguous()
    nat.check(nat.lib().vaeq_awgn_llr(R, N, n, nat.ptr(q), nat.ptr(y), nat.ptr(amp), nat.ptr(am), nat.ptr(var), nat.ptr(shift, i32), nat.ptr(hyp, i32),
                                      nat.ptr(buf), nat.current_stream(buf.device)), "vaeq_awgn_llr")
    return buf


def _awgn_planes(x, hyp, mode, f32=False):
    if mode == "q":
        return L.awgn_llr_q(x["q"], x["n"], x["shift"], hyp)
    return (L.awgn_llr_y32 if f32 else L.awgn_llr_y)(x["y"], x["n"], x["amp"], x["amp_mean"], x["var"], x["shift"], hyp)


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    xs = K.awgn(name)[0]
    fig = _np(_info(xs, mode))
    return fig, _llr(xs, mode, fig["hyp"]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    xs, mq, my = K.awgn(name)
    out = [_awgn_planes(x, m["hyp"], mode) for x, m in zip(xs, mq if mode == "q" else my)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_counts_equal_the_model(name, mode):
    _check_counts(_run(name, mode)[0], K.awgn(name)[1 if mode == "q" else 2], f"{mode}-mode {name}")


@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_q_mode_figures_and_llrs(name):
    (fig, got), (want, mask) = _run(name, "q"), _model(name, "q")
    xs, models, _ = K.awgn(name)
    _check_figures("awgn", "q", name, fig, models, [(Q_TOL, Q_TOL)] * len(xs))
    _check_llrs("awgn", "q", name, got, want, mask, [Q_LLR_TOL] * len(xs))


@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_y_mode_figures_and_llrs(name):
    (fig, got), (want, mask) = _run(name, "y"), _model(name, "y")
    xs, _, models = K.awgn(name)
    fb = [max(Y_TOL["awgn"], FACTOR * (A.y_mode_float32_deviation(x, m) or 0.0)) for x, m in zip(xs, models)]
    _check_figures("awgn", "y", name, fig, models, [(b, b) for b in fb])
    lb = [max(Y_LLR_TOL["awgn"], FACTOR * L.rel_dev(_awgn_planes(x, m["hyp"], "y", True)[0], want[i], mask[i])) for i, (x, m) in enumerate(zip(xs, models))]
    _check_llrs("awgn", "y", name, got, want, mask, lb)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_llr_writes_every_entry_of_a_nan_filled_buffer(name, mode):
    xs = K.awgn(name)[0]
    fig, want = _run(name, mode)
    got = _llr_into_nan(xs, mode, fig["hyp"]).cpu().numpy()
    print(f"{mode}-mode {name}: {int(np.isnan(got).sum())} NaN left of {got.size}")
    assert not np.isnan(got).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _erasures_are_plus_zero(got, _model(name, mode)[1])


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.AWGN))
def test_awgn_sign_errors_and_gmi_of_the_llrs_are_awgn_infos(name, mode):
    fig, got = _run(name, mode)
    _check_consistency("awgn", mode, name, K.awgn(name)[0], fig, got, _model(name, mode)[1])


def test_awgn_runs_in_one_call_give_the_bits_of_single_calls():
    xs = K.awgn("N257")[0]
    hyp = np.arange(len(xs)) % 4
    for mode in ("q", "y"):
        a, la = _info(xs, mode), _llr(xs, mode, hyp)
        for i in range(len(xs)):
            one, lone = _info(xs[i:i + 1], mode), _llr(xs[i:i + 1], mode, hyp[i:i + 1])
            assert _same({k: v[i:i + 1] for k, v in a.items()}, one) and _same(la[i:i + 1], lone), (mode, i)


@pytest.mark.parametrize("mode", ["q", "y"])
def test_awgn_llr_hypotheses_outside_0_to_3_count_by_their_low_bits(mode):
    xs = K.awgn("N256")[0]
    hyp = np.array([0, 3, 1, 2, 2, 1], np.int64)
    want = _llr(xs, mode, hyp)
    for other in (hyp + 4, hyp + 8, hyp - 8, hyp - 2 ** 31):
        assert _same(want, _llr(xs, mode, other)), other.tolist()
    assert _same(_llr(xs, mode, np.full(6, 3)), _llr(xs, mode, np.full(6, -1)))
    assert not _same(want, _llr(xs, mode, np.full(6, 3)))


def _planted_tols(name, n):
    big = name.startswith("subnormal")                                          # a 126-bit term: Q_TOL per float32 log2 term of a symbol
    return (2 * Q_TOL, 2 * L.nbits(n) * Q_TOL) if big else (Q_TOL, Q_TOL)


@pytest.mark.parametrize("name", list(K.PLANTED_AWGN) + list(K.AWGN_TIES))
def test_awgn_planted_q_mode_edges(name):
    """Ties of posteriors (the first maximum) and of hypotheses (the smallest), TX samples off the grid, subnormal posteriors (126 bit, finite LLRs),
    pmfs with zero entries: counts and hypothesis are the model's, figures and LLRs within the q-mode bounds.  The sign errors of the LLRs are
    compared where no posterior ties: an LLR of exactly zero has no sign."""
    x, m = K.planted_awgn(name)
    n = x["n"]
    fig = _np(_info([x], "q"))
    got = _llr([x], "q", fig["hyp"]).cpu().numpy()
    _check_counts(fig, [m], name)
    _check_figures("awgn", "q", name, fig, [m], [_planted_tols(name, n)])
    want, mask = L.awgn_llr_q(x["q"], n, x["shift"], m["hyp"])
    print(f"{name}: cnt {m['cnt'].tolist()}")
    _check_llrs("awgn", "q", name, got, want[None], mask[None], [Q_LLR_TOL])
    if name.startswith("subnormal"):
        assert np.abs(want).max() > 120 * LN2 and fig["AIR"][0] < -126.0 * 2 / 38
    if not name.startswith("posterior-tie"):
        assert L.sign_errors(got[0], L.label_bits(x["tx"], n), mask) == int(fig["bit_err"][0])


@pytest.mark.parametrize("n", [2, 4, 8])
def test_awgn_y_mode_far_from_the_grid(n):
    """|yhat| = 50 and var = 1e-6 on eight kept symbols per component: exponents of 1e9 bit stay finite, the decisions are the outer level's."""
    x, m = K.far_awgn(n)
    fig = _np(_info([x], "y"))
    got = _llr([x], "y", fig["hyp"]).cpu().numpy()
    _check_counts(fig, [m], f"far n_lev {n}")
    # exponents of 1e9 .. 1e10 bit are spaced 128 .. 1024 bit apart in float32: the figures are held to what the format can hold of each symbol's term
    b = max(Y_TOL["awgn"], FACTOR * (A.y_mode_float32_deviation(x, m) or 0.0))
    _check_figures("awgn far", "y", f"far-n{n}", fig, [m], [tuple(max(b, f) for f in m["format_bounds"])])
    want, mask = L.awgn_llr_y(x["y"], n, x["amp"], x["amp_mean"], x["var"], 0, m["hyp"])
    print(f"far n_lev {n}: largest |LLR| {np.abs(got).max():.3e} nats (model {np.abs(want).max():.3e})")
    assert np.isfinite(got).all() and all(np.isfinite(fig[k]).all() for k in FIG) and fig["sym_err"].tolist() == [0]
    assert L.sign_errors(got[0], L.label_bits(x["tx"], n), mask) == 0 and np.abs(got).max() > 1e6 and _erasures_are_plus_zero(got, mask[None])


# ------------------------------------------------------------------ the track pair
def _z(xs):
    """The runs' tracks in the launch's layout: complex [R,Nz] (interleaved) or float [R,2,Nz] (planar)."""
    z = _dev(xs, "z")
    return z if xs[0]["interleaved"] else torch.stack([z.real, z.imag], 1).contiguous()


def _track_info(xs, **over):
    from vae_equalizer_amd.engine import awgn_track_info
    kw = dict(z=_z(xs), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), var=_dev(xs, "var"), shift=_dev(xs, "shift"), edge=xs[0]["edge"])
    kw.update(over)
    return awgn_track_info(**kw)


def _track_llr(xs, hyp, **over):
    from vae_equalizer_amd.engine import awgn_track_llr
    kw = dict(z=_z(xs), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], var=_dev(xs, "var"), shift=_dev(xs, "shift"), hyp=_hyp(hyp), edge=xs[0]["edge"])
    kw.update(over)
    return awgn_track_llr(**kw)


@functools.lru_cache(maxsize=None)
def _track_run(name):
    xs = K.track(name)[0]
    fig = _np(_track_info(xs))
    return fig, _track_llr(xs, fig["hyp"]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _track_model(name):
    xs, ms = K.track(name)
    out = [B.track_llr(x, m["hyp"]) for x, m in zip(xs, ms)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("name", list(K.TRACK))
def test_track_counts_figures_and_llrs(name):
    (fig, got), (want, mask) = _track_run(name), _track_model(name)
    xs, ms = K.track(name)
    assert len({(len(x["z"]), x["tx"].shape[-1], x["edge"], x["interleaved"]) for x in xs}) == 1
    _check_counts(fig, ms, name)
    fb = [max(Y_TOL["track"], FACTOR * (T.track_float32_deviation(x, m) or 0.0)) for x, m in zip(xs, ms)]
    _check_figures("track", "y", name, fig, ms, [(b, b) for b in fb])
    lb = [max(Y_LLR_TOL["track"], FACTOR * L.rel_dev(B.track_llr32(x, m["hyp"])[0], want[i], mask[i])) for i, (x, m) in enumerate(zip(xs, ms))]
    _check_llrs("track", "y", name, got, want, mask, lb)


@pytest.mark.parametrize("name", list(K.TRACK))
def test_track_sign_errors_and_gmi_of_the_llrs_are_the_info_kernels(name):
    fig, got = _track_run(name)
    _check_consistency("track", "y", name, K.track(name)[0], fig, got, _track_model(name)[1])


@pytest.mark.parametrize("name", ["Nd257-e31-s-12-dz1-il1", "Nd30-e0-s5-dz0-il0"])
def test_track_runs_in_one_call_give_the_bits_of_single_calls(name):
    xs = K.track(name)[0]
    hyp = np.array([3, 1])
    a, la = _track_info(xs), _track_llr(xs, hyp)
    for i in range(len(xs)):
        one, lone = _track_info(xs[i:i + 1]), _track_llr(xs[i:i + 1], hyp[i:i + 1])
        assert _same({k: v[i:i + 1] for k, v in a.items()}, one) and _same(la[i:i + 1], lone), i


def test_track_llr_hypotheses_outside_0_to_3_count_by_their_low_bits():
    xs = K.track("Nd256-e11-s11-dz1-il0")[0]
    hyp = np.array([1, 2], np.int64)
    want = _track_llr(xs, hyp)
    for other in (hyp + 4, hyp - 8, hyp - 2 ** 31):
        assert _same(want, _track_llr(xs, other)), other.tolist()
    assert _same(_track_llr(xs, np.full(2, 3)), _track_llr(xs, np.full(2, -1)))
    assert not _same(want, _track_llr(xs, np.full(2, 3)))


def test_the_largest_errors_of_this_module():
    """Printed last: per pair, mode and output the largest error relative to its bound."""
    for key in sorted(WORST):                                                   # ("... far": the samples far from the grid, held to the format's spacing)
        err, bound, where = WORST[key]
        print(f"{key[0]} {key[1]}-mode {key[2]}: largest error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f} ({where})")
    assert all(err <= bound for err, bound, _ in WORST.values())

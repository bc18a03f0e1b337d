"""vaeq_dp_epilogue_info / _llr and vaeq_cma_epilogue_info / _llr over their envelope (tests/_info_envelope_cases.py) against the float64 models
tests/_ref_info.py, _ref_llr.py, _ref_cma_info.py and _ref_baseline_llr.py, through the engine.py wrappers (the C ABI only where the output buffer is
filled with NaN first).  tests/test_ref_info_envelope_host.py asserts every case's preconditions on the CPU.

What the feature tests leave out: every shift in -10 .. 10, the frame lengths around the LLR grid's block edge and the info kernel's strided
rounds, batch_len < 20, >= 256, == 256 and == N (KeepWalk's carry against epi_keep per element), empty windows between kept runs, the clamp of a
shift nobody can find, (run, polarisation) pairs past the LLR grid's y limit, ties of posteriors and of hypotheses, TX samples off the grid,
subnormal posteriors, pmfs with zero entries, hypotheses outside 0 .. 7, samples far from the grid; for the CMA pair the four extreme shifts
of both stages with every exchange, and both LLR grids.

Bounds.  Counts: equal to the model's.  Erasures: +0.0 through the uint32 view.  q-mode: the project's Q_TOL = 1e-4 bit per float32 log2 and
Q_LLR_TOL = 2 Q_TOL ln 2 nats; a case with a 126-bit term (a subnormal posterior) has its figure bounded by Q_TOL times the figure's float32
log2 terms per symbol (2 for AIR, 2 b for GMI), the form of tests/test_epilogue_llr_gpu.py's _gmi_tol.  y-mode, per run: the larger of the pair's
existing bound and FACTOR = 4 times the deviation of the float32 restatement of that run (the kernel's operation order in numpy float32, never
the kernel) from the float64 model: the cost of float32 grows as the kept count shrinks.  The GMI recomputed from the LLRs and the sign
errors: the bounds of the feature tests' test_sign_errors_and_gmi_*.  Every test prints its figures before it asserts; the last test prints
the largest error of each pair and mode with its bound.
"""
import functools

import numpy as np
import pytest
import torch

import _info_envelope_cases as K
import _ref_baseline_llr as B
import _ref_cma_info as C
import _ref_info as I
import _ref_llr as L

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
FACTOR = 4
Q_TOL = 1e-4
Q_LLR_TOL = 2 * Q_TOL * LN2
Y_TOL = {"dp": 3 * I.Y_DEV, "cma": 3 * C.CMA_DEV}
Y_LLR_TOL = {"dp": 4 * L.Y_LLR_DEV, "cma": 4 * B.Y_LLR_DEV_CMA}
FIG = ("AIR", "GMI", "NGMI", "BER")
CNT = ("kept", "sym_err", "bit_err", "hyp")
ALIGN = ("shift_c", "r_c", "shift_q", "r_q")
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


# ------------------------------------------------------------------ the DP pair
def _src(xs, mode):
    if mode == "q":
        return dict(q=_dev(xs, "q"))
    return dict(y=_dev(xs, "y"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"))


def _info(xs, mode, **over):
    from vae_equalizer_amd.engine import dp_epilogue_info
    kw = dict(data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), shift=_dev(xs, "shift"), r=_dev(xs, "r"), batch_len=xs[0]["batch_len"],
              **_src(xs, mode))
    kw.update(over)
    return dp_epilogue_info(**kw)


def _llr(xs, mode, hyp, **over):
    from vae_equalizer_amd.engine import dp_epilogue_llr
    kw = dict(amp_levels=xs[0]["amp"], shift=_dev(xs, "shift"), r=_dev(xs, "r"), hyp=_hyp(hyp),
              batch_len=xs[0]["batch_len"], **_src(xs, mode))
    kw.update(over)
    return dp_epilogue_llr(**kw)


def _llr_into_nan(n, batch_len, amp, shift, r, hyp, q=None, y=None, nu_sc=None, var=None):
    """vaeq_dp_epilogue_llr through the C ABI into a buffer filled with NaN (device tensors in, the buffer out)."""
    from vae_equalizer_amd import _native as nat
    src = q if y is None else y
    R, N = src.shape[0], src.shape[-1]
    buf = torch.full((R, 2, 2 * L.nbits(n), N), float("nan"), dtype=torch.float32, device="cuda")
    f = lambda t: None if t is None else t.float().contiguous()
    q, y, nu_sc, var = f(q), f(y), f(nu_sc), f(var)
    amp = torch.as_tensor(np.asarray(amp), dtype=torch.float32).cuda()
    shift, r, hyp = shift.to(i32).contiguous(), r.to(i32).contiguous(), hyp.to(i32).contiguous()
    nat.check(nat.lib().vaeq_dp_epilogue_llr(R, N, n, int(batch_len or 0), nat.ptr(q), nat.ptr(y), nat.ptr(amp), nat.ptr(var), nat.ptr(nu_sc),
                                             nat.ptr(shift, i32), nat.ptr(r, i32), nat.ptr(hyp, i32), nat.ptr(buf), nat.current_stream(buf.device)),
              "vaeq_dp_epilogue_llr")
    return buf


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    """One information-rate launch and one LLR launch under its hypotheses per (launch, mode), shared by the tests."""
    xs = K.dp(name)[0]
    fig = _np(_info(xs, mode))
    return fig, _llr(xs, mode, fig["hyp"]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    """-> (planes[R,2,2b,N] float64, mask[R,2,N]) under the information-rate model's hypotheses."""
    xs, mq, my = K.dp(name)
    out = [_dp_planes(x, m["hyp"], mode) for x, m in zip(xs, mq if mode == "q" else my)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _dp_planes(x, hyp, mode, f=np.float64):
    if mode == "q":
        return L.dp_llr_q(x["q"], x["n"], x["shift"], x["r"], hyp, x["batch_len"])
    return L.dp_llr_y(x["y"], x["n"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], hyp, x["batch_len"], f)


def _check_counts(got, models, tag):
    print(f"{tag}: " + ", ".join(f"{k} {got[k].tolist()}" for k in CNT))
    for i, m in enumerate(models):
        for k in CNT:
            assert np.array_equal(got[k][i], np.asarray(m[k])), (tag, i, k, got[k][i], m[k])
        if np.max(m["kept"]) == 0:
            for k in FIG:
                assert np.isnan(got[k][i]).all(), (tag, i, k)


def _check_figures(pair, mode, tag, got, models, bounds):
    """|kernel - model| of AIR, GMI, NGMI within bounds[i] = (AIR bound, GMI bound) of run i, BER within one float32 division."""
    for i, m in enumerate(models):
        if np.max(m["kept"]) == 0:
            continue
        d = {k: float(np.abs(got[k][i].astype(np.float64) - np.asarray(m[k])).max()) for k in FIG}
        ba, bg = bounds[i]
        print(f"{mode}-mode {tag} run {i} (kept {np.asarray(m['kept']).tolist()}): " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()) + f"; bounds {ba:.2e} {bg:.2e}")
        _record((pair, mode, "AIR"), d["AIR"], ba, f"{tag} run {i}")
        _record((pair, mode, "GMI"), d["GMI"], bg, f"{tag} run {i}")
        assert d["AIR"] <= ba and d["GMI"] <= bg and d["NGMI"] <= bg and d["BER"] <= 1e-7, (tag, i, d)


def _gmi_and_sign_errors(llr, bits, mask, P):
    R = llr.shape[0]
    gmi, err = np.full((R, 2), np.nan), np.zeros((R, 2), np.int64)
    for i in range(R):
        for p in range(2):
            gmi[i, p] = L.gmi_from_llr(llr[i, p], bits[i, p], mask[i, p], I.entropy(P[i]))
            err[i, p] = L.sign_errors(llr[i, p], bits[i, p], mask[i, p])
    return gmi, err


def _gmi_tol(pair, mode, n, llr, mask):
    """2 b (LLR bound in bit) + the information-rate kernel's own bound: tests/test_epilogue_llr_gpu.py's and tests/test_cma_llr_gpu.py's."""
    b2 = 2 * L.nbits(n)
    if mode == "q":
        return b2 * (Q_LLR_TOL / LN2) + Q_TOL
    big = float(np.abs(llr[np.broadcast_to(mask[:, :, None, :], llr.shape)]).max()) if mask.any() else 0.0
    return b2 * (Y_LLR_TOL[pair] * max(1.0, big) / LN2) + Y_TOL[pair]


def _check_consistency(pair, mode, tag, xs, fig, got, mask):
    """Pair consistency: the mask is the kept count, the LLR signs that contradict the TX bits are bit_err, the GMI of the LLRs is the reported one."""
    from vae_equalizer_amd.engine import label_bits
    n = xs[0]["n"]
    bits = label_bits(_dev(xs, "tx"), n).cpu().numpy().astype(np.int64)
    assert np.array_equal(bits, np.stack([L.label_bits(x["tx"], n) for x in xs]))
    gmi, err = _gmi_and_sign_errors(got, bits, mask, [x["P"] for x in xs])
    tol = _gmi_tol(pair, mode, n, got, mask)
    kept = fig["kept"] > 0
    d = float(np.abs(gmi - fig["GMI"])[kept].max()) if kept.any() else 0.0
    print(f"{mode}-mode {tag}: sign errors {err.tolist()} bit_err {fig['bit_err'].tolist()}; max |GMI(LLR) - GMI| {d:.3e} bit (bound {tol:.3e})")
    assert np.array_equal(mask.sum(-1), fig["kept"]) and np.array_equal(err, fig["bit_err"])
    assert np.array_equal(np.isnan(gmi), ~kept) and d <= tol


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.DP))
def test_dp_counts_equal_the_model(name, mode):
    _check_counts(_run(name, mode)[0], K.dp(name)[1 if mode == "q" else 2], f"{mode}-mode {name}")


@pytest.mark.parametrize("name", list(K.DP))
def test_dp_q_mode_figures_and_llrs(name):
    (fig, got), (want, mask) = _run(name, "q"), _model(name, "q")
    xs, models, _ = K.dp(name)
    _check_figures("dp", "q", name, fig, models, [(Q_TOL, Q_TOL)] * len(xs))
    m = np.broadcast_to(mask[:, :, None, :], want.shape)
    dev = float(np.abs(got.astype(np.float64) - want)[m].max()) if m.any() else 0.0
    print(f"q-mode {name}: max |LLR - model| {dev:.3e} nats over {int(m.sum())} kept entries (bound {Q_LLR_TOL:.3e})")
    _record(("dp", "q", "LLR"), dev, Q_LLR_TOL, name)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and dev <= Q_LLR_TOL
    assert _erasures_are_plus_zero(got, mask)


@pytest.mark.parametrize("name", list(K.DP))
def test_dp_y_mode_figures_and_llrs(name):
    (fig, got), (want, mask) = _run(name, "y"), _model(name, "y")
    xs, _, models = K.dp(name)
    fb = [max(Y_TOL["dp"], FACTOR * (I.y_mode_float32_deviation(x) or 0.0)) for x in xs]
    _check_figures("dp", "y", name, fig, models, [(b, b) for b in fb])
    assert np.isfinite(got).all() and _erasures_are_plus_zero(got, mask)
    for i, (x, m) in enumerate(zip(xs, models)):
        p32 = _dp_planes(x, m["hyp"], "y", np.float32)[0]
        bound = max(Y_LLR_TOL["dp"], FACTOR * L.rel_dev(p32, want[i], mask[i]))
        dev = L.rel_dev(got[i], want[i], mask[i])
        print(f"y-mode {name} run {i}: max |LLR - model| / max(1, |model|) {dev:.3e} (bound {bound:.3e}), largest |lam| {np.abs(want[i]).max():.1f} nats")
        _record(("dp", "y", "LLR"), dev, bound, f"{name} run {i}")
        assert dev <= bound, (name, i)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.DP))
def test_dp_llr_writes_every_entry_of_a_nan_filled_buffer(name, mode):
    xs = K.dp(name)[0]
    fig, want = _run(name, mode)
    buf = _llr_into_nan(xs[0]["n"], xs[0]["batch_len"], xs[0]["amp"], _dev(xs, "shift"), _dev(xs, "r"), torch.from_numpy(fig["hyp"]).cuda(), **_src(xs, mode))
    got = buf.cpu().numpy()
    print(f"{mode}-mode {name}: {int(np.isnan(got).sum())} NaN left of {got.size}")
    assert not np.isnan(got).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _erasures_are_plus_zero(got, _model(name, mode)[1])


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", list(K.DP))
def test_dp_sign_errors_and_gmi_of_the_llrs_are_the_info_kernels(name, mode):
    fig, got = _run(name, mode)
    _check_consistency("dp", mode, name, K.dp(name)[0], fig, got, _model(name, mode)[1])


@pytest.mark.parametrize("name", [n for n in K.DP if n.startswith("B")])
def test_dp_symbol_errors_are_the_epilogues_ser_on_its_own_alignment(name):
    """On the alignment dp_epilogue itself finds on the same inputs, sym_err / kept is its soft-demapper SER bit for bit, NaN where empty."""
    from vae_equalizer_amd.engine import dp_epilogue
    xs = K.dp(name)[0]
    ep = dp_epilogue(_dev(xs, "q"), _dev(xs, "y"), _dev(xs, "tx"), xs[0]["amp"], _dev(xs, "nu_sc"), _dev(xs, "var"), batch_len=xs[0]["batch_len"])
    got = _info(xs, "q", shift=ep["shift_q"], r=ep["r_q"])
    ser = got["sym_err"].float() / got["kept"].float()                         # 0 / 0 = NaN, the epilogue's empty window
    print(f"{name}: shift_q {ep['shift_q'].tolist()} SER_q {ep['SER'][:, 2:4].tolist()} sym_err / kept {ser.tolist()}")
    assert torch.equal(torch.nan_to_num(ser, nan=-1.0), torch.nan_to_num(ep["SER"][:, 2:4], nan=-1.0))
    assert torch.equal(torch.isnan(ser), got["kept"] == 0)


def test_dp_runs_in_one_call_give_the_bits_of_single_calls():
    xs = K.dp("B257-N771")[0]
    hyp = np.array([[1, 6], [4, 3], [7, 2], [0, 5], [2, 2]], np.int64)
    for mode in ("q", "y"):
        a, la = _info(xs, mode), _llr(xs, mode, hyp)
        for i in range(len(xs)):
            one, lone = _info(xs[i:i + 1], mode), _llr(xs[i:i + 1], mode, hyp[i:i + 1])
            assert _same({k: v[i:i + 1] for k, v in a.items()}, one) and _same(la[i:i + 1], lone), (mode, i)


@pytest.mark.parametrize("mode", ["q", "y"])
@pytest.mark.parametrize("name", ["clamp-B0", "clamp-B100"])
def test_dp_shifts_beyond_ten_are_clamped(name, mode):
    """shift in {+-11, +-1000, INT32_MIN, INT32_MAX}: the outputs are the bits of the call with the clamped shift."""
    xs = K.dp(name)[0]
    wild = _dev(xs, "wild")
    a, b = _info(xs, mode), _info(xs, mode, shift=wild)
    la, lb = _llr(xs, mode, a["hyp"]), _llr(xs, mode, a["hyp"], shift=wild)
    print(f"{mode}-mode {name}: shifts {wild.tolist()} as {_dev(xs, 'shift').tolist()}: kept {b['kept'].tolist()}")
    assert (a["kept"] > 200).all() and _same(a, b) and _same(la, lb)


@pytest.mark.parametrize("mode", ["q", "y"])
def test_dp_llr_grid_stride_past_32768_pairs(mode):
    """R = 16385 runs = 32770 (run, polarisation) pairs, two more than the LLR grid's y limit: a three-run base launch tiled (16385 = 3 * 5461 + 2,
    so the last run is base run 1).  Every run's outputs are its base run's single-launch bits; the LLR buffer is filled with NaN first."""
    xs = K.dp("stride")[0]
    R = 16385
    idx = torch.arange(R, device="cuda") % 3
    tile = lambda t: t[idx].contiguous()
    base = _info(xs, mode)
    base_llr = _llr(xs, mode, base["hyp"])
    src = {k: tile(v) for k, v in _src(xs, mode).items()}
    shift, r, hyp = tile(_dev(xs, "shift")), tile(_dev(xs, "r")), tile(base["hyp"])
    from vae_equalizer_amd.engine import dp_epilogue_info
    big = dp_epilogue_info(data=tile(_dev(xs, "tx")), amp_levels=xs[0]["amp"], P=tile(_dev(xs, "P")), shift=shift, r=r, **src)
    buf = _llr_into_nan(2, None, xs[0]["amp"], shift, r, hyp, **src)
    left = int(torch.isnan(buf).sum())
    print(f"{mode}-mode: R = {R}, {left} NaN left of {buf.numel()}; last run's kept {big['kept'][-1].tolist()} (base run 1: {base['kept'][1].tolist()})")
    assert left == 0 and _same(buf, tile(base_llr))
    assert _same(big, {k: tile(v) for k, v in base.items()})
    assert int(base["kept"].min()) >= 11 and not torch.equal(base_llr[0], base_llr[1])


@pytest.mark.parametrize("mode", ["q", "y"])
def test_dp_llr_hypotheses_outside_0_to_7_count_by_their_low_bits(mode):
    xs = K.dp("N257")[0]
    hyp = np.array([[0, 5], [3, 6], [7, 1], [2, 4]], np.int64)
    want = _llr(xs, mode, hyp)
    for other in (hyp + 8, hyp - 8, hyp + 8 * 1000003, hyp - 2 ** 31):
        assert _same(want, _llr(xs, mode, other)), other.tolist()
    assert _same(_llr(xs, mode, np.full((4, 2), 7)), _llr(xs, mode, np.full((4, 2), -1)))
    assert not _same(want, _llr(xs, mode, np.full((4, 2), 7)))


def _planted_tols(name, n):
    big = name.startswith("subnormal")                                          # a 126-bit term: Q_TOL per float32 log2 term of a symbol
    return (2 * Q_TOL, 2 * L.nbits(n) * Q_TOL) if big else (Q_TOL, Q_TOL)


@pytest.mark.parametrize("name", list(K.PLANTED_DP) + list(K.DP_TIES))
def test_dp_planted_q_mode_edges(name):
    """Ties of posteriors (the first maximum) and of hypotheses (the smallest), TX samples off the grid, subnormal posteriors (126 bit, finite LLRs),
    pmfs with zero entries: counts and hypothesis are the model's, figures and LLRs within the q-mode bounds.  The sign errors of the LLRs are
    compared where no posterior ties: an LLR of exactly zero has no sign."""
    x, m = K.planted_dp(name)
    n = x["n"]
    fig = _np(_info([x], "q"))
    got = _llr([x], "q", fig["hyp"]).cpu().numpy()
    _check_counts(fig, [m], name)
    _check_figures("dp", "q", name, fig, [m], [_planted_tols(name, n)])
    want, mask = L.dp_llr_q(x["q"], n, x["shift"], x["r"], m["hyp"], None)
    dev = float(np.abs(got[0] - want).max())
    print(f"{name}: cnt {m['cnt'].T.tolist()}, max |LLR - model| {dev:.3e} nats, largest |lam| {np.abs(want).max():.1f}")
    _record(("dp", "q", "LLR"), dev, Q_LLR_TOL, name)
    assert np.isfinite(got).all() and dev <= Q_LLR_TOL and _erasures_are_plus_zero(got, mask[None])
    if name.startswith("subnormal"):
        assert np.abs(want).max() > 120 * LN2 and np.min(fig["AIR"]) < -126.0 * 2 / 38
    if not name.startswith("posterior-tie"):
        bits = L.label_bits(x["tx"], n)
        assert [L.sign_errors(got[0, p], bits[p], mask[p]) for p in range(2)] == fig["bit_err"][0].tolist()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_dp_y_mode_far_from_the_grid(n):
    """|y| = 50 and var = 1e-6 on eight kept symbols per row: exponents of 1e9 bit stay finite, the decisions are the outer level's."""
    x, m = K.far_dp(n)
    fig = _np(_info([x], "y"))
    got = _llr([x], "y", fig["hyp"]).cpu().numpy()
    _check_counts(fig, [m], f"far n_lev {n}")
    # exponents of 1e9 .. 1e10 bit are spaced 128 .. 1024 bit apart in float32: the figures are held to what the format can hold of each symbol's term
    b = max(Y_TOL["dp"], FACTOR * (I.y_mode_float32_deviation(x) or 0.0))
    _check_figures("dp far", "y", f"far-n{n}", fig, [m], [tuple(max(b, f) for f in m["format_bounds"])])
    want, mask = L.dp_llr_y(x["y"], n, x["amp"], x["nu_sc"], x["var"], x["shift"], 0, m["hyp"], None)
    bits = L.label_bits(x["tx"], n)
    print(f"far n_lev {n}: largest |LLR| {np.abs(got).max():.3e} nats (model {np.abs(want).max():.3e})")
    assert np.isfinite(got).all() and all(np.isfinite(fig[k]).all() for k in FIG) and fig["sym_err"].tolist() == [[0, 0]]
    assert [L.sign_errors(got[0, p], bits[p], mask[p]) for p in range(2)] == [0, 0] and np.abs(got).max() > 1e6


# ------------------------------------------------------------------ the CMA pair
def _cma_info(xs, **over):
    from vae_equalizer_amd.engine import cma_epilogue_info
    kw = dict(y=_dev(xs, "y"), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"),
              **{k: _dev(xs, k) for k in ALIGN})
    kw.update(over)
    return cma_epilogue_info(**kw)


def _cma_llr(xs, hyp, **over):
    from vae_equalizer_amd.engine import cma_epilogue_llr
    kw = dict(y=_dev(xs, "y"), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"),
              **{k: _dev(xs, k) for k in ALIGN}, hyp=_hyp(hyp))
    kw.update(over)
    return cma_epilogue_llr(**kw)


@functools.lru_cache(maxsize=None)
def _cma_run(name):
    xs = K.cma(name)[0]
    fig = _np(_cma_info(xs))
    return fig, _cma_llr(xs, fig["hyp"]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _cma_model(name):
    xs, ms = K.cma(name)
    out = [B.cma_llr(x, m["hyp"]) for x, m in zip(xs, ms)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("name", list(K.CMA))
def test_cma_counts_figures_and_llrs(name):
    (fig, got), (want, mask) = _cma_run(name), _cma_model(name)
    xs, ms = K.cma(name)
    _check_counts(fig, ms, name)
    fb = [max(Y_TOL["cma"], FACTOR * (C.float32_deviation(x, ordered=True) or 0.0)) for x in xs]
    _check_figures("cma", "y", name, fig, ms, [(b, b) for b in fb])
    assert np.isfinite(got).all() and _erasures_are_plus_zero(got, mask)
    for i, (x, m) in enumerate(zip(xs, ms)):
        bound = max(Y_LLR_TOL["cma"], FACTOR * L.rel_dev(B.cma_llr32(x, m["hyp"])[0], want[i], mask[i]))
        dev = L.rel_dev(got[i], want[i], mask[i])
        print(f"{name} run {i}: max |LLR - model| / max(1, |model|) {dev:.3e} (bound {bound:.3e}), largest |lam| {np.abs(want[i]).max():.1f} nats")
        _record(("cma", "y", "LLR"), dev, bound, f"{name} run {i}")
        assert dev <= bound, (name, i)


@pytest.mark.parametrize("name", list(K.CMA))
def test_cma_sign_errors_and_gmi_of_the_llrs_are_the_info_kernels(name):
    fig, got = _cma_run(name)
    _check_consistency("cma", "y", name, K.cma(name)[0], fig, got, _cma_model(name)[1])


def test_cma_runs_in_one_call_give_the_bits_of_single_calls():
    xs = K.cma("extremes0-n8")[0]
    hyp = (np.arange(16).reshape(8, 2) * 3) % 8
    a, la = _cma_info(xs), _cma_llr(xs, hyp)
    for i in range(len(xs)):
        one, lone = _cma_info(xs[i:i + 1]), _cma_llr(xs[i:i + 1], hyp[i:i + 1])
        assert _same({k: v[i:i + 1] for k, v in a.items()}, one) and _same(la[i:i + 1], lone), i


@pytest.mark.parametrize("R", [512, 513])
def test_cma_both_llr_grids_give_the_base_launchs_bits(R):
    """Up to 512 runs a run's polarisations go to two workgroups, beyond that to one: four base runs tiled to R = 512 and R = 513."""
    xs = K.cma("N43")[0]
    idx = torch.arange(R, device="cuda") % 4
    tile = lambda t: t[idx].contiguous()
    base = _cma_info(xs)
    base_llr = _cma_llr(xs, base["hyp"])
    over = dict(y=tile(_dev(xs, "y")), data=tile(_dev(xs, "tx")), nu_sc=tile(_dev(xs, "nu_sc")), var=tile(_dev(xs, "var")),
                **{k: tile(_dev(xs, k)) for k in ALIGN})
    big = _cma_info(xs, P=tile(_dev(xs, "P")), **over)
    big_llr = _cma_llr(xs, tile(base["hyp"]), **over)
    print(f"R = {R}: kept of the last run {big['kept'][-1].tolist()} (base run {(R - 1) % 4}: {base['kept'][(R - 1) % 4].tolist()})")
    assert _same(big, {k: tile(v) for k, v in base.items()}) and _same(big_llr, tile(base_llr))


def test_cma_llr_hypotheses_outside_0_to_7_count_by_their_low_bits():
    xs = K.cma("N257")[0]
    hyp = np.array([[0, 5], [3, 6], [7, 1], [2, 4]], np.int64)
    want = _cma_llr(xs, hyp)
    for other in (hyp + 8, hyp - 8, hyp - 2 ** 31):
        assert _same(want, _cma_llr(xs, other)), other.tolist()
    assert _same(_cma_llr(xs, np.full((4, 2), 7)), _cma_llr(xs, np.full((4, 2), -1)))


def test_the_largest_errors_of_this_module():
    """Printed last: per pair, mode and output the largest error relative to its bound."""
    for key in sorted(WORST):                                                   # ("... far": the samples far from the grid, held to the format's spacing)
        err, bound, where = WORST[key]
        print(f"{key[0]} {key[1]}-mode {key[2]}: largest error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f} ({where})")
    assert all(err <= bound for err, bound, _ in WORST.values())

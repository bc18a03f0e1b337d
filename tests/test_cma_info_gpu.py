"""vaeq_cma_epilogue_info (GMI, NGMI, achievable rate, pre-FEC BER of a frame of the constant-modulus DP baselines) against the float64 model
tests/_ref_cma_info.py, and through cma_runs.run_cma_batch(want_info=True) and the Eval_run_DP script.

Launches of R = 3 runs: N in {43, 47, 400, 1030} (the smallest row, an odd one, one beyond 4 x 256 symbols), n_lev in {2, 4, 8}, constellation-stage
shifts (-10, 0) / (0, 10) / (10, -10), soft-demapper-stage shifts (0, 0) / (2, -1) / (-3, 3), both r_c and r_q, every hypothesis, a window scale of
0.8 / 1.25 / 0.6 that the mean-radius normalisation has to undo inside W_c and must leave alone outside it, uniform and heavily shaped pmf.
tests/test_ref_cma_info_host.py asserts the preconditions (top-two posterior gap above 0.05, planted counts recovered by the model).

Bounds.  Counts are exact.  AIR, GMI and NGMI: three times CMA_DEV, the deviation of the kernel's operation order evaluated in numpy float32 from the
float64 model (the margin of tests/test_epilogue_info_gpu.py's y-mode, for its reason: the device's exp2 / log2 are not numpy's and its sums run in
another order).  BER: 1e-7, one float32 division.  Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _ref_cma_info as C
import _ref_epilogue as E

pytestmark = pytest.mark.gpu

TOL = 3 * C.CMA_DEV
FIG, CNT = C.FIG, C.CNT
ALIGN = ("shift_c", "r_c", "shift_q", "r_q")


def _dev(xs, key, dtype=None):
    a = np.stack([np.asarray(x[key]) for x in xs])
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _call(xs, **over):
    from vae_equalizer_amd.engine import cma_epilogue_info
    kw = dict(y=_dev(xs, "y"), data=_dev(xs, "tx"), amp_levels=xs[0]["amp"], P=_dev(xs, "P"), nu_sc=_dev(xs, "nu_sc"), var=_dev(xs, "var"),
              **{k: _dev(xs, k) for k in ALIGN})
    kw.update(over)
    return cma_epilogue_info(**kw)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One kernel launch per launch name, shared by the tests; -> dict of numpy arrays [R,2]."""
    return {k: v.cpu().numpy() for k, v in _call(C.build_launch(name)[0]).items()}


def _same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_counts_equal_the_model(name):
    got, models = _run(name), C.build_launch(name)[1]
    for i, m in enumerate(models):
        for k in CNT:
            assert np.array_equal(got[k][i], m[k]), (i, k, got[k][i], m[k])


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_figures(name):
    got, models = _run(name), C.build_launch(name)[1]
    dev = {k: max(np.abs(got[k][i].astype(np.float64) - m[k]).max() for i, m in enumerate(models)) for k in FIG}
    print(f"{name}: max |kernel - model| " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()) + f" (bound {TOL:.2e})")
    assert dev["AIR"] <= TOL and dev["GMI"] <= TOL and dev["NGMI"] <= TOL
    assert dev["BER"] <= 1e-7
    for k in FIG:
        assert got[k].dtype == np.float32 and got[k].shape == (3, 2)
    for k in CNT:
        assert got[k].dtype == np.int64 and got[k].shape == (3, 2)


@pytest.mark.parametrize("name", [n for n in C.LAUNCHES if n.startswith(("N400-", "N1030-"))])
def test_symbol_errors_are_the_epilogue_ser(name):
    """On the alignment cma_epilogue itself returns for the launch's frames: the runs built with a zero stage-q shift and r_q = 0 are found as planted,
    and there sym_err / kept is its soft-demapper SER, exactly."""
    from vae_equalizer_amd.engine import cma_epilogue
    xs = C.build_launch(name)[0]
    ep = cma_epilogue(_dev(xs, "y"), _dev(xs, "tx"), xs[0]["amp"], _dev(xs, "nu_sc"), _dev(xs, "var"))
    got = _call(xs, **{k: ep[k] for k in ALIGN})
    ser = (got["sym_err"].float() / got["kept"].float()).cpu()
    sel = [i for i, x in enumerate(xs) if not x["shift_q"].any() and x["r_q"] == 0]
    print(f"{name}: runs {sel}; epilogue shift_c {ep['shift_c'].tolist()} r_c {ep['r_c'].tolist()} shift_q {ep['shift_q'].tolist()} r_q {ep['r_q'].tolist()}; "
          f"SER_q {ep['SER'][:, 2:4].tolist()} sym_err / kept {ser.tolist()}")
    for i in sel:
        x = xs[i]
        assert ep["shift_c"][i].tolist() == x["shift_c"].tolist() and int(ep["r_c"][i]) == x["r_c"]
        assert ep["shift_q"][i].tolist() == [0, 0] and int(ep["r_q"][i]) == 0
        assert torch.equal(ser[i], ep["SER"][i, 2:4].cpu())
        assert got["sym_err"][i].tolist() == list(x["n_err"])


def test_the_selected_runs_cover_both_long_rows():
    sel = [(n, i) for n in C.LAUNCHES if n.startswith(("N400-", "N1030-")) for i, x in enumerate(C.build_launch(n)[0])
           if not x["shift_q"].any() and x["r_q"] == 0]
    assert {n.split("-")[0] for n, _ in sel} == {"N400", "N1030"} and len(sel) >= 3


@pytest.mark.parametrize("name", ["N1030-n8", "N47-n4"])
def test_determinism(name):
    """Two calls give identical bits, and a launch of three runs gives the bits of three launches of one run."""
    xs = C.build_launch(name)[0]
    a, b = _call(xs), _call(xs)
    singles = [_call([x]) for x in xs]
    for k in FIG + CNT:
        assert _same_bits(a[k], b[k]), k
        assert _same_bits(a[k], torch.cat([s[k] for s in singles])), k


def test_zero_output_gives_nan_figures_and_zero_counts_and_disturbs_no_other_run():
    xs = C.build_launch("N400-n8")[0]
    base = _call(xs)
    y = _dev(xs, "y").clone()
    y[1] = 0
    got = _call(xs, y=y)
    for k in FIG:
        assert torch.isnan(got[k][1]).all(), k
    for k in CNT:
        assert not got[k][1].any(), k
    for k in FIG + CNT:
        assert torch.equal(got[k][[0, 2]], base[k][[0, 2]]) and torch.isfinite(base[k].float()).all(), k


def test_shifts_are_clamped():
    """An alignment outside what the epilogue can return is clamped to +-10, as the DP info kernel clamps its own: no index leaves the row."""
    xs = C.build_launch("N43-n4")[0]
    sc, sq = _dev(xs, "shift_c").clone(), _dev(xs, "shift_q").clone()
    sc[0, 0], sq[2, 1] = -10, 10
    want = _call(xs, shift_c=sc, shift_q=sq)
    sc[0, 0], sq[2, 1] = -1000, 2 ** 31 - 1
    got = _call(xs, shift_c=sc, shift_q=sq)
    for k in FIG + CNT:
        assert _same_bits(got[k], want[k]), k


@pytest.mark.parametrize("name", ["G14_cma_epilogue_64qam", "G14_cma_epilogue_64qam_pcs"])
def test_reference_frame_agrees_with_the_materialised_sequence(name):
    """On the last frame of a hand-driven reference loop: the figures from the raw y are those of vaeq_dp_epilogue_info's y-mode on the aligned,
    window-normalised sequence that the torch restatement of the reference's steps materialises (its factor is torch's sum, this kernel's is its
    own: a sample within float32 rounding of a threshold may decide differently, so counts may differ by one)."""
    from conftest import load_golden
    from vae_equalizer_amd.cma_runs import N_CUT, cma_frame_epilogue, cma_frame_epilogue_torch
    from vae_equalizer_amd.engine import dp_epilogue_info
    g = load_golden(name)
    R = 3
    rep = lambda a: torch.from_numpy(a)[None].expand(R, *a.shape).contiguous().cuda()
    amp = torch.from_numpy(g["amp_levels"]).cuda()
    n = amp.numel()
    var = torch.from_numpy(g["var"])[None].expand(R, 2).contiguous().cuda()
    nu = torch.full((R,), float(g["nu_sc"]), device="cuda")
    P = torch.exp(-nu[0] * amp ** 2)
    P = (P / P.sum()).reshape(1, n).expand(R, n).contiguous()
    rt = cma_frame_epilogue_torch(rep(g["cma_out"]), rep(g["data"]), amp, nu, var)
    rk = cma_frame_epilogue(rep(g["cma_out"]), rep(g["data"]), amp, nu, var, P=P)
    for k in ALIGN:
        assert torch.equal(rt[k], rk[k]), k
    ref = dp_epilogue_info(y=rt["y"].contiguous(), data=rep(g["data"])[..., N_CUT:-N_CUT], amp_levels=amp, P=P, nu_sc=nu, var=var, shift=rt["shift_q"],
                           r=rt["r_q"])
    got = rk["info"]
    print(f"{name}: GMI {got['GMI'][0].tolist()} (materialised {ref['GMI'][0].tolist()}) NGMI {got['NGMI'][0].tolist()} BER {got['BER'][0].tolist()} "
          f"sym_err {got['sym_err'][0].tolist()} / {ref['sym_err'][0].tolist()} of {got['kept'][0].tolist()}; SER_q {rk['SER'][0, 2:4].tolist()}")
    assert torch.equal(got["kept"], ref["kept"]) and torch.equal(got["hyp"], ref["hyp"])
    assert (got["sym_err"] - ref["sym_err"]).abs().max() <= 1
    K = got["kept"].double()
    assert ((got["sym_err"].double() - rk["SER"][:, 2:4].double() * K).abs() <= 1).all()
    for k in ("AIR", "GMI"):                                                   # a sample at a threshold moves its term by next to nothing; fac by ~1e-7 relative
        assert (got[k] - ref[k]).abs().max() <= 1e-3 * max(1.0, float(ref[k].abs().max())), k


RUN_KW = dict(mod="64-QAM", sps=2, M_est=25, batch_len=100, N_train_max=400, num_frames=2, flex_step=10, channel="h0", tau_cd=-26e-24,
              tau_pmd=0.1e-12 * np.sqrt(1000), phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), N_lrhalf=170)


@pytest.mark.parametrize("mode,lr", [("CMA", 1e-4), ("CMAbatch", 1e-4), ("CMAflex", 1e-5)])   # step sizes at which two frames do not diverge
def test_run_cma_batch_want_info(mode, lr, monkeypatch):
    from vae_equalizer_amd import cma_runs
    from vae_equalizer_amd.dp_runs import DPRun
    runs = [DPRun(22 + 2 * i, (0.0, 0.0270955)[i], 0.01, 0.3, lr, 90e9, seed=500 + i) for i in range(2)]
    seen = []
    inner = cma_runs.cma_frame_epilogue

    def spy(out_const, data, amp, nu_sc, var, P=None):
        res = inner(out_const, data, amp, nu_sc, var, P=P)
        seen.append((out_const.shape[-1] - 2 * cma_runs.N_CUT, res["shift_q"].cpu(), P is not None))
        return res
    monkeypatch.setattr(cma_runs, "cma_frame_epilogue", spy)
    a = cma_runs.run_cma_batch(runs, mode, want_info=True, **RUN_KW)
    n_on = len(seen)
    b = cma_runs.run_cma_batch(runs, mode, **RUN_KW)
    assert n_on == 2 and len(seen) == 4 and [s[2] for s in seen] == [True, True, False, False]
    assert "info" not in b and set(a) - set(b) == {"info"}
    assert a["SER"].shape == (2, 4, 2) and _same_bits(a["SER"], b["SER"])
    assert torch.equal(a["Var_est"], b["Var_est"]) and torch.equal(a["var"], b["var"])
    info = a["info"]
    print(f"{mode}: GMI {info['GMI'].tolist()} NGMI {info['NGMI'].tolist()} AIR {info['AIR'].tolist()} BER {info['BER'].tolist()} kept {info['kept'].tolist()} "
          f"sym_err {info['sym_err'].tolist()} SER_q {a['SER'][:, 2:4].tolist()}")
    assert set(info) == set(FIG + CNT)
    for k in FIG:
        assert info[k].shape == (2, 2, 2) and info[k].dtype == torch.float32 and not info[k].is_cuda and torch.isfinite(info[k]).all(), k
    for k in CNT:
        assert info[k].shape == (2, 2, 2) and info[k].dtype == torch.int64 and not info[k].is_cuda, k
    for f in range(2):
        N, shift_q, _ = seen[f]                                                # N: the frame length after the [10:-10] cut (N_train_max - 20)
        assert N == RUN_KW["N_train_max"] - 2 * cma_runs.N_CUT
        kept = N - 2 * E.EDGE - shift_q.abs().max(dim=1).values                # the window [11, N - 11 - max|shift_q|) = N_train_max - 42 - max|shift_q|
        assert torch.equal(info["kept"][:, :, f], kept[:, None].expand(2, 2))
    err = (info["sym_err"].double() - a["SER"][:, 2:4].double() * info["kept"].double()).abs()
    assert (err <= 1).all(), err.tolist()


DP_KEYS = {"SER", "Var_est", "var_real", "SNR", "nu", "theta_diff", "theta", "M", "lr", "batch_len", "symb_rate", "symb_step"}


@pytest.mark.parametrize("on", [False, True])
def test_eval_run_dp_script_info_metrics_on_the_cma_baseline(tmp_path, monkeypatch, on):
    import scipy.io as io
    from vae_equalizer_amd import Eval_run_DP as ev
    for k, v in dict(loss_type="CMA", mod="64-QAM", SNR_vec=[20], nu_vec=[0, 0.0270955], lr_optim_vec=[1e-4], iter=2, num_frames=2, N_frame_max=400,
                     savePATH=str(tmp_path) + "/", base_seed=9, info_metrics=on).items():
        monkeypatch.setattr(ev, k, v)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    print(f"info_metrics={on}: keys {sorted(m.dtype.names)}" + (f" GMI {d['GMI'].ravel().tolist()} BER {d['BER'].ravel().tolist()}" if on else ""))
    assert "SERvsSNR_CMA_DP_64-QAM_" in name
    assert set(m.dtype.names) == (DP_KEYS | {"GMI", "NGMI", "AIR", "BER"} if on else DP_KEYS) and set(d) == set(m.dtype.names)
    assert d["SER"].shape == (4, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 2)
    if on:
        for k in ("GMI", "NGMI", "AIR", "BER"):
            assert d[k].shape == (2,) + d["SER"].shape[1:] and d[k].dtype == np.float32 and np.isfinite(d[k]).all(), k

"""fec_metrics of the sweep scripts: one small seeded sweep point through Eval_run_shaping_vaele and through Eval_run_DP (one VAE and one
constant-modulus loss_type).  The .mat gains BER_post, FER, BER_pre_fec and fec_iters, one value per sweep point and run (the shape of SER
without its frame / validation axis, and without the DP script's leading axis); they are what the batch runner returns under "fec" for the
same seeds; with fec_metrics = None the .mat has exactly the old key set.  Eval_run_shaping_cma and Eval_run_vaenn, which share the row packer,
are held to the schema and the shapes, and DFE_MQAM_shaping.main to its longer return value."""
import numpy as np
import pytest
import scipy.io as io
import torch

pytestmark = pytest.mark.gpu

FEC_KEYS = ("BER_post", "FER", "BER_pre_fec", "fec_iters")
DP_KEYS = {"SER", "Var_est", "var_real", "SNR", "nu", "theta_diff", "theta", "M", "lr", "batch_len", "symb_rate", "symb_step"}
LE_KEYS = {"SER", "SNR", "M", "lr", "N_train", "nu"}


def _fec(depth):
    from vae_equalizer_amd.engine import array_code
    return dict(code=array_code(4, 24, 31), t0=13, max_iter=8, depth=depth)


def _want(fec):
    """The runner's figures -> [R, 4] in FEC_KEYS order."""
    return np.stack([fec["BER_post"].cpu().numpy(), fec["FER"].cpu().numpy(), fec["BER_pre"].cpu().numpy(),
                     fec["iters"].double().mean(1).float().cpu().numpy()], 1)


def _main(ev, tmp_path, monkeypatch, const, fec):
    for k, v in dict(const, savePATH=str(tmp_path) + "/", fec_metrics=fec).items():
        monkeypatch.setattr(ev, k, v)
    name, d = ev.main()
    m = io.loadmat(name)["dict"]
    assert set(d) == set(m.dtype.names)
    return d, m


def test_eval_run_shaping_vaele_fec_metrics(tmp_path, monkeypatch):
    from vae_equalizer_amd import Eval_run_shaping_vaele as ev
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    const = dict(mod="16-QAM", SNR_vec=[14], iter=2, num_epochs=4, N_valid=1000, train_len=700, base_seed=3)
    fec = _fec(5)                                                                 # w = 4, S = 186: 5 codewords behind t0 = 13
    d0, _ = _main(ev, tmp_path, monkeypatch, const, None)
    assert set(d0) == LE_KEYS
    d, m = _main(ev, tmp_path, monkeypatch, const, fec)
    assert set(d) == LE_KEYS | set(FEC_KEYS) and np.array_equal(d["SER"], d0["SER"]) and d["SER"].shape == (1, 1, 1, 1, 1, 1, 2, 2)
    runs = [dict(SNR=14, nu=0, lr_optim=5e-3, seed=3 + 1000 * i) for i in range(2)]
    r = run_awgn_batch(runs, "16-QAM", 2, 25, 350, 1000, 700, 4, 2, "h1", generator=None, seed=3, fec=fec)
    want = _want(r[2]["fec"])
    print("VAE-LE:", {k: d[k].ravel().tolist() for k in FEC_KEYS}, "runner", want.tolist())
    assert tuple(r[2]["fec"]["iters"].shape) == (2, 5) and torch.equal(r[0], torch.from_numpy(d["SER"]).reshape(2, 2))
    for j, k in enumerate(FEC_KEYS):
        assert d[k].shape == d["SER"].shape[:-1] and d[k].dtype == np.float32 and np.array_equal(d[k].ravel(), want[:, j]), k
        assert np.array_equal(np.asarray(m[k][0, 0]).ravel(), want[:, j]), k
    assert (d["BER_pre_fec"] > 0).all()                                           # there was something to decode
    d2, _ = _main(ev, tmp_path, monkeypatch, dict(const, info_metrics=True), fec)  # beside info_metrics: both sets of rows, each in its place
    assert set(d2) == LE_KEYS | set(FEC_KEYS) | set(ev.INFO_KEYS) and d2["GMI"].shape == d["SER"].shape
    assert all(np.array_equal(d2[k], d[k]) for k in FEC_KEYS + ("SER",))


@pytest.mark.parametrize("loss_type", ["VAE", "CMAflex"])
def test_eval_run_dp_fec_metrics(tmp_path, monkeypatch, loss_type):
    from vae_equalizer_amd import Eval_run_DP as ev
    from vae_equalizer_amd.dp_runs import DPRun
    lr = 2.5e-3 if loss_type == "VAE" else 1e-5
    const = dict(loss_type=loss_type, mod="16-QAM", SNR_vec=[12], lr_optim_vec=[lr], iter=2, num_frames=2, N_frame_max=400, base_seed=9)
    fec = _fec(2)                                                                 # w = 8, S = 93: 4 (VAE) or 3 (after the CMA's cut) codewords
    d0, _ = _main(ev, tmp_path, monkeypatch, const, None)
    assert set(d0) == DP_KEYS
    d, m = _main(ev, tmp_path, monkeypatch, const, fec)
    assert set(d) == DP_KEYS | set(FEC_KEYS) and np.array_equal(d["SER"], d0["SER"], equal_nan=True)
    runs = [DPRun(12, ev.nu_vec[0], ev.theta_diff_vec[0], ev.theta_vec[0], lr, ev.symb_rate_vec[0], 9 + 1000 * i) for i in range(2)]
    args = ("16-QAM", ev.sps, ev.M_vec[0], ev.batch_len_vec[0], 400, 2, ev.flex_step_vec[0], ev.channel, ev.tau_cd, ev.tau_pmd, ev.phiIQ, ev.N_lrhalf)
    if loss_type == "VAE":
        from vae_equalizer_amd.dp_runs import run_dp_batch
        r = run_dp_batch(runs, *args, flex=False, generator=None, verbose=False, fec=fec)
    else:
        from vae_equalizer_amd.cma_runs import run_cma_batch
        r = run_cma_batch(runs, loss_type, *args, generator=None, verbose=False, fec=fec)
    want = _want(r["fec"])
    print(f"{loss_type}:", {k: d[k].ravel().tolist() for k in FEC_KEYS}, "runner", want.tolist())
    assert r["fec"]["iters"].shape[1] == (4 if loss_type == "VAE" else 3)
    for j, k in enumerate(FEC_KEYS):
        assert d[k].shape == d["SER"].shape[1:-1] and d[k].dtype == np.float32 and np.array_equal(d[k].ravel(), want[:, j]), k
        assert np.array_equal(np.asarray(m[k][0, 0]).ravel(), want[:, j]), k
    assert (d["BER_pre_fec"] > 0).all()


@pytest.mark.parametrize("which", ["cma", "nn"])
def test_eval_run_cma_and_vaenn_fec_metrics(tmp_path, monkeypatch, which):
    """The two other AWGN scripts share the row packer: the schema, the shapes, and the old key set with fec_metrics = None."""
    import importlib
    ev = importlib.import_module("vae_equalizer_amd." + dict(cma="Eval_run_shaping_cma", nn="Eval_run_vaenn")[which])
    const = dict(cma=dict(mod="16-QAM", M_vec=[9], lr_optim_vec=[3e-4], SNR_vec=[12, 16], iter=2, N_valid=1100, train_len=600, num_epochs=4, base_seed=11),
                 nn=dict(mod="16-QAM", SNR_vec=[12, 16], iter=2, num_epochs=4, N_valid=1000, train_len=900, base_seed=3))[which]
    old = dict(cma={"SER", "SNR", "M", "lr", "nu"}, nn={"SER", "SNR", "k2", "k1", "M", "lr", "N_train"})[which]
    d0, _ = _main(ev, tmp_path, monkeypatch, const, None)
    assert set(d0) == old
    d, _ = _main(ev, tmp_path, monkeypatch, const, _fec(5))
    print(which, {k: d[k].ravel().tolist() for k in FEC_KEYS})
    assert set(d) == old | set(FEC_KEYS) and np.array_equal(d["SER"], d0["SER"], equal_nan=True) and d["SER"].shape[-2:] == (2, 2)
    for k in FEC_KEYS:
        assert d[k].shape == d["SER"].shape[:-1] and d[k].dtype == np.float32 and np.isfinite(d[k]).all(), k
    assert (d["BER_pre_fec"] > 0).all() and (d["FER"] <= 1).all() and (d["fec_iters"] <= 8).all()


def test_dfe_main_returns_the_fec_dicts(monkeypatch):
    from vae_equalizer_amd import DFE_MQAM_shaping as D
    for k, v in dict(SNR_vec=np.array([12, 16]), num_epochs=2, N_valid=1100, mod="16-QAM", base_seed=5).items():
        monkeypatch.setattr(D, k, v)
    plain = D.main()
    monkeypatch.setattr(D, "fec_metrics", _fec(5))
    out = D.main()
    assert len(plain) == 2 and len(out) == 4 and all(torch.equal(a, b) for a, b in zip(plain, out))
    for fec in out[2:]:
        assert tuple(fec["iters"].shape) == (2, 2, 5) and tuple(fec["BER_post"].shape) == (2, 2) and fec["iters"].is_cuda
    monkeypatch.setattr(D, "info_metrics", True)
    both = D.main()
    assert len(both) == 6 and all(torch.equal(both[4 + i][k], out[2 + i][k]) for i in range(2) for k in out[2])

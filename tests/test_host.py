"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol of include/vaeq.h, the host mirrors
keep the reference's call surface, the batched epilogue agrees with the oracle, product code never imports the oracle."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT, load_golden


def test_library_builds_and_exports_every_declared_symbol():
    from vae_equalizer_amd import _native as nat
    nat.build()
    L = nat.lib()
    header = open(os.path.join(ROOT, "include", "vaeq.h")).read()
    declared = set(re.findall(r"\b(vaeq_[a-z_0-9]+)\s*\(", header))
    assert declared == set(nat.EXPORTS), declared ^ set(nat.EXPORTS)
    for s in declared:
        assert hasattr(L, s), s
    assert L.vaeq_version() == 100
    assert L.vaeq_strerror(-2) == b"inconsistent or unsupported sizes"
    # shape validation is host-side: no GPU needed
    assert L.vaeq_dp_lds_bytes(100, 2, 25, 8) > 0
    assert L.vaeq_dp_lds_bytes(100, 2, 24, 8) == -2       # even M_est
    assert L.vaeq_dp_lds_bytes(100, 2, 25, 3) == -2       # levels
    assert L.vaeq_dp_lds_bytes(10, 2, 25, 8) == -2        # window shorter than the channel memory
    assert L.vaeq_awgn_lds_bytes(350, 2, 25, 8) > 0


def test_struct_mirrors_match_header_field_order():
    from vae_equalizer_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "vaeq.h")).read()
    for name, cls in (("vaeq_dp_args", nat.DPArgs), ("vaeq_awgn_args", nat.AWGNArgs), ("vaeq_nn_args", nat.NNArgs)):
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        fields = []
        for line in body.splitlines()[1:]:
            line = line.split("/*")[0].strip()
            if not line.endswith(";"):
                continue
            for part in line[:-1].split(","):
                fields.append(part.replace("*", " ").split()[-1])
        assert fields == [f[0] for f in cls._fields_], name


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "vae_equalizer_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), f


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.func_VAELE_DP_MQAM_shaping import processing
    with pytest.raises(nat.VaeqError):
        processing('64-QAM', 2, 23, 0, 25, 0.0, 0.3, 2.5e-3, 100, 1000, 1, 10, 'h0', 90e9, -26e-24, 3e-12,
                   np.array([0.03, 0.03], dtype=np.complex64), 170, verbose=False)


def test_processing_signatures_match_reference():
    from vae_equalizer_amd import func_VAEflex_DP_MQAM_shaping as fx
    from vae_equalizer_amd import func_VAELE_DP_MQAM_shaping as le
    from vae_equalizer_amd import func_VAELE_MQAM_shaping as aw
    pos = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos(le.processing) == ["mod", "sps", "SNR", "nu", "M_est", "theta_diff", "theta", "lr_optim", "batch_len", "N_frame_max",
                                  "num_frames", "flex_step", "channel", "symb_rate", "tau_cd", "tau_pmd", "phiIQ", "N_lrhalf"]
    assert pos(fx.processing) == ["mod", "sps", "SNR", "nu", "M_est", "theta_diff", "theta", "lr_optim", "batch_len", "N_train_max",
                                  "num_frames", "flex_step", "channel", "symb_rate", "tau_cd", "tau_pmd", "phiIQ", "N_lrhalf"]
    assert pos(aw.processing) == ["mod", "sps", "SNR", "nu", "M_est", "lr_optim", "batch_len", "N_valid", "N_train", "num_epochs", "epe", "channel"]
    from vae_equalizer_amd import func_VAENN_MQAM as nn_
    assert pos(nn_.processing) == ["mod", "sps", "SNR", "M_est", "kernel_1", "kernel_2", "lr_optim", "batch_len", "N_valid", "N_train",
                                   "num_epochs", "epe", "channel", "net_type"]                # func_VAENN_MQAM.py:215


def test_vaenn_tables_and_host_generator():
    """Constants of func_VAENN_MQAM.processing (:219-237) and the host restatement of its generate_data (:39-61): fixed noise level,
    uniform symbols, reference aligned at T + M - 1."""
    import torch
    from vae_equalizer_amd import channel as ch
    from vae_equalizer_amd import func_VAENN_MQAM as nn_
    t = nn_.vaenn_tables("16-QAM", "h1", 2)
    assert abs(np.mean(np.abs(t["constellation"]) ** 2) - 1) < 1e-12 and len(t["amps"]) == 4 and abs(np.linalg.norm(t["h_channel"]) - 1) < 1e-6
    rx, data = nn_.generate_data(4000, t["M_channel"], t["constellation"], 200.0, t["h_channel"], 2, "cpu", np.random.RandomState(3))
    assert rx.shape == (2, 8000) and data.shape == (2, 4000) and data.dtype == torch.float16
    # noiseless: rx is the zero-stuffed reference filtered by rrc * h (samples whose pulse support lies inside the reference)
    g = np.convolve(ch.rrcfir(8, 2, 0.1), t["h_channel"])
    up = np.zeros(2 * 3999 + 1, complex)
    up[::2] = data[0].numpy().astype(float) + 1j * data[1].numpy().astype(float)
    clean = np.convolve(up, g, mode="valid")
    o = 2 * (8 + t["M_channel"] - 1)
    got = (rx[0].numpy() + 1j * rx[1].numpy())[o:o + len(clean)]
    assert np.max(np.abs(got - clean[:len(got)])) < 3e-3                       # fp16 reference levels
    with pytest.raises(UnboundLocalError):
        nn_.vaenn_tables("16-QAM", "h7", 2)


def test_init_tables_bit_exact():
    from vae_equalizer_amd import shared_funcs as sfun
    g = load_golden("G0_init")
    for k in range(int(g["n_cases"])):
        mod, nu, SNR, ch, M = g[f"c{k}_args"]
        r = sfun.init(str(ch), str(mod), "cpu", float(nu), 2, int(M), float(SNR))
        for nm, v in zip(["h_est", "h_channel", "P", "amp_levels", "amps", None, "nu_sc", "var", "pow_mean"], r):
            if nm is None:
                assert v == 2
                continue
            v = v.detach().numpy() if hasattr(v, "detach") else np.asarray(v)
            assert np.array_equal(v, g[f"c{k}_{nm}"]), (k, nm)
    with pytest.raises(KeyError):
        sfun.init("h0", "8-QAM", "cpu", 0, 2, 25, 20)
    with pytest.raises(UnboundLocalError):
        sfun.init("h9", "4-QAM", "cpu", 0, 2, 25, 20)


def test_awgn_tables_match_capture():
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import awgn_tables
    g = load_golden("G4_awgn_64qam_pcs_free10")
    t = awgn_tables("64-QAM", float(g["nu"]), float(g["SNR"]), "h1", 2)
    assert np.allclose(t["amps"].astype(np.float32), g["amp_levels"]) and np.allclose(t["P"].astype(np.float32), g["P"])
    assert abs(t["amp_mean"] - float(g["amp_mean"])) < 1e-12 and abs(t["var"] - float(g["var"])) < 1e-15


def _epi_inputs(g):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return t(g["out_train"])[None], t(g["out_const"])[None], t(g["data"])[None], t(g["amp_levels"])


def test_batched_epilogue_matches_oracle_and_reference_on_converged_frame():
    """The torch epilogue (device-agnostic) on G5's converged frame == the reference's own results."""
    from vae_equalizer_amd import epilogue as epi
    g = load_golden("G5_dp_epilogue")
    q, y, data, amp = _epi_inputs(g)
    nu = torch.tensor([float(g["nu_sc"])]); var = torch.from_numpy(g["var"])[None]
    r = epi.dp_frame_epilogue(q, y, data, amp, nu, var, batch_len=int(g["B"]))
    assert np.array_equal(r["shift_q"][0].numpy(), g["shifts"][-1, 0]) and int(r["r_q"][0]) == g["rs"][-1, 0]
    assert np.array_equal(r["shift_c"][0].numpy(), g["shifts"][-1, 1]) and int(r["r_c"][0]) == g["rs"][-1, 1]
    assert np.allclose(r["SER"][0].numpy(), g["SER_valid"][:, -1], atol=1e-6)


@pytest.mark.parametrize("batch_len", [None, 100])
def test_batched_epilogue_random_batch_vs_oracle(batch_len):
    """R=6 synthetic runs with different delays / swaps / rotations: batched torch epilogue == per-run numpy oracle."""
    from vae_equalizer_amd import epilogue as epi
    g = load_golden("G5_dp_epilogue")
    amp, var0 = g["amp_levels"], g["var"]
    rng = np.random.default_rng(11)
    R, N, n = 6, 1000, amp.shape[0]
    qs, ys, ds, nus, vars_ = [], [], [], [], []
    for i in range(R):
        lev = rng.integers(0, n, (2, 2, N))
        clean = amp[lev].astype(np.float32)
        k = i % 4
        rot = [clean, np.stack([-clean[:, 1], clean[:, 0]], 1), -clean, np.stack([clean[:, 1], -clean[:, 0]], 1)][k]
        if i == 4:
            rot = np.stack([rot[:, 0], -rot[:, 1]], 1)          # conjugate (IQ flip)
        y = rot + (0.03 + 0.02 * i) * rng.standard_normal(rot.shape).astype(np.float32)
        sw, d = i % 2, int(rng.integers(-9, 10))
        y = np.roll(y, sw, axis=0)
        dl = (d, d) if sw else (d, int(rng.integers(-9, 10)))
        y = np.stack([np.roll(y[0], dl[0], -1), np.roll(y[1], dl[1], -1)])
        nu_sc = float(rng.uniform(0, 1.2)); v = (var0 * rng.uniform(0.5, 2)).astype(np.float32)
        qs.append(oracle.dp_soft_dec(y, v, amp, nu_sc)); ys.append(y); ds.append(amp[lev].astype(np.float16)); nus.append(nu_sc); vars_.append(v)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack(a)))
    r = epi.dp_frame_epilogue(t(qs), t(ys), t(ds), torch.from_numpy(amp), torch.tensor(nus, dtype=torch.float32), t(vars_), batch_len)
    for i in range(R):
        o = oracle.dp_frame_epilogue(qs[i], ys[i], ds[i], amp, nus[i], vars_[i], batch_len=batch_len)
        assert np.array_equal(r["shift_q"][i].numpy(), o["shift_q"]) and int(r["r_q"][i]) == o["r_q"], i
        assert np.array_equal(r["shift_c"][i].numpy(), o["shift_c"]) and int(r["r_c"][i]) == o["r_c"], i
        assert np.allclose(r["SER"][i].numpy(), o["SER"], atol=1e-6), (i, r["SER"][i], o["SER"])


def test_unbatched_mirrors_keep_reference_shapes():
    from vae_equalizer_amd import shared_funcs as sfun
    g = load_golden("G5_dp_epilogue")
    q, y, data, amp = (x[0] if x.dim() == 4 else x for x in _epi_inputs(g))
    shift, r = sfun.find_shift(q, data, 21, amp, 2)
    assert shift.dtype == torch.int16 and shift.shape == (2,) and r in (0, 1)
    shift2, r2 = sfun.find_shift_symb_full(y, data, 21)
    assert np.array_equal(shift.numpy(), g["shifts"][-1, 0]) and np.array_equal(shift2.numpy(), g["shifts"][-1, 1])
    o = oracle.SER_IQflip(g["out_train"][:, :, 11:-11], g["data"][:, :, 11:-11])
    assert np.allclose(sfun.SER_IQflip(q[:, :, 11:-11], data[:, :, 11:-11]).numpy(), o, atol=1e-7)
    yy = y[:, :, 11:-11].clone()
    o = oracle.SER_constell_shaping(g["out_const"][:, :, 11:-11].copy(), g["data"][:, :, 11:-11], g["amp_levels"], float(g["nu_sc"]), g["var"])
    s = sfun.SER_constell_shaping(yy, data[:, :, 11:-11], amp, float(g["nu_sc"]), torch.from_numpy(g["var"]))
    assert np.allclose(s.numpy(), o, atol=1e-7)
    assert not torch.equal(yy, y[:, :, 11:-11])       # rescaled in place like the reference (shared_funcs.py:242)


def test_host_threads_divide_by_local_world_size(monkeypatch):
    """under torch.distributed.run every rank takes its share of the host cores, not all of them."""
    from vae_equalizer_amd import dp_runs
    monkeypatch.delenv("VAEQ_CPU_THREADS", raising=False)
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    n1 = dp_runs.host_threads()
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "8")
    assert dp_runs.host_threads() == max(1, n1 // 8)
    monkeypatch.setenv("VAEQ_CPU_THREADS", "3")
    assert dp_runs.host_threads() == 3


def test_device_generators_refuse_mixed_symbol_rates():
    """the on-device simulators take one symbol rate per call; a mixed batch must not silently run at runs[0]'s rate."""
    from vae_equalizer_amd.dp_runs import DPRun, check_one_symb_rate
    runs = [DPRun(23, 0.0, 0.0, 0.3, 2.5e-3, 40e9), DPRun(23, 0.0, 0.0, 0.3, 2.5e-3, 90e9)]
    check_one_symb_rate(runs, "numpy")
    for g in ("hip", "torch"):
        with pytest.raises(ValueError, match="symb_rate"):
            check_one_symb_rate(runs, g)
    check_one_symb_rate(runs[:1] * 2, "hip")


def test_stream_seeds_differ_across_ranks_batches_and_unseeded_invocations():
    from vae_equalizer_amd import sweep
    s = {sweep.stream_seed(5, r, b) for r in range(8) for b in range(4)}
    assert len(s) == 32 and sweep.stream_seed(5, 1, 2) == sweep.stream_seed(5, 1, 2)
    assert sweep.stream_seed(None, 0, 0) != sweep.stream_seed(None, 0, 0)


def test_default_generator_follows_the_seed():
    """generator=None (the default of every entry point): unseeded runs -- the reference seeds nothing (shared_funcs.py:75,84) -- take the on-device channel
    simulator, seeded runs the reference-faithful host simulator; an explicit choice is never overridden.  The sweep scripts ship with generator = None."""
    from vae_equalizer_amd import Eval_run_DP, Eval_run_shaping_vaele
    from vae_equalizer_amd.dp_runs import resolve_generator
    assert resolve_generator(None, False) == "hip" and resolve_generator(None, True) == "numpy"
    assert resolve_generator("numpy", False) == "numpy" and resolve_generator("hip", True) == "hip" and resolve_generator("torch", False) == "torch"
    assert Eval_run_DP.generator is None and Eval_run_DP.base_seed is None and Eval_run_shaping_vaele.generator is None
    import inspect
    from vae_equalizer_amd import func_VAELE_DP_MQAM_shaping as f1, func_VAEflex_DP_MQAM_shaping as f2, func_VAELE_MQAM_shaping as f3
    for f in (f1, f2, f3):
        assert inspect.signature(f.processing).parameters["generator"].default is None


def test_padded_rows_prefer_the_librarys_own_fft_lengths():
    """channel.padded_row_len: the smallest N1 x 1024 row the three-pass generator covers (N1 in {4, 5, 8, 10, 16, 20}) whenever one fits -- frames up to
    ~10 200 symbols never need a hipFFT plan --, else the next {1, 3, 5} x 2^a length."""
    from vae_equalizer_amd import channel as ch
    assert [ch.padded_row_len(n) for n in (1, 2098, 4096, 4097, 6098, 10098, 12098, 16385, 20098, 20480)] == [4096, 4096, 4096, 5120, 8192, 10240, 16384, 20480, 20480, 20480]
    assert ch.padded_row_len(20481) == ch.fast_fft_len(20481) == 24576 and ch.padded_row_len(40098) == 40960
    assert ch.STREAM_BLOCK == 8192 and "chunk" not in ch.generate_batch_hip.__code__.co_varnames[:ch.generate_batch_hip.__code__.co_argcount]


def test_bench_dump_outputs_fixed_sample_within_64_mb(tmp_path):
    """bench.py --dump-outputs on host tensors shaped like a DP step's outputs: float32 .npy files, at most 64 MB in all, every run of the
    per-run arrays, a seeded sample of runs for q / y that is the same on every call and holds those runs' rows unchanged."""
    import types
    import bench
    R, n, N, M = 40, 8, 10000, 25
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    eng = types.SimpleNamespace(R=R, W=r(R, 2, 4, M), h=r(R, 2, 2, 2, M))
    out = {"loss": r(R, 1, 100), "var_est": r(R, 1, 2, 100), "q": r(R, 1, 2, 2 * n, N), "y": r(R, 1, 2, 2, N)}
    shapes = bench.dump_outputs(out, eng, str(tmp_path / "a"))
    bench.dump_outputs(out, eng, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["W.npy", "h.npy", "loss.npy", "q.npy", "var_est.npy", "y.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for k, v in a.items():
        assert v.dtype == np.float32 and list(v.shape) == shapes[k] and np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    for k in ("loss", "var_est"):
        assert np.array_equal(a[k], out[k].numpy())
    assert np.array_equal(a["W"], eng.W.numpy()) and np.array_equal(a["h"], eng.h.numpy())
    k = a["q"].shape[0]
    assert 1 <= k < R and a["y"].shape[0] == k
    rows = [i for i in range(R) if (out["y"][i].numpy() == a["y"]).all(axis=tuple(range(1, 5))).any()]
    assert len(rows) == k and np.array_equal(a["q"], out["q"][rows].numpy())

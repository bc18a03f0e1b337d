#!/usr/bin/env python3
"""Headline benchmark: equalized DP symbols/s on optical DP 64-QAM VAE-LE (BASELINE.json metric, SURVEY config 3).

One bench "step" = one frame of the reference's training loop (N_frame_max = 10 000 DP symbols = 100 minibatch steps of 100
symbols: FIR + soft demap + ELBO + backward + Adam each, optical_DP_channel/func_VAELE_DP_MQAM_shaping.py:57-66) for every one of the
R independent runs of this GPU's shard of the sweep -- ONE launch of the fused HIP kernel.  Config 3's own sweep is 3 learning rates x
iter=5 = 15 runs (Eval_run_DP.py:41,44), which cannot fill a 256-CU GPU; the workload keeps every other constant of config 3 and raises
the seed axis (``iter``) so that R runs per GPU saturate it (SURVEY 8d "saturation variant").  Received samples come from the on-device
channel simulator (synthetic, distinct per run and per frame) and are resident in HBM before the timed region starts.

What one invocation does (rank 0 prints ONE JSON line, contract in the task statement):
  1. parity gate (before anything is timed): the first runs are trained from the Dirac start on the GPU and by the CPU oracle on the same
     samples; per-step ELBO, taps and the epilogue's SER must agree (tolerances below) or the process exits non-zero -> ``parity``;
  2. W warm-up steps, then ONE timed region of EXACTLY K steps (barrier + synchronize on both sides, max over ranks); --min-seconds S > 0
     repeats the region until S seconds of timed GPU work have accumulated, and ``value`` is then the MEDIAN region (``timed_regions`` /
     ``region_ms`` say how many and how they spread); per-launch HIP-event times -> ``roofline`` (HBM and flop fractions, measured
     stream-copy bandwidth); --dump-outputs DIR writes what the last timed step returned (see dump_outputs);
  3. N = 1 only, all untimed for the headline: ``extra.pipeline`` (generate -> train -> epilogue per frame, compact mode),
     ``extra.configs`` (config 4 VAEflex and config 2 AWGN kernel rates), ``cpu_baseline`` (the C oracle on the host cores).

N > 1: one process per GPU (torch.distributed.run), each rank owns its own R runs (weak scaling, the sweep is embarrassingly parallel),
no data-path collective; the only communication is the all_gather of the per-run result rows, inside every timed region.

--config5: the same step on SURVEY config 5's saturation variant (Eval_run_DP.py:24,34: 4 nu x 5 SNR x 3 lr x iter 64 = 3840 runs with
per-run PCS tables / noise levels), a FIXED total sharded r mod N over the ranks: "scaling": "strong" (DESIGN.md section 6 states the expected curve).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ALGO_BYTES_PER_DP_SYMBOL = 176      # 32 B rx read + 128 B q write + 16 B out write (SURVEY 8d, 64-QAM, 2 sps)
HBM_PEAK_GBS = 8000.0               # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP32_PEAK_TFLOPS = 157.3            # MI355X fp32 vector peak (v_pk_fma_f32; the f32 MFMA peak is the same)
# Useful flops per DP symbol of a VAE-LE step at B = 100, M = 25, n = 8:
#   ALGO: complex MACs of the five convolution-shaped phases per 100-symbol step (FIR 2x2x25x100, D 2x2x13x176, dL/dh 100 taps x 88 terms,
#         dL/dU 2x2x25x100, dL/dw 100 taps x 100 symbols = 47 600 cMAC = 3808 flop/symbol) + soft demap / moments / dL/dy (~ 500 flop/symbol);
#   ISSUED: the 1970 v_pk_fma_f32 per wave-step the kernel spends on those phases x 64 lanes x 4 flop / 100 symbols (lane padding of a
#         100-symbol minibatch on 64-lane waves included) -- the figure round 1's verdict priced the kernel with (0.29 at 9.1 G symbols/s).
ALGO_FLOPS_PER_DP_SYMBOL = 4300.0
ISSUED_FMA_FLOPS_PER_DP_SYMBOL = 5043.0
REFERENCE_DP_SYMBOLS_PER_S = 2.17e3  # the reference itself (PyTorch CPU, 4 threads), measured in the survey container: BASELINE.md section 2
PARITY_TOL = 1e-5                    # north_star's bound: per-batch ELBO (relative) and taps (absolute) over the gate's free run
PARITY_STEPS = 10                    # free-running steps from the Dirac start.  fp32 chaos doubles the tap deviation every ~3-4 steps (measured, GPU vs
                                     # oracle over 256 runs, tools/probe_parity.py: 3e-6 at 10 steps, 2e-5 at 20, 1.3e-4 at 30; SURVEY section 7 shows the
                                     # same for the reference against itself), so 10 steps is where a 1e-5 gate still has a 3x margin

CFG = dict(mod="64-QAM", sps=2, nu=0.0, channel="h0", SNR=23.0, symb_rate=90e9, tau_cd=-26e-24, tau_pmd=0.1e-12 * np.sqrt(1000),
           phiIQ=np.array([0.0314, 0.0314], dtype=np.complex64), theta=np.pi / 10, theta_diff=0.06 * np.pi, M_est=25, batch_len=100,
           N_frame_max=10000, lr_optim_vec=[2.5e-3, 2e-3, 3e-3], flex_step=10)
CFG2 = dict(mod="64-QAM", nu=0.0270955, SNR=24.0, channel="h1", M_est=25, batch_len=350, train_len=1200, lr=5e-3)   # Eval_run_shaping_vaele.py:19-36


def make_frames(n_frames, R, device, seed, with_data=False):
    """rx for n_frames frames x R runs from the on-device channel simulator: list of [R,1,2,2,S] tensors (+ the TX reference of frame 0)."""
    from vae_equalizer_amd import channel as ch
    from vae_equalizer_amd import shared_funcs as sfun
    t = sfun.qam_tables(CFG["mod"], CFG["nu"])
    h_ch = sfun.upsampled_channel(CFG["channel"], CFG["sps"])
    frames, data0 = [], None
    for f in range(n_frames):       # HIP generator kernels (vaeq_gen_dp_frame, three-pass form), Philox streams keyed by (seed, frame, run)
        rx, data = ch.generate_batch_hip(R, CFG["N_frame_max"], t["amps"], t["P"], CFG["SNR"], h_ch, CFG["symb_rate"], CFG["sps"], CFG["tau_cd"],
                                         CFG["tau_pmd"], CFG["phiIQ"], CFG["theta"] + f * CFG["theta_diff"], device, seed, f)
        frames.append(rx.unsqueeze(1))
        if f == 0:
            data0 = data
    return (frames, t, data0) if with_data else (frames, t)


def config5_points(n_iter):
    """SURVEY config 5 (Eval_run_DP.py:24,34 comments x :41 x iter): the sweep script's own loop order flattened, one dict per run."""
    from vae_equalizer_amd import Eval_run_DP as ev
    saved = ev.nu_vec, ev.SNR_vec, ev.iter
    ev.nu_vec, ev.SNR_vec, ev.iter = [0, 0.0270955, 0.0872449, 0.1222578], [20, 22, 24, 26, 28], n_iter
    try:
        return [p for _, p in ev.sweep_points()]
    finally:
        ev.nu_vec, ev.SNR_vec, ev.iter = saved


def make_frames_config5(n_frames, pts, device, seed):
    """rx of n_frames frames for the runs ``pts`` (per-run PCS tables and SNR) -> (frames, amps, P[R,n], var[R,2], nu_sc[R], lr[R])."""
    from vae_equalizer_amd import channel as ch
    from vae_equalizer_amd import shared_funcs as sfun
    tabs = [sfun.qam_tables(CFG["mod"], p["nu"]) for p in pts]
    h_ch = sfun.upsampled_channel(CFG["channel"], CFG["sps"])
    R = len(pts)
    P = np.stack([t["P"] for t in tabs]).astype(np.float32)
    snr = np.array([p["SNR"] for p in pts], np.float32)
    var = np.stack([np.full(2, t["pow_mean"] / 10 ** (p["SNR"] / 10) / 2) for t, p in zip(tabs, pts)]).astype(np.float32)
    nu_sc = np.array([t["nu_sc"] for t in tabs], np.float32)
    lr = np.array([p["lr_optim"] for p in pts], np.float32)
    frames = []
    for f in range(n_frames):
        theta = np.array([p["theta"] + f * p["theta_diff"] for p in pts])
        rx, _ = ch.generate_batch_hip(R, CFG["N_frame_max"], tabs[0]["amps"], P, snr, h_ch, CFG["symb_rate"], CFG["sps"], CFG["tau_cd"], CFG["tau_pmd"],
                                      CFG["phiIQ"], theta, device, seed, f)
        frames.append(rx.unsqueeze(1))
    return frames, tabs[0]["amps"], P, var, nu_sc, lr


def host_cores():
    """CPU cores this process may actually use: affinity mask, capped by the cgroup CPU quota (a 1-GPU box of the pool
    owns 16 of the host's cores) -- never os.cpu_count() of the whole host."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    if os.environ.get("VAEQ_CPU_THREADS"):
        n = int(os.environ["VAEQ_CPU_THREADS"])
    return min(n, 16) if n > 64 else n


def _oracle_state(Rc, M):
    W = np.zeros((Rc, 2, 4, M), np.float32)
    h = np.zeros((Rc, 2, 2, 2, M), np.float32)
    W[:, 0, 0, M // 2] = W[:, 1, 1, M // 2] = 1
    h[:, 0, 0, 0, M // 2] = h[:, 1, 1, 0, M // 2] = 1
    return W, h, np.zeros_like(W), np.zeros_like(W), np.zeros_like(h), np.zeros_like(h), np.zeros(Rc, np.int32)


def _oracle_train(rx, t, var, lr, steps, cores):
    """The C oracle (fp32, OpenMP over runs) on rx[Rc,2,2,S] from the Dirac start -> dict(loss[Rc,steps], W, h, q, y, threads)."""
    import oracle
    Rc = rx.shape[0]
    M, B, sps, n = CFG["M_est"], CFG["batch_len"], CFG["sps"], len(t["amps"])
    W, h, mW, vW, mh, vh, step = _oracle_state(Rc, M)
    amp = t["amps"].astype(np.float32)
    P = np.tile(t["P"].astype(np.float32), (Rc, 1))
    varr = np.full((Rc, 2), var, np.float32)
    nu = np.full(Rc, t["nu_sc"], np.float32)
    lrs = np.asarray(lr[:Rc], np.float32)
    q = np.zeros((Rc, 2, 2 * n, steps * B), np.float32)
    y = np.zeros((Rc, 2, 2, steps * B), np.float32)
    loss, ve = np.zeros((Rc, steps), np.float32), np.zeros((Rc, 2, steps), np.float32)
    used = oracle.dp_train_batch_f32(Rc, cores, steps, B, sps, M, n, B, 0, B, np.ascontiguousarray(rx), W, h, mW, vW, mh, vh, step, amp, P, varr,
                                     nu, lrs, lrs, q, y, loss, ve)
    return dict(loss=loss, W=W, h=h, q=q, y=y, threads=int(used), state=(W, h, mW, vW, mh, vh, step), tabs=(amp, P, varr, nu, lrs))


def parity_gate(frame_rx, data0, t, var, lr, device, threads):
    """SER/ELBO/tap match vs the CPU oracle on the bench's own samples, before anything is timed (parity with every timing).

    The first Rc runs train PARITY_STEPS free-running minibatch steps from the Dirac start on the GPU (the product path, through the C ABI) and
    in the oracle; gate: every step's ELBO <= PARITY_TOL relative, taps after the last step <= PARITY_TOL absolute, the epilogue's four SER
    estimates of the equalised block <= 2e-3 absolute.  20 steps and the whole 100-step frame are compared too, as information only: free runs
    that long are chaotic in fp32 (the reference itself differs by 2.6e-2 in W between 1 and 4 CPU threads after 100 steps)."""
    import oracle
    from vae_equalizer_amd.engine import DPEngine, dp_epilogue
    B, M, sps = CFG["batch_len"], CFG["M_est"], CFG["sps"]
    Rc = int(min(frame_rx.shape[0], 64))
    steps_frame = CFG["N_frame_max"] // B
    cores = host_cores()
    rx_dev = frame_rx[:Rc].contiguous()
    rx_np = rx_dev[:, 0].cpu().numpy()
    res = {}
    for tag, steps in (("gate", PARITY_STEPS), ("s20", 20), ("frame", steps_frame)):
        eng = DPEngine(Rc, M, t["amps"], t["P"], [var, var], t["nu_sc"], device, sps, threads)
        lr_t = torch.tensor(lr[:Rc], device=device)
        g = eng.train(rx_dev, B, steps, lr_t, want_q=(tag == "gate"))
        torch.cuda.synchronize()
        o = _oracle_train(rx_np[..., :steps * B * sps], t, var, lr, steps, cores)
        gl = g["loss"][:, 0].cpu().numpy()
        res[tag] = dict(loss_rel=float(np.max(np.abs(gl - o["loss"]) / np.abs(o["loss"]))),
                        taps_abs=float(max(np.max(np.abs(eng.W.cpu().numpy() - o["W"])), np.max(np.abs(eng.h.cpu().numpy() - o["h"])))))
        if tag == "gate":
            ne = min(Rc, 8)
            amp_t = torch.tensor(t["amps"], dtype=torch.float32, device=device)
            nu_t = torch.full((ne,), float(t["nu_sc"]), device=device)
            var_t = torch.full((ne, 2), float(var), device=device)
            N = steps * B
            ser_g = dp_epilogue(g["q"][:ne, 0].contiguous(), g["y"][:ne, 0].contiguous(), data0[:ne, :, :, :N].contiguous(), amp_t, nu_t, var_t, B)["SER"].cpu().numpy()
            dn = data0[:ne, :, :, :N].cpu().numpy()
            ser_o = np.stack([oracle.dp_frame_epilogue(o["q"][i], o["y"][i], dn[i], t["amps"].astype(np.float32), float(t["nu_sc"]),
                                                       np.full(2, var, np.float32), B)["SER"] for i in range(ne)])
            res[tag]["ser_abs"] = float(np.max(np.abs(ser_g - ser_o)))
            res[tag]["ser_mean"] = float(ser_o.mean())
    gt = res["gate"]
    ok = bool(np.isfinite([gt["loss_rel"], gt["taps_abs"], gt["ser_abs"]]).all() and gt["loss_rel"] <= PARITY_TOL and gt["taps_abs"] <= PARITY_TOL
              and gt["ser_abs"] <= 2e-3)
    return {"ok": ok, "against": "oracle/ (C restatement of the reference, fp32, pinned by tests/golden)", "runs": Rc, "steps": PARITY_STEPS,
            "elbo_rel_max": gt["loss_rel"], "taps_abs_max": gt["taps_abs"], "tol": PARITY_TOL, "ser_abs_max": gt["ser_abs"], "ser_tol": 2e-3,
            "ser_level": gt["ser_mean"],
            "informational_not_gated": {"20_steps": {"elbo_rel_max": res["s20"]["loss_rel"], "taps_abs_max": res["s20"]["taps_abs"]},
                                        "full_frame_100_steps": {"elbo_rel_max": res["frame"]["loss_rel"], "taps_abs_max": res["frame"]["taps_abs"]},
                                        "note": "free runs past the chaotic horizon (SURVEY section 7)"}}


def cpu_baseline(frame_rx, t, var, lr, target_s, threads, note=""):
    """The C oracle (oracle/, a port of the reference's step) on the host cores, OpenMP over runs, on a bounded sample of
    the same workload: the first `Rc` runs of the first frame, trained repeatedly until ~target_s of wall time."""
    import oracle
    cores = threads or host_cores()
    Rc = min(frame_rx.shape[0], 8 * cores)
    rx = np.ascontiguousarray(frame_rx[:Rc, 0].cpu().numpy())
    M, B, sps, n = CFG["M_est"], CFG["batch_len"], CFG["sps"], len(t["amps"])
    steps = CFG["N_frame_max"] // B
    W, h, mW, vW, mh, vh, step = _oracle_state(Rc, M)
    amp = t["amps"].astype(np.float32)
    P = np.tile(t["P"].astype(np.float32), (Rc, 1))
    varr = np.full((Rc, 2), var, np.float32)
    nu = np.full(Rc, t["nu_sc"], np.float32)
    lrs = np.asarray(lr[:Rc], np.float32)
    q = np.zeros((Rc, 2, 2 * n, steps * B), np.float32)
    y = np.zeros((Rc, 2, 2, steps * B), np.float32)
    loss, ve = np.zeros((Rc, steps), np.float32), np.zeros((Rc, 2, steps), np.float32)
    done, t0, used = 0, time.perf_counter(), cores
    while True:
        used = oracle.dp_train_batch_f32(Rc, cores, steps, B, sps, M, n, B, 0, B, rx, W, h, mW, vW, mh, vh, step, amp, P, varr, nu, lrs,
                                         lrs, q, y, loss, ve)
        done += 1
        el = time.perf_counter() - t0
        if el >= target_s or done >= 200:
            break
    sym = done * Rc * steps * B
    return {"value": sym / el, "unit": "DP-symbols/s", "cores": int(used), "kind": "port",
            "sample": f"{Rc} runs x {done} frame(s) x {steps * B} DP symbols of the same config, fp32 C oracle with OpenMP over runs, "
                      f"{el:.1f} s wall; per core {sym / el / used:.0f} DP-symbols/s. The reference itself (PyTorch, CPU-only by construction, "
                      f"func_VAELE_DP_MQAM_shaping.py:18) ran {REFERENCE_DP_SYMBOLS_PER_S:.0f} DP-symbols/s on 4 threads in the survey container "
                      "(BASELINE.md section 2); it cannot travel to the GPU box" + note,
            "reference_dp_symbols_per_s": REFERENCE_DP_SYMBOLS_PER_S}


DUMP_BYTES_PER_GROUP = 32 << 20       # --dump-outputs: the per-run result arrays and the per-symbol arrays get 32 MB each (64 MB in all)


def dump_outputs(out, eng, directory):
    """What the last timed step handed its caller, as float32 .npy files: loss [r,1,steps], var_est [r,1,2,steps] and the trained taps W [r,2,4,M],
    h [r,2,2,2,M] for every run (a fixed seeded sample of runs beyond 32 MB), q [r',1,2,2n,N] and y [r',1,2,2,N] for a fixed seeded sample of runs.
    The samples depend only on the run count, so two builds run with the same arguments write the same runs."""
    os.makedirs(directory, exist_ok=True)
    R = eng.R
    per_run = {"loss": out["loss"], "var_est": out["var_est"], "W": eng.W, "h": eng.h}
    per_symbol = {"q": out["q"], "y": out["y"]}
    written = {}
    for group in (per_run, per_symbol):
        run_bytes = sum(t[0].numel() * t.element_size() for t in group.values())
        n = max(1, min(R, DUMP_BYTES_PER_GROUP // run_bytes))
        runs = np.arange(R) if n == R else np.sort(np.random.default_rng(0).choice(R, n, replace=False))
        idx = torch.from_numpy(runs).to(eng.W.device)
        for name, t in group.items():
            a = t.index_select(0, idx).cpu().numpy().astype(np.float32, copy=False)
            np.save(os.path.join(directory, name + ".npy"), a)
            written[name] = list(a.shape)
    return written


def _event_ms(fn, n):
    """n launches of fn() on the current stream, each bracketed by HIP events -> list of ms."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def stream_copy_gbs(device, nbytes=4 << 30):
    """Measured HBM copy bandwidth (read + write bytes per second) of a plain 16-byte grid-stride copy kernel (vaeq_stream_copy)."""
    from vae_equalizer_amd import _native as nat
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=device).normal_()
    dst = torch.empty_like(src)

    def go():
        nat.check(nat.lib().vaeq_stream_copy(nat.ptr(dst), nat.ptr(src), nbytes, nat.current_stream(device)), "vaeq_stream_copy")
    go()
    ms = float(np.median(_event_ms(go, 5)))
    return 2 * nbytes / (ms * 1e-3) / 1e9


def extra_pipeline(R, t, var, device, frames=4):
    """What a sweep spends per frame: channel simulator -> training kernel (compact outputs, q not materialised) -> epilogue, back to back on
    one stream, timed as a whole with HIP events (the per-frame SER row is what leaves the device)."""
    from vae_equalizer_amd import channel as ch
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.engine import DPEngine, dp_epilogue_compact
    B, M, sps = CFG["batch_len"], CFG["M_est"], CFG["sps"]
    h_ch = sfun.upsampled_channel(CFG["channel"], sps)
    eng = DPEngine(R, M, t["amps"], t["P"], [var, var], t["nu_sc"], device, sps)
    amp = torch.tensor(t["amps"], dtype=torch.float32, device=device)
    nu = torch.full((R,), float(t["nu_sc"]), device=device)
    varr = torch.full((R, 2), float(var), device=device)
    state = {"f": 0}

    def frame(ev=None):
        f = state["f"]
        if ev:
            ev[0].record()
        rx, data = ch.generate_batch_hip(R, CFG["N_frame_max"], t["amps"], t["P"], CFG["SNR"], h_ch, CFG["symb_rate"], sps, CFG["tau_cd"], CFG["tau_pmd"],
                                         CFG["phiIQ"], CFG["theta"] + f * CFG["theta_diff"], device, 77, f)
        if ev:
            ev[1].record()
        out = eng.train(rx, B, CFG["N_frame_max"] // B, 2.5e-3, want_q=False, want_compact=True)
        if ev:
            ev[2].record()
        state["ser"] = dp_epilogue_compact(out["eq"][:, 0], out["dec"][:, 0], out["y"][:, 0], data, amp, nu, varr, B)["SER"]
        if ev:
            ev[3].record()
        state["f"] = f + 1
    frame()
    ms = float(np.median(_event_ms(frame, frames)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]          # one more frame with an event after every stage (same stream, no host waits)
    frame(ev)
    torch.cuda.synchronize()
    stage = {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(("generate", "train", "epilogue"))}
    return {"ms_per_frame": ms, "dp_symbols_per_s": R * CFG["N_frame_max"] / (ms * 1e-3), "runs": R, "stage_ms": stage,
            "stages": "vaeq_gen_dp_frame (three passes, own split FFT) -> vaeq_dp_train (eq_out/dec_out, q not materialised) -> vaeq_dp_epilogue_compact, one stream, "
                      "back to back"}


def extra_pipeline_small(device, runs=300, frames=40):
    """The script-faithful config-5 grid size (4 nu x 5 SNR x 3 lr x iter 5 = 300 runs, Eval_run_DP.py:24,34,41,44) through run_dp_batch itself -- what
    Eval_run_DP.main() spends per frame: below the resident-run count the three stages of a frame run on three streams (channel model of frame f + 1
    and epilogue of frame f - 1 beside the training launch of frame f, bit-identical results); the serial order is timed beside it."""
    from vae_equalizer_amd.dp_runs import DPRun, run_dp_batch
    NU, SNR = [0, 0.0270955, 0.0872449, 0.1222578], [20, 22, 24, 26, 28]
    pts = [DPRun(s, nu, CFG["theta_diff"], CFG["theta"], lr, CFG["symb_rate"]) for nu in NU for lr in CFG["lr_optim_vec"] for s in SNR for _ in range(5)][:runs]
    out = {"runs": len(pts), "frames": frames}
    for key, serial in (("ms_per_frame", False), ("ms_per_frame_serial", True)):
        if serial:
            os.environ["VAEQ_SERIAL_FRAMES"] = "1"
        try:
            run_dp_batch(pts, CFG["mod"], CFG["sps"], CFG["M_est"], CFG["batch_len"], CFG["N_frame_max"], 3, CFG["flex_step"], CFG["channel"], CFG["tau_cd"],
                         CFG["tau_pmd"], CFG["phiIQ"], 170, device=device)                                     # warm-up: tables, allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_dp_batch(pts, CFG["mod"], CFG["sps"], CFG["M_est"], CFG["batch_len"], CFG["N_frame_max"], frames, CFG["flex_step"], CFG["channel"],
                         CFG["tau_cd"], CFG["tau_pmd"], CFG["phiIQ"], 170, device=device)
            torch.cuda.synchronize()
            out[key] = (time.perf_counter() - t0) / frames * 1e3
        finally:
            os.environ.pop("VAEQ_SERIAL_FRAMES", None)
    out["dp_symbols_per_s"] = len(pts) * CFG["N_frame_max"] / (out["ms_per_frame"] * 1e-3)
    out["stages"] = "run_dp_batch: vaeq_gen_dp_frame | vaeq_dp_train | vaeq_dp_epilogue_compact on three streams (wall time per frame incl. the host side); serial order beside it"
    return out


def extra_configs(R, t, var, frame_rx, device):
    """Kernel-level rates of BASELINE configs 4 (VAEflex) and 2 (AWGN 64-QAM + PCS) from the same invocation."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd import shared_funcs as sfun
    from vae_equalizer_amd.engine import AWGNEngine, DPEngine
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import awgn_tables
    out = {}
    # config 4: VAEflex, window 100 symbols, stride 10, the centre 10 outputs kept (func_VAEflex_DP_MQAM_shaping.py:59-70): 990 steps per frame
    B, M, sps, fs = CFG["batch_len"], CFG["M_est"], CFG["sps"], CFG["flex_step"]
    N_out = (CFG["N_frame_max"] - B) // fs * fs
    steps = N_out // fs
    Rf = R
    eng = DPEngine(Rf, M, t["amps"], t["P"], [var, var], t["nu_sc"], device, sps)
    rx = frame_rx[:Rf]

    def flex():
        eng.train(rx, B, steps, 2.5e-3, stride=fs, keep_off=(B - fs) // 2, keep_len=fs)
    flex()
    name = nat.last_kernel()
    ms = float(np.median(_event_ms(flex, 3)))
    rate = Rf * N_out / (ms * 1e-3)
    flops = Rf * steps * B * ISSUED_FMA_FLOPS_PER_DP_SYMBOL / (ms * 1e-3)          # every window step costs a full 100-symbol VAE-LE step
    out["config4_vaeflex"] = {"workload": f"optical DP 64-QAM VAEflex, batch_len {B}, flex_step {fs}: {steps} window steps per 10 000-symbol frame, {Rf} runs",
                              "kernel": name, "kernel_ms": ms, "value": rate, "unit": "output DP-symbols/s", "window_steps_per_s": Rf * steps / (ms * 1e-3),
                              "hbm_gbs": ALGO_BYTES_PER_DP_SYMBOL * rate / 1e9, "hbm_frac": ALGO_BYTES_PER_DP_SYMBOL * rate / 1e9 / HBM_PEAK_GBS,
                              "flop_frac": flops / 1e12 / FP32_PEAK_TFLOPS}
    del eng
    # config 2: AWGN 64-QAM + PCS, B = 350, M = 25 (Eval_run_shaping_vaele.py:19-36): 3 steps per 1200-symbol epoch; 10 epochs' worth per launch
    c = CFG2
    ta = awgn_tables(c["mod"], c["nu"], c["SNR"], c["channel"], 2)
    Ba, stepsA = c["batch_len"], 10 * (c["train_len"] // c["batch_len"])
    Ra = R
    rxa = 0.4 * torch.randn(Ra, 2, stepsA * Ba * 2, device=device)
    enga = AWGNEngine(Ra, c["M_est"], ta["amps"], ta["P"], ta["amp_mean"], ta["var"], device, 2)

    def awgn():
        enga.train(rxa, Ba, stepsA, c["lr"])
    awgn()
    name = nat.last_kernel()
    ms = float(np.median(_event_ms(awgn, 3)))
    rate = Ra * stepsA * Ba / (ms * 1e-3)
    nm = 2 * Ba - 2 * (c["M_est"] // 2)
    cmac = c["M_est"] * Ba + 13 * nm + c["M_est"] * (nm // 2) + c["M_est"] * Ba + c["M_est"] * Ba      # FIR, D, dL/dh, dL/dU, dL/dw per step
    flop_sym = (8 * cmac + 250 * Ba) / Ba                                                               # + demap / moments per symbol
    # the same config as a sweep spends it, per epoch (func_VAELE_MQAM_shaping.py:291-322): generate 1200 training symbols, 3 minibatch steps, and -- on the
    # evaluated epochs (every epe-th) -- generate N_valid = 15 000 symbols and run the fused validation pass, the way run_awgn_batch does it: the
    # validation frame is generated clean and its noise added while the validation kernel stages it (vaeq_gen_awgn_clean -> vaeq_awgn_validate_gen)
    from vae_equalizer_amd import channel as ch
    snr = np.full(Ra, c["SNR"], np.float32)
    stepsE = c["train_len"] // Ba
    st = {}

    def epoch_train():
        rx, _ = ch.generate_awgn_batch_hip(Ra, c["train_len"], ta["amps"], ta["P"], snr, ta["h_channel"], 2, device, 3, 0)
        enga.train(rx, Ba, stepsE, c["lr"])

    def epoch_valid():
        st["ser"] = enga.validate_clean(ch.generate_awgn_clean_batch_hip(Ra, 15000, ta["amps"], ta["P"], snr, ta["h_channel"], 2, device, 3, 1), 21)

    def epoch_valid_two_step():
        rxv, dv = ch.generate_awgn_batch_hip(Ra, 15000, ta["amps"], ta["P"], snr, ta["h_channel"], 2, device, 3, 1)
        st["ser2"] = enga.validate(rxv, dv, 21)
    epoch_train(); epoch_valid(); epoch_valid_two_step()
    ms_t, ms_v = float(np.median(_event_ms(epoch_train, 5))), float(np.median(_event_ms(epoch_valid, 3)))
    ms_v2 = float(np.median(_event_ms(epoch_valid_two_step, 3)))
    epoch = {"ms_train_part": ms_t, "ms_validation_part": ms_v, "ms_validation_part_two_step": ms_v2, "ms_per_epoch_epe2": ms_t + 0.5 * ms_v,
             "run_epochs_per_s_epe2": Ra / ((ms_t + 0.5 * ms_v) * 1e-3), "validation_forms_agree_bitwise": bool(torch.equal(st["ser"][0], st["ser2"][0])),
             "stages": "vaeq_gen_awgn(1200) -> vaeq_awgn_train(3 x 350); every 2nd epoch (epe = 2) vaeq_gen_awgn_clean(15000) -> vaeq_awgn_validate_gen "
                       "(noise added while the frame is read; two_step = vaeq_gen_awgn(15000) -> vaeq_awgn_validate)"}
    out["config2_awgn"] = {"workload": f"AWGN 64-QAM + PCS (nu {c['nu']}), batch_len {Ba}, M_est {c['M_est']}: {stepsA} minibatch steps per launch, {Ra} runs "
                                       "(training loop; q is not materialised, like the reference)",
                           "kernel": name, "kernel_ms": ms, "value": rate, "unit": "symbols/s", "hbm_gbs": 16 * rate / 1e9, "hbm_frac": 16 * rate / 1e9 / HBM_PEAK_GBS,
                           "flop_frac": flop_sym * rate / 1e12 / FP32_PEAK_TFLOPS, "algorithmic_flops_per_symbol": flop_sym, "epoch_pipeline": epoch}
    # row f3 (AWGN VAE-NN, AWGN_channel/func_VAENN_MQAM.py): the sweep script's shape (Eval_run_vaenn.py:25-28: 64-QAM, batch_len 300, M_est 25, kernel sizes 25 / 3),
    # one training launch of an epoch (13 minibatch steps of train_len 4000) and the fused validation pass on 15 000 symbols, 2048 runs.  flops: the three GEMM-shaped
    # passes of each convolution (forward, input gradient, weight gradient), 2 per multiply-add -- what tools/probe_nn.py and DESIGN.md quote
    from vae_equalizer_amd.engine import NNEngine
    from vae_equalizer_amd.func_VAENN_MQAM import vaenn_tables
    tn = vaenn_tables("64-QAM", "h1", 2)
    Rn, Bn, stepsN, Nv = 2048, 300, 13, 15000
    engn = NNEngine(Rn, 25, 25, 3, tn["amps"], device, 2)
    engn.init_parameters()
    sig = np.full(Rn, np.sqrt(0.5) / 10 ** (24 / 20), np.float32)
    Pn = np.full(len(tn["amps"]), 1 / len(tn["amps"]))
    rxn, _ = ch.generate_awgn_batch_hip(Rn, 4000, tn["amps"], Pn, 24.0, tn["h_channel"], 2, device, 1, 0, sigma_fixed=sig)
    rxv, dv = ch.generate_awgn_batch_hip(Rn, Nv, tn["amps"], Pn, 24.0, tn["h_channel"], 2, device, 1, 1, sigma_fixed=sig)

    def nn_train():
        engn.train(rxn, Bn, stepsN, 4e-3)

    def nn_valid():
        engn.validate(rxv, dv, 21)
    nn_train(); nn_valid()
    ms_nt, ms_nv = float(np.median(_event_ms(nn_train, 5))), float(np.median(_event_ms(nn_valid, 3)))
    macs_step = 600 * 16 * 50 * 3 + 300 * 16 * 48 * 3
    out["vaenn_f3"] = {"workload": f"AWGN VAE-NN `Net`, 64-QAM, batch_len {Bn}, M_est 25, kernel sizes 25 / 3: {stepsN} minibatch steps per launch, {Rn} runs; validation on {Nv} symbols",
                       "train_ms_per_launch": ms_nt, "us_per_run_step": ms_nt * 1e3 / stepsN / (Rn / 256.0), "value": Rn * stepsN * Bn / (ms_nt * 1e-3), "unit": "symbols/s",
                       "tflops": 2 * Rn * stepsN * macs_step / (ms_nt * 1e-3) / 1e12, "flop_frac": 2 * Rn * stepsN * macs_step / (ms_nt * 1e-3) / 1e12 / FP32_PEAK_TFLOPS,
                       "validate_ms": ms_nv, "validate_tflops": 2 * Rn * Nv * (2 * 16 * 50 + 16 * 48) / (ms_nv * 1e-3) / 1e12}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=0, help="independent runs per GPU (one workgroup each); 0 = 4 x the number of runs "
                    "the device keeps co-resident (vaeq_dp_resident_runs), i.e. four full rounds, no ragged tail")
    ap.add_argument("--threads", type=int, default=0, help="workgroup size per run (0 = library default)")
    ap.add_argument("--min-seconds", type=float, default=0.0, help="repeat the K-step timed region until this much timed GPU work has accumulated "
                    "(0 = one region: exactly --steps timed steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one returned (rank 0's runs) as DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip extra.pipeline / extra.configs / the stream-copy calibration")
    ap.add_argument("--no-parity", action="store_true", help="skip the parity gate (profiling runs only)")
    ap.add_argument("--distinct-frames", type=int, default=4, help="distinct synthetic frames cycled through the steps")
    ap.add_argument("--config5", action="store_true", help="strong scaling: SURVEY config 5's saturation variant (4 nu x 5 SNR x 3 lr x --iter seeds), "
                    "a fixed total sharded r mod N over the ranks, one gather of the result rows")
    ap.add_argument("--iter", type=int, default=64, help="--config5: seeds per sweep point (script default 5 -> 300 runs; 64 -> 3840 runs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.min_seconds > 0:              # repeated regions train on for a time-dependent number of steps
        ap.error("--dump-outputs needs a fixed number of timed steps: leave --min-seconds at 0")

    from vae_equalizer_amd import sweep
    from vae_equalizer_amd.engine import DPEngine
    rank, world, local_rank = sweep.init_distributed(os.environ.get("VAEQ_DIST_BACKEND"))   # default nccl (= RCCL); gloo only to
    if os.environ.get("VAEQ_BENCH_SINGLE_DEVICE"):                                          # rehearse N > 1 on a one-GPU box
        local_rank = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    import torch.distributed as dist
    collective = dist.is_available() and dist.is_initialized()   # N > 1, or N = 1 under VAEQ_FORCE_COLLECTIVE=1 (RCCL exercised on one GPU)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    K, Wm = args.steps, args.warmup
    B, M, sps = CFG["batch_len"], CFG["M_est"], CFG["sps"]
    from vae_equalizer_amd import _native as nat
    resident = int(nat.lib().vaeq_dp_resident_runs(B, sps, M, 8, args.threads))
    if resident <= 0:
        raise SystemExit(f"vaeq_dp_resident_runs failed: {resident}")
    steps_per_frame = CFG["N_frame_max"] // B
    n_distinct = max(1, min(args.distinct_frames, K + Wm))
    from vae_equalizer_amd import shared_funcs as sfun
    t = sfun.qam_tables(CFG["mod"], CFG["nu"])
    var = t["pow_mean"] / 10 ** (CFG["SNR"] / 10) / 2
    if args.config5:
        pts = config5_points(args.iter)
        R_total = len(pts)
        mine = sweep.my_slice(R_total, rank, world)
        R = len(mine)
        frames, amps5, P5, var5, nu5, lr = make_frames_config5(n_distinct, [pts[i] for i in mine], device, seed=1000 + rank)
        eng_args = (R, M, amps5, P5, var5, nu5, device, sps, args.threads)
    else:
        R = args.runs if args.runs > 0 else 4 * resident
        R_total = world * R
        frames, _t = make_frames(n_distinct, R, device, seed=1000 + rank)
        lr = np.array([CFG["lr_optim_vec"][(rank * R + i) % 3] for i in range(R)], np.float32)     # the sweep's lr axis
        eng_args = (R, M, t["amps"], t["P"], [var, var], t["nu_sc"], device, sps, args.threads)

    parity = None
    if rank == 0 and not args.no_parity:
        if args.config5:                                       # the gate's runs: config 3's constants (the config-5 points are pinned by tests/golden G10, G13)
            gframes, _t, data0 = make_frames(1, 64, device, seed=1000, with_data=True)
            glr = np.array([CFG["lr_optim_vec"][i % 3] for i in range(64)], np.float32)
        else:
            gframes, _t, data0 = make_frames(1, min(R, 64), device, seed=1000 + rank, with_data=True)   # = the first runs of frames[0]
            glr = lr
        parity = parity_gate(gframes[0], data0, t, var, glr, device, args.threads)
        del gframes, data0
        if not parity["ok"]:
            print(json.dumps({"metric": "equalized symbols/s/GPU, DP 64-QAM VAE-LE", "value": None, "parity": parity,
                              "error": "parity gate failed: the HIP path disagrees with the CPU oracle; nothing was timed"}), flush=True)
            sys.exit(3)

    eng = DPEngine(*eng_args)
    lr_t = torch.tensor(lr, device=device)

    def one_step(k):
        return eng.train(frames[k % n_distinct], B, steps_per_frame, lr_t)

    # allocator priming (untimed setup, not a warm-up step of the metric): two sets of output buffers are alive at the hand-over
    # `out = one_step(...)`, so both are put into the caching allocator now and no hipMalloc lands in the timed region even for W <= 1
    _prime = [torch.empty(R, 1, 2, c, steps_per_frame * B, dtype=torch.float32, device=device) for c in (16, 16, 2, 2)]
    del _prime
    for k in range(Wm):
        out = one_step(k)
    torch.cuda.synchronize()
    kernel_name = nat.last_kernel()                            # the instantiation vaeq_dp_train actually launched
    regions, launch_ms, step_no = [], [], Wm
    while True:
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
        if collective:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            ev[k][0].record()          # HIP events on the stream the kernel is launched on (torch's current stream)
            out = one_step(step_no + k)
            ev[k][1].record()
        rows = torch.cat([out["loss"][:, 0, -1:], out["var_est"][:, 0, :, -1]], dim=1)             # per-run result row
        if collective:
            allrows = sweep.gather_rows(rows, R_total, rank, world, force_collective=True)         # the sweep's single gather (RCCL over xGMI)
            assert allrows.shape[0] == R_total
        torch.cuda.synchronize()
        if collective:
            dist.barrier()
        el = time.perf_counter() - t0
        if collective:
            tt = torch.tensor([el], device=device if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())                              # identical on every rank: all ranks take the same number of regions
        regions.append(el)
        launch_ms += [a.elapsed_time(b) for a, b in ev]
        step_no += K
        assert torch.isfinite(rows).all(), "non-finite training result"
        if sum(regions) >= args.min_seconds or len(regions) >= 200:
            break
    el = float(np.median(regions))
    kern_ms = float(np.median(launch_ms))                     # the MEDIAN launch of the timed regions prices the roofline, like `value` takes the median
    kern_ms_mean = float(np.mean(launch_ms))                  # region (one cold launch no longer puts kernel_ms above ms_per_step); the mean -- the statistic
                                                              # rocprofv3's kernel stats report -- is given next to it
    dumped = dump_outputs(out, eng, args.dump_outputs) if args.dump_outputs and rank == 0 else None

    if rank == 0:
        sym_per_launch = R * CFG["N_frame_max"]
        value = R_total * CFG["N_frame_max"] * K / el
        achieved = ALGO_BYTES_PER_DP_SYMBOL * sym_per_launch / (kern_ms * 1e-3) / 1e9
        rate_k = sym_per_launch / (kern_ms * 1e-3)
        traffic, why = None, "profiles/pmc_traffic.json is missing"
        tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tj):
            try:
                d = json.load(open(tj))
                mism = [f"{k}: profiled {d.get(k)!r}, this run {v!r}" for k, v in (("runs", R), ("threads", args.threads), ("kernel", kernel_name)) if d.get(k) != v]
                if args.config5:
                    mism.append("workload: profiled the default workload, this run --config5")
                if mism:                                       # not the launch that was profiled: say so instead of quoting a stale figure
                    why = "profiles/pmc_traffic.json is of another launch (" + "; ".join(mism) + ")"
                else:
                    traffic, why = d.get("hbm_bytes_per_launch"), None
            except Exception as e:
                why = f"profiles/pmc_traffic.json unreadable: {e}"
        extras = world == 1 and not args.no_extras and not args.config5
        copy_gbs = stream_copy_gbs(device) if extras else None
        if args.config5:
            workload = (f"SURVEY config 5, saturation variant: optical DP 64-QAM + PCS VAE-LE, nu in {{0, .0270955, .0872449, .1222578}} x SNR in {{20..28}} dB x "
                        f"lr in {{2.5e-3,2e-3,3e-3}} x iter {args.iter} = {R_total} runs in total, run r on rank r mod {world}; h0, 90 GBd, M_est=25, batch_len=100, "
                        "N_frame_max=10000 (100 minibatch steps per bench step)")
        else:
            workload = ("SURVEY config 3: optical DP 64-QAM VAE-LE, nu=0, SNR 23 dB, h0, 90 GBd, M_est=25, batch_len=100, "
                        "N_frame_max=10000 (100 minibatch steps per bench step), lr in {2.5e-3,2e-3,3e-3}; seed axis raised to "
                        f"{R} independent runs per GPU (script default iter=5 -> 15 runs)")
        res = {
            "metric": "equalized symbols/s/GPU, DP 64-QAM VAE-LE", "value": value, "unit": "DP-symbols/s (1 DP symbol = 2 polarisation symbols)",
            "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": el / K * 1e3, "higher_is_better": True, "scaling": "strong" if args.config5 else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic (on-device DP channel simulator vaeq_gen_dp_*: Philox PCS draw, RRC, CD+PMD+rotation in the frequency domain, AWGN)",
            "per_gpu": value / world,
            "timed_regions": len(regions), "region_ms": {"min": min(regions) * 1e3, "median": el * 1e3, "max": max(regions) * 1e3},
            "config": {"workload": workload,
                       "runs_per_gpu": R, "runs_total": R_total, "resident_runs_per_gpu": resident, "dp_symbols_per_step_per_gpu": sym_per_launch,
                       "kernel_choice": args.threads,
                       "distinct_frames": n_distinct, "parallelism": f"sweep-sharded x{world}, one all_gather of result rows per timed region"
                                                                      + (f" ({dist.get_backend()})" if collective else "")},
            "parity": parity,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this launch, tools/profile_traffic.sh)" if traffic else None,
                         "traffic_dropped_because": why,
                         "kernel": kernel_name, "kernel_ms": kern_ms, "kernel_ms_statistic": "median of the timed launches (HIP events)", "kernel_ms_mean": kern_ms_mean,
                         "kernel_ms_minmax": [min(launch_ms), max(launch_ms)],
                         "launches_timed": len(launch_ms),
                         "algorithmic_bytes_per_launch": ALGO_BYTES_PER_DP_SYMBOL * sym_per_launch,
                         "peak_measured_copy": copy_gbs, "frac_of_measured_copy": (achieved / copy_gbs) if copy_gbs else None,
                         "flop_frac": ISSUED_FMA_FLOPS_PER_DP_SYMBOL * rate_k / 1e12 / FP32_PEAK_TFLOPS, "flop_peak_tflops": FP32_PEAK_TFLOPS,
                         "flops_per_dp_symbol": ISSUED_FMA_FLOPS_PER_DP_SYMBOL,
                         "flop_frac_algorithmic": ALGO_FLOPS_PER_DP_SYMBOL * rate_k / 1e12 / FP32_PEAK_TFLOPS,
                         "algorithmic_flops_per_dp_symbol": ALGO_FLOPS_PER_DP_SYMBOL,
                         "binds": "fp32 VALU issue + LDS (45 flop/B is above the 20 flop/B ridge); the HBM fraction is reported because north_star declares it"},
        }
        if dumped:
            res["dumped_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        if not args.no_cpu_baseline and world == 1 and not args.config5:      # reported baseline: rank 0 at N = 1 only
            # The CPU leg (~12 s of OpenMP work) runs in a thread WHILE the GPU keeps executing the headline launch back to back (untimed for `value`,
            # reported as extra.sustained): the GPU is busy for the whole invocation and the line also says what ten seconds of sustained load reach.
            import threading
            cores = host_cores()
            box = {}
            frame0 = frames[0]
            th = threading.Thread(target=lambda: box.update(r=cpu_baseline(frame0, t, var, lr, args.cpu_seconds, max(1, cores - 1),
                                                                            note="; one host core was left to the thread that kept the GPU busy meanwhile")))
            t0 = time.perf_counter()
            th.start()
            sus_ms, nl = [], 0
            while th.is_alive():
                sus_ms += _event_ms(lambda: one_step(nl), 8)
                nl += 8
            th.join()
            wall = time.perf_counter() - t0
            res["cpu_baseline"] = box["r"]
            if extras:
                res.setdefault("extra", {})["sustained"] = {"seconds": wall, "launches": nl, "kernel_ms_median": float(np.median(sus_ms)),
                                                            "kernel_ms_mean": float(np.mean(sus_ms)), "dp_symbols_per_s": nl * sym_per_launch / wall,
                                                            "note": "the headline launch back to back (host-enqueued in groups of 8) while the CPU baseline leg runs"}
        if extras:
            del out, eng
            torch.cuda.empty_cache()
            res.setdefault("extra", {})["pipeline"] = extra_pipeline(R, t, var, device)
            res["extra"]["pipeline_small"] = extra_pipeline_small(device)
            res["extra"]["configs"] = extra_configs(R, t, var, frames[0], device)
        print(json.dumps(res), flush=True)
    if collective:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

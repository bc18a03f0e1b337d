#!/usr/bin/env python3
"""Time per step of the reference-style VAE-NN loop on the module path (Net / Net_BN forward on vaeq_nn_enc_forward, loss_function,
backward() through vaeq_awgn_loss_bwd and vaeq_nn_enc_backward, torch.optim.Adam(amsgrad=True).step()) at the sweep script's shape
(64-QAM, batch_len 300, sps 2, k1 25, k2 3, M 25), next to the fused vaeq_nn_train time per run-step at R = 1 and at R runs.
The module loop is one run, one workgroup and several launches per step: it is launch-bound, the ratio to the fused kernel is expected to be large.
python tools/probe_nn_module.py [R] [net: Net | Net_BN]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from vae_equalizer_amd.engine import NNEngine
from vae_equalizer_amd.func_VAENN_MQAM import Net, Net_BN, loss_function, vaenn_tables
R = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
bn = len(sys.argv) > 2 and sys.argv[2] == "Net_BN"
dev, sps, B, M, k1, k2, steps = "cuda:0", 2, 300, 25, 25, 3, 13
t = vaenn_tables("64-QAM", "h1", sps)
amp = torch.tensor(t["amps"], dtype=torch.float32, device=dev)
torch.manual_seed(1)
rx = 0.5 * torch.randn(2, steps * B * sps, device=dev)
net = (Net_BN if bn else Net)(k1, k2, len(t["amps"]), sps).to(dev)
h_est = torch.zeros(2, M, device=dev); h_est[0, M // 2] = 1; h_est.requires_grad_(True)
opt = torch.optim.Adam(net.parameters(), lr=1e-3, amsgrad=True)
opt.add_param_group({"params": h_est})
minibatch = torch.empty(1, 2, B * sps, device=dev)


def epoch():
    net.train()
    for m in range(steps):
        opt.zero_grad()
        minibatch[0, :, :] = rx[:, m * B * sps:(m + 1) * B * sps]
        loss = loss_function(net(minibatch).squeeze(), minibatch.squeeze(), h_est, dev, amp)
        loss.backward()
        opt.step()


def wall(fn, warm=3, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


med, lo, hi = wall(epoch)
print(f"module loop ({'Net_BN' if bn else 'Net'}, 1 run): {med / steps * 1e6:.0f} us/step (median of 7 x {steps} steps; min {lo / steps * 1e6:.0f}, max {hi / steps * 1e6:.0f})", flush=True)
for r in (1, R):
    eng = NNEngine(r, M, k1, k2, t["amps"], dev, sps, batch_norm=bn)
    eng.init_parameters()
    rxr = rx[None].expand(r, -1, -1).contiguous()
    med, lo, hi = wall(lambda: eng.train(rxr, B, steps, 1e-3))
    print(f"fused vaeq_nn_train, {r} runs: {med / steps * 1e6:.1f} us/step per launch = {med / steps / r * 1e6:.3f} us per run-step (min {lo / steps * 1e6:.1f}, max {hi / steps * 1e6:.1f})", flush=True)

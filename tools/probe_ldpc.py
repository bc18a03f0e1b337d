#!/usr/bin/env python3
"""Time vaeq_ldpc_decode (GPU) at the size of a sweep: --runs runs x the codewords of one --symbols-symbol DP 64-QAM frame (w = 12 planes) under
array_code(4, 24, 211) (n = 5064, 20 256 edges), at three noise levels that take about 1, about 5 and all 20 iterations.

    python tools/probe_ldpc.py [--runs 8192] [--symbols 10000] [--sigmas 0.3,0.53,0.8] [--rounds 5] [--depth D] [--out profiles/ldpc/probe.txt]

--depth D times vaeq_ldpc_decode_il instead: the same decoder behind the symbol interleaver over groups of D codewords (codewords of whole symbols:
23 of 422 symbols in the default frame, as many as the contiguous form packs into it).

The LLRs are synthetic, generated on the device from a seed: random TX bits, llr = 2 y / sigma^2 of y = (1 - 2 b) + sigma noise (the inputs of
tests/_ref_ldpc.py).  Per level, after a warm-up call, --rounds calls between device events (host wrapper + kernel): median / min / max, codewords/s
and decoded Gbit/s (n bits per codeword) at the median, the iterations the call executed (mean and histogram corners), and the share of the LDS
floor: edges x 8 B (one 4-byte read and one 4-byte write of L per edge) x executed iterations over the chip's LDS bandwidth, 256 CUs x 256 B/clk x
2.4 GHz = 157 TB/s (MI355X_MICROARCH.md, LDS: "64 dwords wide per clock"; its measured aggregate is ~150 TB/s for 8- and 16-byte reads and ~75 TB/s
for the 4-byte reads this kernel issues, 38-51 TB/s for stores).  The kernel itself moves 16 B per edge and iteration (the first pass of a layer
reads L, the second reads and writes it, the syndrome test reads it once more) plus 16 B per check of messages.
Also printed: the LDS bytes of a workgroup and the workgroups a CU holds (160 KiB of LDS, 32 waves; the kernel's registers allow 8 waves per SIMD).
One JSON line per level."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vae_equalizer_amd import _native as nat  # noqa: E402
from vae_equalizer_amd import engine  # noqa: E402

LDS_BPS = 256 * 256 * 2.4e9                                # CUs x B/clk/CU x Hz
LDS_PER_CU, WAVES_PER_CU, STATIC_LDS = 160 * 1024, 32, 272


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--sigmas", default="0.3,0.53,0.8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ldpc", "probe.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    code = engine.array_code(4, 24, 211)
    w, R, N = 12, a.runs, a.symbols
    C_ = N * w // code.n if a.depth is None else N // -(-code.n // w)
    kw = dict(max_iter=a.max_iter) if a.depth is None else dict(max_iter=a.max_iter, depth=a.depth)
    entry = "vaeq_ldpc_decode" if a.depth is None else f"vaeq_ldpc_decode_il at depth {a.depth}"
    edges = int((code.shifts >= 0).sum()) * code.Z
    lds = int(nat.lib().vaeq_ldpc_lds_bytes(code.mb, code.nb, code.Z)) + STATIC_LDS
    waves = (code.Z + 63) // 64
    lines = [f"# {entry}: {R} runs x {C_} codewords of array_code(4, 24, 211), n = {code.n}, {edges} edges, w = {w}, {N} symbols, "
             f"max_iter {a.max_iter}, alpha 0.75; {torch.cuda.get_device_name(dev)}",
             f"# workgroup: {waves * 64} threads, {lds} B of LDS -> {min(LDS_PER_CU // lds, WAVES_PER_CU // waves)} workgroups per CU "
             f"(LDS allows {LDS_PER_CU // lds}, the 32 waves of a CU {WAVES_PER_CU // waves})"]
    print("\n".join(lines), flush=True)
    llr = torch.empty(R, w, N, dtype=torch.float32, device=dev)
    for k, sigma in enumerate(float(s) for s in a.sigmas.split(",")):
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, (R, w, N), dtype=torch.int8, device=dev, generator=g)
        llr.normal_(generator=g).mul_(sigma).add_(1.0).sub_(bits, alpha=2.0).mul_(2.0 / sigma ** 2)
        res = engine.ldpc_decode(llr, bits, code, **kw)                               # warm-up; its figures are the level's
        torch.cuda.synchronize()
        times = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            engine.ldpc_decode(llr, bits, code, **kw)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        it = res["iters"].double()
        med = statistics.median(times)
        floor_ms = edges * 8.0 * float(it.sum()) / LDS_BPS * 1e3
        line = json.dumps(dict(sigma=sigma, codewords=R * C_, unit="ms per call (host wrapper + kernel, device events)", median=round(med, 3),
                               min=round(min(times), 3), max=round(max(times), 3), rounds=a.rounds,
                               codewords_per_s=round(R * C_ / med * 1e3), decoded_Gbit_per_s=round(R * C_ * code.n / med / 1e6, 2),
                               iters_mean=round(float(it.mean()), 3), iters_min=int(it.min()), iters_max=int(it.max()),
                               ok_share=round(float(res["ok"].double().mean()), 4), BER_pre=float(res["BER_pre"].double().mean()),
                               BER_post=float(res["BER_post"].double().mean()), FER=float(res["FER"].double().mean()),
                               lds_floor_ms=round(floor_ms, 3), share_of_lds_floor=round(floor_ms / med, 4)))
        print(line, flush=True)
        lines.append(line)
        del bits, res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time vaeq_ldpc_decode (GPU) at the size of a sweep: --runs runs x the codewords of one --symbols-symbol DP 64-QAM frame (w = 12 planes) under
array_code(4, 24, 211) (n = 5064, 20 256 edges), at three noise levels that take about 1, about 5 and all 20 iterations.

    python tools/probe_ldpc.py [--runs 8192] [--symbols 10000] [--sigmas 0.3,0.53,0.8] [--rounds 5] [--depth D] [--quant BITS] [--out profiles/ldpc/probe.txt]

--depth D times vaeq_ldpc_decode_il instead: the same decoder behind the symbol interleaver over groups of D codewords (codewords of whole symbols:
23 of 422 symbols in the default frame, as many as the contiguous form packs into it).

--quant BITS times vaeq_ldpc_decode_q, the fixed-point decoder at BITS-bit LLRs and messages with engine.ldpc_decode's defaults (with --depth:
behind the interleaver), and the float32 call on the same tensors before and after it in the same session: three tables, written to
profiles/ldpc_quant/probe.txt unless --out says otherwise.  The two decoders execute different numbers of iterations on the same input, so every
line also carries ms per executed iteration (median / the mean over the codewords of iters: what a call costs per sweep of the code).

The LLRs are synthetic, generated on the device from a seed: random TX bits, llr = 2 y / sigma^2 of y = (1 - 2 b) + sigma noise (the inputs of
tests/_ref_ldpc.py).  Per level, after a warm-up call, --rounds calls between device events (host wrapper + kernel): median / min / max, codewords/s
and decoded Gbit/s (n bits per codeword) at the median, the iterations the call executed (mean and histogram corners), and the share of the LDS
floor: edges x 8 B (one 4-byte read and one 4-byte write of L per edge) x executed iterations over the chip's LDS bandwidth, 256 CUs x 256 B/clk x
2.4 GHz = 157 TB/s (MI355X_MICROARCH.md, LDS: "64 dwords wide per clock"; its measured aggregate is ~150 TB/s for 8- and 16-byte reads and ~75 TB/s
for the 4-byte reads this kernel issues, 38-51 TB/s for stores).  The kernel itself moves 16 B per edge and iteration (the first pass of a layer
reads L, the second reads and writes it, the syndrome test reads it once more) plus 16 B per check of messages.
Also printed: the LDS bytes of a workgroup and the workgroups per CU that LDS (160 KiB), waves (32 per CU) and registers (512 VGPRs per lane of a
SIMD, four SIMDs; the kernels' VGPR counts are those of profiles/ldpc_quant/scan_isa.txt) each allow.
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
VGPRS = {"float": 124, "quant": 94}                        # profiles/ldpc_quant/scan_isa.txt


def table(a, code, llr_of, quant):
    """The header and one JSON line per level of one entry point (quant: None = float32, else engine.ldpc_decode's quant dict)."""
    dev = torch.device("cuda", 0)
    w, R, N = 12, a.runs, a.symbols
    C_ = N * w // code.n if a.depth is None else N // -(-code.n // w)
    kw = dict(max_iter=a.max_iter) if a.depth is None else dict(max_iter=a.max_iter, depth=a.depth)
    if quant is None:
        entry = "vaeq_ldpc_decode" if a.depth is None else f"vaeq_ldpc_decode_il at depth {a.depth}"
        lds, rule = int(nat.lib().vaeq_ldpc_lds_bytes(code.mb, code.nb, code.Z)) + STATIC_LDS, "alpha 0.75"
    else:
        kw["quant"] = quant
        q = engine.resolve_quant(quant)
        entry = f"vaeq_ldpc_decode_q at depth {a.depth or 0}"
        lds = int(nat.lib().vaeq_ldpc_q_lds_bytes(code.mb, code.nb, code.Z)) + STATIC_LDS
        rule = f"{q['bits']}-bit LLRs and messages, {q['app_bits']}-bit a-posteriori values, scale {q['scale']}, num {q['num']}, beta {q['beta']}"
    edges = int((code.shifts >= 0).sum()) * code.Z
    waves = (code.Z + 63) // 64
    by_regs = 512 // ((VGPRS["float" if quant is None else "quant"] + 7) // 8 * 8) * 4 // waves
    lines = [f"# {entry}: {R} runs x {C_} codewords of array_code(4, 24, 211), n = {code.n}, {edges} edges, w = {w}, {N} symbols, "
             f"max_iter {a.max_iter}, {rule}; {torch.cuda.get_device_name(dev)}",
             f"# workgroup: {waves * 64} threads, {lds} B of LDS -> {min(LDS_PER_CU // lds, WAVES_PER_CU // waves, by_regs)} workgroups per CU "
             f"(LDS allows {LDS_PER_CU // lds}, the 32 waves of a CU {WAVES_PER_CU // waves}, "
             f"the {VGPRS['float' if quant is None else 'quant']} VGPRs of the kernel {by_regs})"]
    print("\n".join(lines), flush=True)
    for k, sigma in enumerate(float(s) for s in a.sigmas.split(",")):
        llr, bits = llr_of(k, sigma)
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
                               ms_per_executed_iteration=round(med / max(float(it.mean()), 1e-9), 3),
                               ok_share=round(float(res["ok"].double().mean()), 4), BER_pre=float(res["BER_pre"].double().mean()),
                               BER_post=float(res["BER_post"].double().mean()), FER=float(res["FER"].double().mean()),
                               erased_share=round(float(res["erased"].double().mean()) / code.n, 5),
                               lds_floor_ms=round(floor_ms, 3), share_of_lds_floor=round(floor_ms / med, 4)))
        print(line, flush=True)
        lines.append(line)
        del bits, res
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--sigmas", default="0.3,0.53,0.8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--quant", type=int, default=None, metavar="BITS")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = a.out or os.path.join(root, "profiles", "ldpc" if a.quant is None else "ldpc_quant", "probe.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    code = engine.array_code(4, 24, 211)
    llr = torch.empty(a.runs, 12, a.symbols, dtype=torch.float32, device=dev)

    def llr_of(k, sigma):                                      # the level's tensors, the same for every table (llr is one buffer, refilled)
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        llr.normal_(generator=g).mul_(sigma).add_(1.0).sub_(bits, alpha=2.0).mul_(2.0 / sigma ** 2)
        return llr, bits

    if a.quant is None:
        lines = table(a, code, llr_of, None)
    else:
        lines = ["## float32, before"] + table(a, code, llr_of, None)
        lines += ["", f"## fixed point, {a.quant} bits"] + table(a, code, llr_of, dict(bits=a.quant))
        lines += ["", "## float32, after"] + table(a, code, llr_of, None)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

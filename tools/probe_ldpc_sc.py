#!/usr/bin/env python3
"""Time vaeq_ldpc_sc_decode (GPU), the sliding-window decoder of spatially coupled LDPC chains, at the size of a sweep: --runs runs x one chain of
sc_array_code(3, 6, 101, 198) (rate 5/6 in the limit, column weight 4, row weight 24; 119 988 of the 120 000 bits of a 10 000-symbol DP 64-QAM
frame, w = 12 planes) at window 8 and at most 10 iterations per position, at three noise levels.

    python tools/probe_ldpc_sc.py [--runs 8192] [--symbols 10000] [--sigmas 0.3,0.53,0.8] [--rounds 5] [--window 8] [--iters 10] [--out profiles/ldpc_sc/probe.txt]
    python tools/probe_ldpc_sc.py --quant 5 [--windows 4,6,8,12] [--vgprs 206,142] [--out profiles/ldpc_sc_q/probe.txt]

The yardstick is the block decoder in the same session: engine.ldpc_decode with array_code(4, 24, 211) (the workload of tools/probe_ldpc.py) on
the same tensors, before and after the window decoder.  The two execute different amounts of work on the same input, so every line carries the
executed edge-iterations of the call -- for the block decoder iters x edges summed over the codewords, for the window decoder the iterations of
each position x the edges of the rows active there, summed over positions and chains (from pos_iters of a call of its own) -- and ms per 1e9 of
them: what one visit of one edge costs in each kernel.

The LLRs are synthetic, generated on the device from a seed as in tools/probe_ldpc.py.  Per level, after a warm-up call, --rounds calls between
device events (host wrapper + kernel): median / min / max.  One JSON line per level and decoder.

--quant BITS is the fixed-point leg instead: vaeq_ldpc_sc_decode_q at BITS-bit LLRs and messages with engine.ldpc_sc_decode's quant defaults against
the float window kernel, the yardstick here, in the same process on the same tensors, per noise level and per window of --windows.  The two
decoders take different numbers of iterations on the same input, so their milliseconds do not compare: the ms per 1e9 executed edge-iterations
do.  Every line also carries the workgroups of two waves that fit a CU by LDS (160 KiB; the dynamic state plus 432 bytes of static LDS) and by
VGPRs (--vgprs: the float and the fixed-point kernel's counts from the assembly, profiles/ldpc_sc_q/scan_isa.txt; 512 per lane, in steps of 8)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vae_equalizer_amd import _native as nat  # noqa: E402
from vae_equalizer_amd import engine  # noqa: E402


def timed(f, rounds):
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def figures(res, n):
    return dict(ok_share=round(float(res["ok"].double().mean()), 4), BER_pre=float(res["BER_pre"].double().mean()),
                BER_post=float(res["BER_post"].double().mean()), FER=float(res["FER"].double().mean()))


def block_table(a, code, levels, tag):
    w, R, N = 12, a.runs, a.symbols
    C_ = N * w // code.n
    edges = int((code.shifts >= 0).sum()) * code.Z
    lines = [f"## {tag}", f"# vaeq_ldpc_decode: {R} runs x {C_} codewords of array_code(4, 24, 211), n = {code.n}, {edges} edges, max_iter 20, alpha 0.75"]
    print("\n".join(lines), flush=True)
    for k, sigma in levels:
        llr, bits = a.llr_of(k, sigma)
        res = engine.ldpc_decode(llr, bits, code, max_iter=20)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: engine.ldpc_decode(llr, bits, code, max_iter=20), a.rounds)
        work = float(res["iters"].double().sum()) * edges
        line = json.dumps(dict(decoder="block", sigma=sigma, codewords=R * C_, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                               iters_mean=round(float(res["iters"].double().mean()), 3), edge_iterations=work,
                               ms_per_1e9_edge_iterations=round(med / work * 1e9, 4) if work else None, **figures(res, code.n)))
        print(line, flush=True)
        lines.append(line)
        del bits, res
    return lines


def window_table(a, code, levels):
    R, W = a.runs, a.window
    rows = code.L + code.ms
    wt = (code.coupled().shifts >= 0).sum(1).reshape(rows, code.mb).sum(1) * code.Z                  # edges of row block t
    P = max(1, rows - W + 1)
    active = np.array([wt[p:min(p + W, rows)].sum() for p in range(P)], np.float64)               # edges of the rows active at position p
    lds = int(nat.lib().vaeq_ldpc_sc_lds_bytes(code.ms, code.mb, code.nb, code.Z, W))
    lines = ["## window decoder",
             f"# vaeq_ldpc_sc_decode: {R} runs x 1 chain of sc_array_code({code.ms}, {code.nb}, {code.Z}, {code.L}), n_chain = {code.n}, "
             f"{int(wt.sum())} edges, design rate {code.rate:.4f}, window {W}, {P} positions, at most {a.iters} iterations per position, "
             f"test = ms + 1, alpha 0.75; {lds} B of LDS per workgroup of {(code.Z + 63) // 64 * 64} threads; {torch.cuda.get_device_name(0)}"]
    print("\n".join(lines), flush=True)
    act = torch.from_numpy(active).cuda()
    for k, sigma in levels:
        llr, bits = a.llr_of(k, sigma)
        res = engine.ldpc_sc_decode(llr, bits, code, W, chains=1, iters=a.iters, want_profile=True)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: engine.ldpc_sc_decode(llr, bits, code, W, chains=1, iters=a.iters), a.rounds)
        pi = res["pos_iters"].double()
        work = float((pi * act).sum())
        wave = res["pos_err"].double().mean((0, 1))
        line = json.dumps(dict(decoder="window", sigma=sigma, chains=R, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                               iters_per_position_mean=round(float(pi.mean()), 3), idle_positions_share=round(float((pi == 0).double().mean()), 4),
                               iters_max_mean=round(float(res["iters_max"].double().mean()), 3), edge_iterations=work,
                               ms_per_1e9_edge_iterations=round(med / work * 1e9, 4) if work else None,
                               decoded_Gbit_per_s=round(R * code.n / med / 1e6, 2), **figures(res, code.n),
                               errors_per_block_head_mid_tail=[round(float(wave[:8].mean()), 3), round(float(wave[8:-8].mean()), 3),
                                                               round(float(wave[-8:].mean()), 3)]))
        print(line, flush=True)
        lines.append(line)
        del bits, res
    return lines


def resident(lds, vgprs, waves):
    """workgroups of `waves` waves per CU as LDS allows, and as VGPRs allow"""
    return (160 * 1024) // (lds + 432), 4 * min(8, 512 // (-(-vgprs // 8) * 8)) // waves


def fixed_table(a, code, levels):
    R, rows = a.runs, code.L + code.ms
    wt = (code.coupled().shifts >= 0).sum(1).reshape(rows, code.mb).sum(1) * code.Z                  # edges of row block t
    quant = engine.resolve_quant(dict(bits=a.quant))
    waves = (code.Z + 63) // 64
    lines = [f"## fixed-point window decoder against the float window decoder, {torch.cuda.get_device_name(0)}",
             f"# {R} runs x 1 chain of sc_array_code({code.ms}, {code.nb}, {code.Z}, {code.L}), n_chain = {code.n}, {int(wt.sum())} edges, at most "
             f"{a.iters} iterations per position, test = ms + 1; float: alpha 0.75; fixed: {quant}; workgroups of {waves * 64} threads",
             "# ms: the median of --rounds calls of each decoder, same process, same tensors.  Iteration counts differ between the two: compare "
             "ms_per_1e9_edge_iterations only."]
    print("\n".join(lines), flush=True)
    for W in a.windows:
        P = max(1, rows - W + 1)
        act = torch.from_numpy(np.array([wt[p:min(p + W, rows)].sum() for p in range(P)], np.float64)).cuda()
        lds = [int(f(code.ms, code.mb, code.nb, code.Z, W)) for f in (nat.lib().vaeq_ldpc_sc_lds_bytes, nat.lib().vaeq_ldpc_sc_q_lds_bytes)]
        res_f, res_q = resident(lds[0], a.vgprs[0], waves), resident(lds[1], a.vgprs[1], waves)
        for k, sigma in levels:
            llr, bits = a.llr_of(k, sigma)
            row = dict(window=W, sigma=sigma, chains=R)
            for tag, kw, lds_b, res in (("float", {}, lds[0], res_f), ("fixed", dict(quant=quant), lds[1], res_q)):
                r = engine.ldpc_sc_decode(llr, bits, code, W, chains=1, iters=a.iters, want_profile=True, **kw)
                torch.cuda.synchronize()
                med, lo, hi = timed(lambda: engine.ldpc_sc_decode(llr, bits, code, W, chains=1, iters=a.iters, **kw), a.rounds)
                work = float((r["pos_iters"].double() * act).sum())
                row.update({f"{tag}_ms": round(med, 3), f"{tag}_min_ms": round(lo, 3), f"{tag}_max_ms": round(hi, 3),
                            f"{tag}_iters_per_position": round(float(r["pos_iters"].double().mean()), 3), f"{tag}_edge_iterations": work,
                            f"{tag}_ms_per_1e9_edge_iterations": round(med / work * 1e9, 4) if work else None,
                            f"{tag}_BER_post": float(r["BER_post"].double().mean()), f"{tag}_ok_share": round(float(r["ok"].double().mean()), 4),
                            f"{tag}_lds_bytes": lds_b, f"{tag}_workgroups_per_cu_by_lds": res[0], f"{tag}_workgroups_per_cu_by_vgprs": res[1]})
                del r
            a_, b_ = row["float_ms_per_1e9_edge_iterations"], row["fixed_ms_per_1e9_edge_iterations"]
            row["fixed_over_float_per_edge_iteration"] = round(b_ / a_, 4) if a_ and b_ else None
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del bits
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--sigmas", default="0.3,0.53,0.8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quant", type=int, default=None, help="the fixed-point leg at this many bits instead of the float tables")
    ap.add_argument("--windows", default="4,6,8,12", help="with --quant: the windows to time")
    ap.add_argument("--vgprs", default="206,142", help="with --quant: VGPRs of the float and of the fixed-point window kernel")
    a = ap.parse_args()
    a.windows, a.vgprs = [int(x) for x in a.windows.split(",")], [int(x) for x in a.vgprs.split(",")]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = a.out or os.path.join(root, "profiles", "ldpc_sc_q" if a.quant is not None else "ldpc_sc", "probe.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    block = engine.array_code(4, 24, 211)
    code = engine.sc_array_code(3, 6, 101, a.symbols * 12 // 606)
    llr = torch.empty(a.runs, 12, a.symbols, dtype=torch.float32, device=dev)

    def llr_of(k, sigma):                                      # the level's tensors, the same for every table (llr is one buffer, refilled)
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        llr.normal_(generator=g).mul_(sigma).add_(1.0).sub_(bits, alpha=2.0).mul_(2.0 / sigma ** 2)
        return llr, bits

    a.llr_of = llr_of
    levels = list(enumerate(float(s) for s in a.sigmas.split(",")))
    if a.quant is not None:
        lines = fixed_table(a, code, levels)
    else:
        lines = block_table(a, block, levels, "block decoder, before") + [""] + window_table(a, code, levels) + [""]
        lines += block_table(a, block, levels, "block decoder, after")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

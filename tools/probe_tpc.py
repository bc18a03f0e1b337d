#!/usr/bin/env python3
"""Time vaeq_tpc_decode (GPU), the Chase-Pyndiah turbo product decoder, at the size of a sweep: --runs runs x the 7 blocks of the extended
(128, 120)^2 product code that fit the 120 000 bits of a 10 000-symbol DP 64-QAM frame (w = 12 planes), at three synthetic pre-FEC error rates,
0 among them (every block stops after one half-iteration: the cost of the gather, one pass of rows and the stop test).

    python tools/probe_tpc.py [--runs 8192] [--symbols 10000] [--bers 0,0.01,0.02] [--patterns 4] [--iters 4] [--rounds 5] [--out profiles/tpc/probe.txt]

--out is written anew by every run; the committed file is the run with the defaults.

    python tools/probe_tpc.py --bch [--bers 0,0.01,0.02] [--bch-bers 0,0.03,0.045] [--out profiles/tpc_bch/probe.txt]

--bch measures vaeq_tpc_bch_decode on the extended (128, 113)^2 code of double-error-correcting BCH words at --bch-bers (chosen with model (1) of
tests/_ref_ebch.py: clean, a level where every block converges, one past the threshold) behind the table above, taken again in the same session
as the yardstick, and closes with the ratio of the two per block and half-iteration.

The LLRs are synthetic BPSK + AWGN LLRs generated on the device from a seed, as tools/probe_chase.py makes them: random TX bits, y = (1 - 2 b) +
sigma noise with sigma chosen so that Q(1 / sigma) is the level's bit error rate, llr = 2 y / sigma^2; at level 0 there is no noise and sigma is
the next level's.  Per level, after a warm-up call, --rounds calls between device events (host wrapper + kernel): median / min / max, with the scale
given (the kernel and its wrapper) and with the default scale (a torch reduction over |llr| in front of the kernel, what fec= runs).  Beside every
line the floor of reading llr and bits once, 5 R w N bytes, at the copy bandwidth measured in the same session with bench.py's stream_copy_gbs
(vaeq_stream_copy: read + write bytes per second of a plain 16-byte grid-stride copy); the half-iterations per block; BER_pre, BER_post,
BER_payload, FER and the share of blocks that stopped on a product codeword.  One JSON line per level."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vae_equalizer_amd import engine  # noqa: E402
from tools.probe_staircase import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--bers", default="0,0.01,0.02")
    ap.add_argument("--patterns", type=int, default=4)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bch", action="store_true")
    ap.add_argument("--bch-bers", default="0,0.03,0.045")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "tpc_bch" if a.bch else "tpc", "probe.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    w, R, N = 12, a.runs, a.symbols
    copy_gbs = bench.stream_copy_gbs(dev)
    floor_ms = 5 * R * w * N / (copy_gbs * 1e9) * 1e3
    llr = torch.empty(R, w, N, dtype=torch.float32, device=dev)
    lines, per_half = [], []
    tables = [(engine.ProductCode(engine.hamming_code(7), engine.hamming_code(7)), "vaeq_tpc_decode", a.bers)]
    if a.bch:
        tables.append((engine.ProductCode(engine.ebch_code(7), engine.ebch_code(7)), "vaeq_tpc_bch_decode", a.bch_bers))
    for code, name, bers in tables:
        per_half.append(table(a, code, name, bers, llr, g, copy_gbs, floor_ms, lines))
    if a.bch:
        ratio = [round(b / h, 3) for h, b in zip(*per_half)]
        line = json.dumps(dict(us_per_block_half_iteration_hamming=per_half[0], us_per_block_half_iteration_bch=per_half[1], bch_over_hamming=ratio,
                               note="level by level: clean, converging, past the threshold; the levels differ between the codes"))
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def table(a, code, name, bers, llr, g, copy_gbs, floor_ms, lines):
    """One code's table into lines -> us per block and half-iteration, level by level."""
    dev, (R, w, N) = llr.device, llr.shape
    C_ = N * w // code.n
    first, per_half = len(lines), []
    lines += [f"# {name}: {R} runs x {C_} blocks of the extended ({code.row.n}, {code.row.k})^2 product code, n = {code.n}, w = {w}, {N} "
             f"symbols, patterns {a.patterns}, at most {2 * a.iters} half-iterations, Pyndiah's schedules, clip 2^60; "
             f"{torch.cuda.get_device_name(dev)}",
             f"# copy bandwidth (vaeq_stream_copy, read + write): {copy_gbs:.0f} GB/s; llr and bits once: 5 x {R} x {w} x {N} B = "
             f"{5 * R * w * N / 1e9:.3f} GB -> floor {floor_ms:.3f} ms"]
    print("\n".join(lines[first:]), flush=True)
    bers = [float(x) for x in bers.split(",")]
    for k, ber in enumerate(bers):
        noisy = ber if ber > 0 else min(b for b in bers if b > 0)
        sigma = 1.0 / statistics.NormalDist().inv_cdf(1.0 - noisy)
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        if ber > 0:
            llr.normal_(0.0, sigma, generator=g)
        else:
            llr.zero_()
        llr.add_(1.0 - 2.0 * bits.float()).mul_(2.0 / sigma ** 2)
        kw = dict(iters=a.iters, patterns=a.patterns)
        res = engine.tpc_decode(llr, bits, code, **kw)
        torch.cuda.synchronize()
        scale = res["scale"]
        fig = dict(half_iterations_per_block=round(float(res["iters"].double().mean()), 3), ok_share=round(float(res["ok"].double().mean()), 4),
                   BER_pre=float(res["BER_pre"].double().mean()), BER_post=float(res["BER_post"].double().mean()),
                   BER_payload=float(res["BER_payload"].double().mean()), FER=float(res["FER"].double().mean()),
                   nbeta_share=round(float(res["nbeta"].double().sum() / (res["iters"].double().sum() * code.n)), 4),
                   scale_mean=round(float(scale.double().mean()), 4))
        del res
        t = timed(lambda: engine.tpc_decode(llr, bits, code, scale=scale, **kw), a.rounds)
        td = timed(lambda: engine.tpc_decode(llr, bits, code, **kw), a.rounds)
        line = json.dumps(dict(ber=ber, sigma=round(sigma, 5), blocks=R * C_, **t, floor_ms=round(floor_ms, 3),
                               floor_share=round(floor_ms / t["median_ms"], 4), default_scale_median_ms=td["median_ms"],
                               default_scale_min_ms=td["min_ms"], default_scale_max_ms=td["max_ms"],
                               us_per_block_half_iteration=round(t["median_ms"] * 1e3 / (R * C_ * fig["half_iterations_per_block"]), 4), **fig))
        print(line, flush=True)
        lines.append(line)
        per_half.append(round(t["median_ms"] * 1e3 / (R * C_ * fig["half_iterations_per_block"]), 4))
        del bits
    return per_half


if __name__ == "__main__":
    main()

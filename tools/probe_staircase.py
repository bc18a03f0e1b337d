#!/usr/bin/env python3
"""Time vaeq_staircase_decode (GPU), the hard-decision staircase decoder, at the size of a sweep: --runs runs x one chain of
StaircaseCode(BchCode(8, 3, n=240), 8) (eight 120 x 120 blocks, 115 200 of the 120 000 bits of a 10 000-symbol DP 64-QAM frame, w = 12 planes,
rate 0.8) at window 4 and at most 8 iterations per position, at three synthetic pre-FEC error rates: clean, near the threshold and stalled.

    python tools/probe_staircase.py [--runs 8192] [--symbols 10000] [--rates 0.005,0.01,0.02] [--rounds 5] [--window 4] [--iters 8] [--out profiles/staircase/probe.txt]
    python tools/probe_staircase.py --rates 0 --out profiles/staircase/probe_clean.txt

--out is written anew by every run: the two committed files are these two runs.  The second is the same call with no error at all: the gathers,
the window moves and one clean syndrome pass per pair.

The LLRs are synthetic, generated on the device from a seed: random TX bits, every bit wrong with the level's probability, magnitudes in 0.5 .. 4.5.
Per level, after a warm-up call, --rounds calls between device events (host wrapper + kernel): median / min / max.  Beside every line the floor of
reading llr and bits once, 5 R w N bytes, at the copy bandwidth measured in the same session with bench.py's stream_copy_gbs (vaeq_stream_copy:
read + write bytes per second of a plain 16-byte grid-stride copy), the figures the call returns, and the component decodes the schedule executed
(the iterations of each position x the pairs active there x s) with the milliseconds per million pair steps.  One JSON line per level."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vae_equalizer_amd import _native as nat  # noqa: E402
from vae_equalizer_amd import engine  # noqa: E402


def timed(f, rounds):
    f()                                                        # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--rates", default="0.005,0.01,0.02")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staircase", "probe.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    w, R, N, W = 12, a.runs, a.symbols, a.window
    code = engine.StaircaseCode(engine.BchCode(8, 3, n=240), N * w // (120 * 120))
    bch, P = code.component, max(1, code.L - W + 1)
    pairs = torch.tensor([min(q + W, code.L) - q for q in range(P)], dtype=torch.float64, device=dev)   # the pairs active at position q
    lds = int(nat.lib().vaeq_staircase_lds_bytes(bch.m, code.s, W))
    copy_gbs = bench.stream_copy_gbs(dev)
    floor_ms = 5 * R * w * N / (copy_gbs * 1e9) * 1e3
    lines = [f"# vaeq_staircase_decode: {R} runs x 1 chain of StaircaseCode(BchCode({bch.m}, {bch.t}, n={bch.n}), {code.L}), s = {code.s}, n_chain = "
             f"{code.n}, rate {code.rate:.3f}, w = {w}, {N} symbols, window {W}, {P} positions, at most {a.iters} iterations per position; {lds} B of "
             f"LDS per workgroup of {(code.s + 63) // 64 * 64} threads; {torch.cuda.get_device_name(dev)}",
             f"# copy bandwidth (vaeq_stream_copy, read + write): {copy_gbs:.0f} GB/s; llr and bits once: 5 x {R} x {w} x {N} B = "
             f"{5 * R * w * N / 1e9:.3f} GB -> floor {floor_ms:.3f} ms"]
    print("\n".join(lines), flush=True)
    llr = torch.empty(R, w, N, dtype=torch.float32, device=dev)
    for k, rate in enumerate(float(x) for x in a.rates.split(",")):
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        llr.uniform_(0.5, 4.5, generator=g)
        wrong = torch.empty(R, w, N, dtype=torch.float32, device=dev).uniform_(generator=g) < rate
        llr.mul_(1.0 - 2.0 * (bits.bool() ^ wrong).float())
        del wrong
        res = engine.staircase_decode(llr, bits, code, W, chains=1, iters=a.iters, want_profile=True)
        torch.cuda.synchronize()
        t = timed(lambda: engine.staircase_decode(llr, bits, code, W, chains=1, iters=a.iters), a.rounds)
        steps = float((res["pos_iters"].double() * pairs).sum())                                 # pair steps executed, over all chains
        pe = res["pos_err"].double().mean((0, 1))
        line = json.dumps(dict(rate=rate, chains=R, **t, floor_ms=round(floor_ms, 3), floor_share=round(floor_ms / t["median_ms"], 4),
                               BER_pre=float(res["BER_pre"].double().mean()), BER_post=float(res["BER_post"].double().mean()),
                               FER=float(res["FER"].double().mean()), ok_share=round(float(res["ok"].double().mean()), 4),
                               iters_per_position_mean=round(float(res["pos_iters"].double().mean()), 3),
                               nflip_mean=round(float(res["nflip"].double().mean()), 2), bad_flips_mean=round(float(res["bad_flips"].double().mean()), 3),
                               errors_per_block=[round(float(x), 3) for x in pe], pair_steps=steps, component_decodes=steps * code.s,
                               ms_per_1e6_pair_steps=round(t["median_ms"] / steps * 1e6, 4) if steps else None,
                               decoded_Gbit_per_s=round(R * code.n / t["median_ms"] / 1e6, 2)))
        print(line, flush=True)
        lines.append(line)
        del bits, res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
